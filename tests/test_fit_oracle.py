"""CPU: the Python restatement of `nwck2phy` and `phycmp` (tests/fit_oracle.py)
against the reference's bytes under tests/golden/fit (gen_fit_golden.py)."""
import gzip
import json
import os

import numpy as np
import pytest

import fit_oracle as fo
from conftest import GOLDEN

FIT = os.path.join(GOLDEN, "fit")
with open(os.path.join(FIT, "fit.json")) as f:
    CASES = json.load(f)["cases"]
NWCK = [c for c in CASES if c["cmd"] == "nwck2phy"]
PHYCMP = [c for c in CASES if c["cmd"] == "phycmp"]


def golden_out(case):
    if not case["out"]:
        return b""
    with gzip.open(os.path.join(FIT, case["out"])) as f:
        return f.read()


def flag_of(args):
    return int(args[args.index("-f") + 1]) if "-f" in args else 1


def test_case_list_covers_the_issue():
    names = {c["name"] for c in NWCK}
    for t in ("miss80_dnj", "test_hnj_f2", "adv_line_nj", "adv_dupes_dnj", "star", "trifurc", "lj_neg", "two_lines",
              "miss80_nj"):
        assert t in names and t + "_p" in names
    names = {c["name"] for c in PHYCMP}
    for t in ("self_p", "perturbed", "itself", "zero", "missing", "err_missing", "err_size", "err_entries"):
        assert t in names and t + "_p" in names
    biggest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                  if os.path.isfile(os.path.join(GOLDEN, f)))
    assert all(os.path.getsize(os.path.join(FIT, f)) <= biggest for f in os.listdir(FIT))


@pytest.mark.parametrize("case", NWCK, ids=[c["name"] for c in NWCK])
def test_nwck2phy_restatement_equals_reference_bytes(case):
    with open(os.path.join(GOLDEN, case["args"][2]), "rb") as f:
        data = f.read()
    out, rc, err = fo.nwck2phy(data, case["etype"], flag_of(case["args"]))
    assert rc == case["rc"]
    assert err.decode("latin-1") == case["stderr"]
    assert out == golden_out(case)


def test_hand_cases_take_the_paths_they_are_named_for():
    def splits(name):
        with open(os.path.join(FIT, name + ".nwk"), "rb") as f:
            return [r[2] for r in fo.parse_file(f.read())]
    star, = splits("star")
    assert all(Li == 0 for _, Li, _ in star[:2])           # remainder not bifurcating -> Li = 0
    assert [Lj for _, _, Lj in star[:2]] == [-1.0, -1.0]   # a one-digit limb is not found in a node kept one byte short
    tri, = splits("trifurc")
    assert tri[0][1] == 0 and tri[0][2] == 3.5
    a, b = splits("lj_neg")
    assert a[0] == (0, 1.5, 0.0)                           # Lj < 0 <= Li -> Lj = 0
    assert any(Li < 0 for _, Li, _ in b) and any(Lj < 0 for _, _, Lj in b)
    assert len(splits("two_lines")) == 2
    big = [r for c in ("adv_line_nj", "test_hnj_f2") for r in fo.parse_file(open(os.path.join(GOLDEN, c + ".out"), "rb").read())]
    assert any(org > 0 for r in big for org, _, _ in r[2])
    assert any(Lj < 0 or Li < 0 for r in big for _, Li, Lj in r[2])


def load(path, etype):
    from ccphylo_amd import native
    return native.load_phylip(os.path.join(GOLDEN, path), etype=etype)


@pytest.mark.parametrize("case", PHYCMP, ids=[c["name"] for c in PHYCMP])
def test_phycmp_restatement_equals_reference_lines(case):
    if case["rc"]:
        assert case["stdout"] == "" and case["stderr"] in ("Missing matrix\n", "Matrices differ in size.\n",
                                                           "Matrices has different entries.\n")
        mats = [m for f in case["files"] for m in load(f, case["etype"])]
        if case["name"].startswith("err_missing"):
            assert len(mats) == 1
        elif case["name"].startswith("err_size"):
            assert len(mats[0][0]) != len(mats[1][0])
        else:
            assert sorted(mats[0][0]) == sorted(mats[1][0]) and mats[0][0] != mats[1][0]
        return
    (n1, A), (n2, B) = [m for f in case["files"] for m in load(f, case["etype"])]
    assert n1 == n2
    n = len(n1)
    s, mags = fo.cmp_sums(A, B, case["etype"])
    assert fo.phycmp_lines(s, n * (n - 1) // 2, 127) == case["stdout"]
    assert fo.phycmp_lines(s, n * (n - 1) // 2, 1 | 8 | 64).count("\n") == 3


def test_replay_forms_agree():
    rng = np.random.default_rng(5)
    for et in (8, 4):
        sp = []
        for s in range(90):
            Li, Lj = rng.choice([-1.0, -0.5, 0.0, 0.25, 1.5, 2.0 / 3], 2)
            sp.append((int(rng.integers(0, s + 1)), float(Li), float(Lj)))
        assert (fo.replay(sp, et) == fo.replay_np(sp, et)).all()
