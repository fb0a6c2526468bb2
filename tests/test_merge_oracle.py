"""CPU: tests/merge_oracle.py, the numpy restatement of `ccphylo merge`,
reproduces every byte the reference binary wrote for tests/golden/merge, and
-- where the reference binary is built -- its output on seeded random inputs
inside the envelope in which the reference is reliable."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import merge_oracle as mo
from conftest import GOLDEN, ROOT

MERGE = os.path.join(GOLDEN, "merge")
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")


def merge_cases():
    with open(os.path.join(MERGE, "merge.json")) as f:
        return json.load(f)["cases"]


def gz_read(name):
    with gzip.open(os.path.join(MERGE, name), "rb") as f:
        return f.read()


def case_io(c):
    """(input, weights or None, {stdout / o / n: bytes})"""
    out = {k: (gz_read(v) if v else b"") for k, v in c["outputs"].items()}
    return gz_read(c["name"] + ".phy.gz"), gz_read(c["name"] + ".w.phy.gz") if c["weights"] else None, out


def opt(c, name, default):
    return int(c["opts"][c["opts"].index(name) + 1]) if name in c["opts"] else default


def expected_outputs(c, rc, dtext, ntext):
    """where the reference puts the two texts: -o / -n files, else stdout, D first"""
    want = {"stdout": b""}
    if rc:
        return want
    want["o" if "o" in c["files"] else "stdout"] = dtext
    if ntext is not None:
        key = "n" if "n" in c["files"] else "stdout"
        want[key] = want.get(key, b"") + ntext
    return want


@pytest.mark.parametrize("c", merge_cases(), ids=lambda c: c["name"])
def test_restatement_reproduces_golden(c):
    data, wdata, out = case_io(c)
    sep = c["opts"][c["opts"].index("-S") + 1].encode() if "-S" in c["opts"] else b"\t"
    rc, err, dtext, ntext = mo.run(data, wdata, c["etype"], opt(c, "-f", 1), opt(c, "-x", 9), sep)
    assert (rc, err.decode()) == (c["rc"], c["stderr"])
    assert out == expected_outputs(c, rc, dtext, ntext)


def test_goldens_stay_inside_the_reference_envelope():
    for c in merge_cases():
        data, wdata, _ = case_io(c)
        sep = c["opts"][c["opts"].index("-S") + 1].encode() if "-S" in c["opts"] else b"\t"
        mats = mo.parse_multi(data, c["etype"], sep) + (mo.parse_multi(wdata, c["etype"], sep) if wdata else [])
        assert len(mats[0][0]) <= 63 and len({nm for names, _ in mats for nm in names}) <= 126, c["name"]
    names = {c["name"] for c in merge_cases()}
    assert {"edge126", "w_short", "w3_stdout", "never", "w_names", "sep_comma", "one_first"} <= names


def test_later_cells_start_at_plus_zero():
    """a first-matrix cell is x itself, a later cell +0 + x: the sign of zero differs"""
    D, N = np.zeros(1), np.zeros(1)
    mo.apply(D, N, [-0.0], None, [0, 1], first=True)
    assert np.signbit(D[0])
    D, N = np.zeros(1), np.zeros(1)
    mo.apply(D, N, [-0.0], None, [0, 1])
    assert not np.signbit(D[0])
    D, N = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
    mo.apply(D, N, [-3.0], [0.0], [1, 0], first=True)    # -3 * 0 = -0, N = 0 -> the close writes -1
    assert np.signbit(D[0]) and mo.close(D, N)[0] == -1


# ---------------------------------------------------------------- against the binary
VALUES = [0.0, -1.0, 2.0 / 3.0, 1e-7, 12345.678, 1e-40, 0.25, 17.0, 99.999999]   # 1e-40: a float subnormal
WEIGHTS = [0.0, 1.0, 2.0, 1500.0, 0.5, 123456.0, 3.0]


def phy_text(names, cells):
    out = ["%10d\n" % len(names)]
    k = 0
    for i, nm in enumerate(names):
        out.append(nm + "".join("\t" + repr(float(c)) for c in cells[k:k + i]) + "\n")
        k += i
    return "".join(out)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference binary is not built (oracle/_ref)")
@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_binary_on_random_inputs(seed, tmp_path):
    rng = np.random.default_rng(1000 + seed)
    # names the reference is known to keep (its name list drops the last hash bucket): the large golden's
    pool = [nm.decode() for nm in mo.parse_multi(gz_read("edge126.phy.gz"))[1][0]]
    et, weighted = (8, 4)[seed % 2], seed % 3 != 0
    nmat = int(rng.integers(2, 7))
    first = int(rng.integers(1, 64))            # <= 63 entries
    union = list(rng.permutation(pool)[:int(rng.integers(first, 127))])
    sets = [union[:first]] + [list(rng.permutation(union)[:int(rng.integers(1, min(len(union), 40) + 1))])
                              for _ in range(nmat - 1)]
    dtext = "".join(phy_text(s, rng.choice(VALUES, len(s) * (len(s) - 1) // 2)) for s in sets)
    wtext = "".join(phy_text(s, rng.choice(WEIGHTS, len(s) * (len(s) - 1) // 2)) for s in sets)
    (tmp_path / "d.phy").write_text(dtext)
    (tmp_path / "w.phy").write_text(wtext)
    prec = (9, 17)[seed % 2]
    args = [REF, "merge", "-i", str(tmp_path / "d.phy"), "-x", str(prec)] + (["-p"] if et == 4 else [])
    if weighted:
        args += ["-w", str(tmp_path / "w.phy"), "-n", str(tmp_path / "n.out")]
    p = subprocess.run(args, capture_output=True, timeout=120)
    rc, err, dt, nt = mo.run(dtext.encode(), wtext.encode() if weighted else None, et, 1, prec)
    assert (p.returncode, p.stderr) == (rc, err)
    assert p.stdout == dt
    if weighted:
        assert (tmp_path / "n.out").read_bytes() == nt
