"""CPU: the serial restatement of the reference's dbscan (tests/dbscan_oracle.py)
reproduces every golden of tests/golden/dbscan (the reference binary's output),
the host writer ccq_print_dbscan prints the reference's bytes, and the order-free
form the GPU engine runs equals the serial restatement on random matrices."""
import os

import numpy as np
import pytest

import dbscan_oracle as dbo
from conftest import GOLDEN

CASES = dbo.golden_cases()


def test_goldens_cover_the_ground():
    """What gen_dbscan_golden.py asserted, read back from its JSON."""
    assert len(CASES) >= 20
    for c in CASES:
        if not c["extreme"]:
            assert all(1 < k < n for k, n in zip(c["nclust"], c["n"])), c["name"]
    ext = [c for c in CASES if c["extreme"]]
    assert any(c["nclust"] == [1] for c in ext) and any(c["nclust"] == c["n"] for c in ext)
    withb = [c for c in CASES if c["border_attached"] + c["border_alone"]]
    assert len(withb) >= 4 and any(c["border_attached"] for c in withb) and any(c["border_alone"] for c in withb)
    assert any(c["missing_neighbours"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_golden(case):
    from ccphylo_amd import native
    e, minn, et, bs = dbo.case_options(case["args"])
    mats = native.load_phylip(os.path.join(GOLDEN, case["input"]), etype=et, byte_scale=bs)
    blocks = dbo.parse_table(case["bytes"])
    assert len(blocks) == len(mats)
    out = b""
    for (names, D), blk in zip(mats, blocks):
        N, C, nclust = dbo.dbscan(D, len(names), e, minn, et, bs)
        out += dbo.format_table(names, N, C, nclust, e, minn, header=blk[0])
    assert out == case["bytes"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_print_dbscan_byte_exact(case, tmp_path):
    from ccphylo_amd import native
    e, minn, _, _ = dbo.case_options(case["args"])
    out = b""
    for k, (header, n, nclust, names, N, C) in enumerate(dbo.parse_table(case["bytes"])):
        path = str(tmp_path / f"b{k}.txt")
        native.write_dbscan(path, names, N, C, nclust, e, minn, header=header)
        with open(path, "rb") as f:
            out += f.read()
    assert out == case["bytes"]


def random_lt(rng, n, etype, half, missing, top=12):
    """A packed LT of small values: integral or half-integral cells, some of them missing (-1; not for etype 2 / 1)."""
    m = n * (n - 1) // 2
    v = rng.integers(0, top, m).astype(np.float64)
    if half:
        v += rng.integers(0, 2, m) * 0.5
    bs = 1.0
    if etype <= 2:
        bs = 2.0 if half else 1.0
        return (v * bs).astype(dbo.ETYPES[etype]), bs
    if missing:
        v[rng.random(m) < 0.1] = -1.0
    return v.astype(dbo.ETYPES[etype]), bs


@pytest.mark.parametrize("n", [1, 2, 3, 65, 130])
def test_parallel_form_equals_serial(n):
    rng = np.random.default_rng(1000 + n)
    checked = 0
    for etype in (8, 4, 2, 1):
        for half in (False, True):
            for missing in (False, True):
                D, bs = random_lt(rng, n, etype, half, missing)
                for e in (0.0, 2.0, 5.5, 10.0, -2.0):
                    for minn in (0, 1, 2, 4, 9):
                        N, C, k = dbo.dbscan(D, n, e, minn, etype, bs)
                        Np, Cp, kp, rounds = dbo.dbscan_parallel(D, n, e, minn, etype, bs)
                        assert (N == Np).all() and (C == Cp).all() and k == kp
                        assert rounds <= max(n - 1, 1).bit_length() + 1
                        checked += 1
    assert checked == 4 * 2 * 2 * 5 * 5


def test_parallel_form_line_chain():
    """d = |i - j| at -e 1: one chain n - 1 deep, resolved in ceil(log2 n) + 1 rounds."""
    n = 1025
    i, j = np.tril_indices(n, -1)
    D = (i - j).astype(np.float64)
    N, C, k = dbo.dbscan(D, n, 1.0, 1)
    Np, Cp, kp, rounds = dbo.dbscan_parallel(D, n, 1.0, 1)
    assert k == kp == 1 and (C == 0).all() and (Cp == 0).all() and (N == Np).all()
    assert rounds <= (n - 1).bit_length() + 1
    # -N 2: the two ends have one neighbour each and are the border rows; row 0 has no
    # row part and stays alone, row 1 (core) takes it as its first neighbour all the same
    N, C, k, border = dbo.dbscan(D, n, 1.0, 2, want_border=True)
    Np, Cp, kp, _ = dbo.dbscan_parallel(D, n, 1.0, 2)
    assert border == 2 and (C == Cp).all() and k == kp == 1
    # -N 3: no row has three neighbours, so the ends and every row between are border rows
    N, C, k, border = dbo.dbscan(D, n, 1.0, 3, want_border=True)
    Np, Cp, kp, _ = dbo.dbscan_parallel(D, n, 1.0, 3)
    assert border == n and (C == Cp).all() and k == kp == n
