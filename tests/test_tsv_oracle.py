"""CPU: the numpy restatement of `ccphylo tsv2phy` (tests/tsv_oracle.py) against
the reference's bytes (tests/golden/tsv, written by gen_tsv_golden.py).  The
-x 17 outputs carry every double exactly (%.17g round-trips), so the bit-exact
metrics are compared bitwise; l<n> goes through pow() and is compared at rtol
1e-12 (the project's rule for pow metrics, tests/test_gpu_kma.py)."""
import os

import numpy as np
import pytest

import tsv_oracle as tso

TSV, CASES, PHY = tso.TSV, tso.CASES, tso.PHY
case_options, case_bytes = tso.case_options, tso.case_bytes


def test_golden_set_covers_the_issue():
    ds = {case_options(c["args"])["d"] for c in PHY}
    assert ds == {"cos", "chi2", "bc", "l1", "l2", "linf", "l3", "l2.5", "p"}
    for d in ds:
        vt = {case_options(c["args"])["vtype"] for c in PHY if case_options(c["args"])["d"] == d}
        assert vt == {8, 4}, d
    assert {c["tree"] for c in CASES if "tree" in c} == {"dnj", "nj"}


@pytest.mark.parametrize("case", PHY, ids=[c["name"] for c in PHY])
def test_restatement_matches_reference(case):
    o = case_options(case["args"])
    kind, ex = tso.parse_metric(o["d"])
    X = tso.read_tsv(os.path.join(TSV, o["inp"]), o["sep"], o["vtype"])
    D = tso.vec_ltd(X, kind, ex)
    ref = case_bytes(case)
    m, cells = tso.parse_phy(ref)
    assert m == X.shape[0] and len(cells) == len(D)
    if kind == "ln":
        np.testing.assert_allclose(D, cells, rtol=1e-12, atol=0)
        return
    if o["prec"] == 17:
        assert np.array_equal(D.view(np.uint64), cells.view(np.uint64))
    assert tso.format_phy(D, m, o["flag"], o["prec"]) == ref


def test_special_rows():
    """mix12: row 11 repeats row 0, row 1 is zero, row 2 constant."""
    X = tso.read_tsv(os.path.join(TSV, "mix12.tsv"))
    assert X.shape == (12, 37) and (X[11] == X[0]).all() and not X[1].any() and (X[2] == 1.25).all()
    i, j = np.tril_indices(12, -1)
    cos, p, l2 = tso.vec_ltd(X, "cos"), tso.vec_ltd(X, "p"), tso.vec_ltd(X, "l2")
    assert (cos[(i == 1) | (j == 1)] == -1).all()
    assert (p[(i == 1) | (j == 1) | (i == 2) | (j == 2)] == 0).all()
    assert l2[(i == 11) & (j == 0)] == 0
    assert (p < 0).any() and (p > 0).any()
    Xf = X.astype(np.float32)
    assert (tso.vec_ltd(Xf, "cos") != cos).any()   # three decimals: the float rows differ
