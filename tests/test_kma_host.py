"""CPU: the product's KMA loader (ccq_load_kma) against the oracle.

The GPU kernel compares the loader's two views per pair (rec1 of the row
sample after stripMat, rec2 of the column sample), so a direct evaluation of
cmpMats (matcmp.c:448) over those views -- sequential, in Python -- must give
the oracle's matrix bit for bit.  This pins the loader (parsing, the
stripMat stride quirk, inclusion rules, lengths) without a GPU."""
import glob
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

FILES = sorted(glob.glob(os.path.join(GOLDEN, "kma*.mat*")))


def _i32(x):
    return (x + 2**31) % 2**32 - 2**31


def _cos(x, y):
    """coscmp as the reference binary runs it: products wrap to int32, the
    sums of the squares are signed; a negative sum makes the norm NaN and the
    position is dropped (reported here as -1, which cmpMats drops too)."""
    d = 0.0
    c1 = c2 = 0
    for k in range(5):
        d += _i32(int(x[k]) * int(y[k]))
        c1 += _i32(int(x[k]) ** 2)
        c2 += _i32(int(y[k]) ** 2)
    if c1 <= 0 or c2 <= 0:
        return -1.0
    d = 1 - d / (math.sqrt(float(c1)) * math.sqrt(float(c2)))
    return 0.0 if d < 0 else d


def _l1(x, y):
    return float(sum(abs(int(x[k]) - int(y[k])) for k in range(5)))


def view_matrix(K, metric, min_depth=15, min_length=1, min_cov=0.5):
    n = K["n"]
    out = []
    f = {"cos": _cos, "l1": _l1}[metric]
    for i in range(1, n):
        for j in range(i):
            l1, l2 = int(K["len1"][i]), int(K["len2"][j])
            if l2 > l1:
                out.append(-1.0)
                continue
            dist, inc, nn = 0.0, 0, 0
            for r in range(l2):
                x, y = K["rec1"][i, r], K["rec2"][j, r]
                t1 = int(x[6]) | int(x[7]) << 16
                t2 = int(y[6]) | int(y[7]) << 16
                if min_depth <= t2:
                    nn += 1
                    if min_depth <= t1:
                        d = f(x, y)
                        if d >= 0:
                            dist += d
                            inc += 1
            assert not (nn < min_length or nn < min_cov * l2)
            out.append(-1.0 if (inc < min_length or inc < min_cov * l2) else dist)
    return np.array(out)


@pytest.mark.parametrize("tmpl,metric", [("tmpl_one", "cos"), ("tmpl_two", "cos"), ("tmpl_two", "l1")])
def test_loader_views_match_oracle(tmpl, metric):
    import ccphylo_amd as cg
    from oracle import pyoracle
    K = cg.native.load_kma(FILES, tmpl)
    D, _, inc, n = pyoracle.kma_dist(FILES, tmpl, metric=metric)
    assert K["n"] == n and (K["include"] == inc).all()
    got = view_matrix(K, metric)
    assert np.array_equal(got, D)


def _adv_files(profile, tmp_path_factory):
    """The golden adversarial sets (wrap, zero); "plain" has no golden cases and
    is written here, with the golden sets' shape and seed."""
    if profile != "plain":
        files = sorted(glob.glob(os.path.join(GOLDEN, f"adv_{profile}*.mat.gz")))
        assert len(files) == 9
        return files
    import sys
    sys.path.insert(0, GOLDEN)
    from gen_golden import kma_adversarial
    d = tmp_path_factory.mktemp("adv_plain")
    files = [str(d / f"adv_plain{k}.mat.gz") for k in range(9)]
    for k, f in enumerate(files):
        kma_adversarial(f, 400, seed=20, profile="plain", k=k)
    return files


@pytest.mark.parametrize("metric", ["cos", "l1"])
@pytest.mark.parametrize("profile,min_depth", [("wrap", 15), ("zero", 0), ("plain", 15)])
def test_loader_views_match_oracle_adversarial(tmp_path_factory, profile, min_depth, metric):
    """The same on the adversarial sets (gen_golden.kma_adversarial): counts at
    the u16 / int32 edges, zero totals under min_depth 0, leading and trailing
    insertion rows, and samples cut short -- one of them by a single row and
    without insertion rows, whose last compared row is the leftover of the
    samples loaded before it (kmamat.c, the replay of the reference's mat1)."""
    import ccphylo_amd as cg
    from oracle import pyoracle
    files = _adv_files(profile, tmp_path_factory)
    K = cg.native.load_kma(files, "x", min_depth=min_depth)
    D, _, inc, n = pyoracle.kma_dist(files, "x", metric=metric, min_depth=min_depth)
    assert K["n"] == n == 9 and (K["include"] == inc).all()
    got = view_matrix(K, metric, min_depth=min_depth)
    assert np.array_equal(got, D)
    assert (D == -1).any() and (D >= 0).any()


def test_loader_missing_file():
    import ccphylo_amd as cg
    with pytest.raises(cg.CcgError):
        cg.native.load_kma(FILES[:2] + ["/nonexistent.mat.gz"], "tmpl_one")
