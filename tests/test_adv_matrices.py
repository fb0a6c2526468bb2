"""CPU: the adversarial distance-matrix generators of tools/synth.py
(ADVERSARIAL) keep the property that makes each kind hard for the tree
engines, measured with the oracle at n = 600, seed 7.  tests/test_gpu_adv_tree.py
feeds these matrices to every engine; a later edit that made a generator
benign would leave those tests green and empty, so the properties are pinned
here.  The thresholds sit well under what the generators give (the measured
value stands beside each); a generator that misses one is changed, not the
threshold."""
import numpy as np
import pytest

from tools.synth import ADVERSARIAL

N, SEED = 600, 7
KINDS = sorted(ADVERSARIAL)
_CACHE = {}


def _run(kind):
    """(D, {method: (joins, final_n, final_d, stats)}) of one kind, computed once."""
    if kind not in _CACHE:
        from oracle import pyoracle
        D = ADVERSARIAL[kind](N, SEED)
        D.setflags(write=False)
        _CACHE[kind] = (D, {m: pyoracle.tree(D, N, method=m, stats=True) for m in (0, 1, 2)})
    return _CACHE[kind]


def _first_join_contributions(kind):
    """(c, raw): updateD's contributions c_k = max((D_ik + D_kj - D_ij) / 2, 0)
    of the oracle's first DNJ join (i, j) over the other rows k, and the
    values before the clamp."""
    D, trees = _run(kind)
    i, j = int(trees[1][0]["i"][0]), int(trees[1][0]["j"][0])
    M = np.zeros((N, N))
    a, b = np.tril_indices(N, -1)
    M[a, b] = D
    M[b, a] = D
    k = np.setdiff1d(np.arange(N), [i, j])
    raw = (M[i, k] + M[k, j] - M[i, j]) / 2
    return np.maximum(raw, 0.0), raw


def _binade_span(c):
    e = np.frexp(c[c > 0])[1]
    return int(e.max() - e.min())


def _zero_limbs(kind):
    joins = _run(kind)[1][1][0]
    return int((joins["Li"] == 0).sum() + (joins["Lj"] == 0).sum())


@pytest.mark.parametrize("kind", KINDS)
def test_shape_and_determinism(kind):
    D = _run(kind)[0]
    assert D.dtype == np.float64 and D.shape == (N * (N - 1) // 2,)
    assert np.isfinite(D).all() and (D >= 0).all()
    assert (ADVERSARIAL[kind](N, SEED) == D).all()
    assert (ADVERSARIAL[kind](N, SEED + 1) != D).any()
    assert ADVERSARIAL[kind].__doc__.startswith("Attacks ")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", [0, 1, 2], ids=["nj", "dnj", "hnj"])
def test_oracle_finishes(kind, method):
    joins, fn, fd, _ = _run(kind)[1][method]
    assert fn == 2 and len(joins) == N - 2
    assert np.isfinite(joins["Li"]).all() and np.isfinite(joins["Lj"]).all() and np.isfinite(fd)


def test_additive_spans_binades():
    c, _ = _first_join_contributions("additive")
    assert _binade_span(c) >= 12   # 18


def test_dyadic_clamps_spans_and_defeats_the_shortcut():
    c, raw = _first_join_contributions("dyadic")
    assert np.mean(raw < 0) >= 0.10   # 0.61
    assert np.mean(c == 0) >= 0.10
    assert _binade_span(c) >= 20   # 24
    # the row sum's order-independence test (fold_update_wave) on these
    # contributions: with 2^e the largest power of two dividing every c_k,
    # sum(c) (1 + 1e-9) < 2^(53 + e) would prove any order exact; it must fail
    mant, ex = np.frexp(c[c > 0])
    units = (mant * 2.0 ** 53).astype(np.int64)   # exact: 53-bit mantissas
    e = int((ex - 53 + np.array([(int(u) & -int(u)).bit_length() - 1 for u in units])).min())
    assert np.abs(c).sum() * (1 + 1e-9) >= 2.0 ** (53 + e)   # e = -58


def test_line_zero_limbs():
    assert _zero_limbs("line") >= N // 4   # 310 of 1196


def test_dupes_zero_limbs():
    assert _zero_limbs("dupes") >= N // 2   # 1049 of 1196


def test_grid_rows_per_join():
    joins, _, _, stats = _run("grid")[1][1]
    assert stats[0] / len(joins) >= 20   # 40.3 (additive: 11.1)
