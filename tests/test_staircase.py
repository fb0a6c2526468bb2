"""tools/synth.staircase_packed: an alignment whose SNP distances are known in
closed form from the include mask alone (staircase_truth), checked here against
the oracle's fsacmp / fsacmpair so that the GPU tests of the dist kernels
(test_gpu_dist_slices.py) can use the closed form as their truth."""
import numpy as np
import pytest

from tools.synth import staircase_packed, staircase_pair_masks, staircase_prefix, staircase_truth


def _steps(L, n, seed):
    """q with 0, 1, L - 1, L, every word boundary +-1 that fits and duplicates
    (taxa n - 1 and n - 2 repeat taxa 0 and 1: identical pairs); q = L twice
    with different shifts (a pair that differs everywhere)."""
    rng = np.random.default_rng(seed)
    edge = [0, 1, L - 1, L, L] + [b + d for b in range(32, L + 1, 32) for d in (-1, 0, 1)]
    rest = n - 2 - 5
    if len(edge) - 5 > rest:   # more boundaries than taxa: a random subset of them
        edge = edge[:5] + [edge[5 + k] for k in sorted(rng.choice(len(edge) - 5, rest, replace=False))]
    q = [min(max(x, 0), L) for x in edge]
    q += list(rng.integers(0, L + 1, n - 2 - len(q)))
    s = list(rng.integers(1, 4, n - 2))
    s[3], s[4] = 1, 3
    return np.array(q + q[:2]), np.array(s + s[:2])


@pytest.mark.parametrize("L", [1, 31, 32, 33, 4097])
def test_staircase_truth_vs_oracle(L):
    """The closed form equals pyoracle.snp_ltd on every cell, with q = 0, 1,
    L - 1, L and duplicated taxa, with and without norm; it spans 0 (identical
    taxa) to the included count (q = L, different shifts)."""
    from oracle import pyoracle
    n = 70
    q, s = _steps(L, n, L)
    seqs, incs, inc = staircase_packed(L, q, s, seed=L, holes=0.1 if L > 1 else 0.0)
    assert seqs.shape == (n, L // 32 + 1) and incs.shape == (L // 32 + 1,)
    C = staircase_prefix(incs, L)
    assert inc == C[L] and (L == 1 or 0 < inc < L)
    T = staircase_truth(incs, L, q, s)
    D, _, oinc = pyoracle.snp_ltd(seqs, incs, n, L)
    assert oinc == inc
    assert (D == T).all()
    tri = lambda i, j: i * (i - 1) // 2 + j
    assert T[tri(n - 2, 0)] == 0 and T[tri(n - 1, 1)] == 0     # identical taxa
    assert T[tri(4, 3)] == inc and T.max() == inc              # q = L, shifts 1 and 3
    Dn, _, _ = pyoracle.snp_ltd(seqs, incs, n, L, norm=1000)
    assert (Dn == T * (1000.0 / inc)).all()                    # fsacmpthrd.c:171-176: d * (norm / inc)


def test_staircase_pair_masks():
    """Pair mode: per-taxon masks are the global holes minus one interval each,
    one taxon empty; the oracle's n is the popcount of the and-ed masks and its
    distance the closed form restricted to them (checked cell by cell from the
    unpacked bits at a small size)."""
    from oracle import pyoracle
    L, n = 1000, 20
    q, s = _steps(L, n, 3)
    seqs, incs, _ = staircase_packed(L, q, s, seed=3, holes=0.05)
    pm = staircase_pair_masks(incs, L, n, seed=4)
    assert (pm & ~incs == 0).all() and not pm[n // 2].any()
    bits = np.unpackbits(pm.astype(">u4").view(np.uint8), axis=1)[:, :L].astype(np.int64)
    assert (bits == 0).any(axis=1).all()
    D, N, _ = pyoracle.snp_ltd(seqs, pm, n, L, pair=True, min_length=1, want_n=True)
    pos = np.arange(L)
    for i in range(1, n):
        for j in range(i):
            both = bits[i] & bits[j]
            lo, hi = min(q[i], q[j]), max(q[i], q[j])
            diff = ((pos < lo) & (s[i] != s[j])) | ((pos >= lo) & (pos < hi))
            f = i * (i - 1) // 2 + j
            assert N[f] == both.sum()
            assert D[f] == ((diff & (both == 1)).sum() if both.sum() >= 1 else -1)
