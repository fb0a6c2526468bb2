"""Synthetic inputs shared by the development tools and bench.py."""
import numpy as np


def euclid(n, seed=1, dim=8):
    """Packed LT (reference order) of Euclidean distances between n random
    points in [0,1)^dim, rounded to 9 decimals like a Phylip matrix."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, dim))
    D = np.empty(n * (n - 1) // 2)
    for i in range(1, n):
        o = i * (i - 1) // 2
        D[o:o + i] = np.sqrt(((pts[:i] - pts[i]) ** 2).sum(1))
    return np.round(D * 1e9) / 1e9


def euclid_shard_dev(torch, n, rank, world, seed=4, dim=8, band=8, chunk_rows=512, dtype=None, cdist=False):
    """This rank's row bands (ccg_tree_shard_dev layout: bands of `band` rows
    dealt round-robin, owned rows back to back, row r = D(r, 0..r-1)) of the
    Euclidean distances between n points of U[0,1)^dim, computed on the GPU.
    Every rank draws the same points (CPU generator, fixed seed); computed in
    double, stored as `dtype` (default float64; float32 = `-p`).  cdist: the
    round-4 form (torch.cdist per chunk of rows), kept to reproduce that
    round's configs[3] matrix.  On this image's PyTorch-ROCm build
    torch.cdist gives wrong cells once a chunk has more than ~32k columns
    (tools/cdist_check.py, profiles/r06_generator_check.txt), so at n = 200k
    that form is not a Euclidean matrix."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand((n, dim), generator=g, dtype=torch.float64).cuda()
    nb = (n + band - 1) // band
    mine = list(range(rank, nb, world))
    sizes = [sum(range(b * band, min(b * band + band, n))) for b in mine]
    out = torch.empty(max(sum(sizes), 1), dtype=dtype or torch.float64, device="cuda")
    per = max(1, chunk_rows // band)
    pos = 0
    for c0 in range(0, len(mine), per):
        bands = mine[c0:c0 + per]
        rows_h = [r for b in bands for r in range(b * band, min(b * band + band, n))]
        rows = torch.tensor(rows_h, device="cuda")
        rmax = rows_h[-1]
        if rmax == 0:
            continue
        # elementwise, one dimension at a time: every cell's value depends on
        # its two points only (torch.cdist's may depend on the batch's shape,
        # so the ranks of a world-8 run and the world-1 LT disagreed in the
        # last bit of some cells)
        if cdist:
            d = torch.cdist(pts[rows], pts[:rmax], compute_mode="donot_use_mm_for_euclid_dist")
        else:
            a, c = pts[rows][:, None, :], pts[:rmax][None, :, :]
            t = a[..., 0] - c[..., 0]
            s2 = t * t
            for k in range(1, dim):
                t = a[..., k] - c[..., k]
                s2 = s2 + t * t
            d = torch.sqrt(s2)
        # row-major: each row's prefix, rows in order (views concatenated: a
        # boolean-mask select of this size crashed torch inside a long process)
        vals = torch.cat([d[i, :r] for i, r in enumerate(rows_h) if r > 0])
        out[pos:pos + vals.numel()] = vals
        pos += vals.numel()
    assert pos == sum(sizes)
    return out


def clade_packed(n, L, clades, seed=3, every=10, flips=8):
    """A clade-structured packed alignment in the reference's layout, numpy
    only (the same bytes on the GPU box and in the build container): `clades`
    random root sequences, taxon t = root t % clades with each bit set to 1
    with p = 2^-flips xor-ed in (~0.8% of the 2-bit codes flipped at 8), as
    tools/config3.make_packed.  Returns (seqs n x W u64, W = L // 32 + 1
    words per taxon as cdist.c:290 allocates, positions past L zero;
    incs W u32: every `every`-th word excluded (the "N columns"), the tail
    past L cleared as initIncPos does, fsacmp.c:164)."""
    W = L // 32 + 1
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, 2 ** 64, (clades, W), dtype=np.uint64, endpoint=False)
    seqs = np.empty((n, W), dtype=np.uint64)
    step = 4096
    for t0 in range(0, n, step):
        t1 = min(n, t0 + step)
        m = rng.integers(0, 2 ** 64, (t1 - t0, W), dtype=np.uint64, endpoint=False)
        for _ in range(flips - 1):
            m &= rng.integers(0, 2 ** 64, (t1 - t0, W), dtype=np.uint64, endpoint=False)
        seqs[t0:t1] = roots[np.arange(t0, t1) % clades] ^ m
    W32 = (L + 31) // 32
    seqs[:, W32:] = 0
    if L % 32:
        seqs[:, W32 - 1] &= np.uint64(((1 << (2 * (L % 32))) - 1) << (64 - 2 * (L % 32)))
    incs = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    if every:
        incs[::every] = 0
    incs[W32:] = 0
    if L % 32:
        incs[W32 - 1] &= np.uint32((0xFFFFFFFF << (32 - L % 32)) & 0xFFFFFFFF)
    return seqs, incs


def _pack_codes(codes, W):
    """2-bit codes of positions 0..len-1 into W u64 words, position p at bits
    63 - 2p .. 62 - 2p of word p // 32 (qseqs.c:60); positions past len zero."""
    pad = np.zeros(W * 32, dtype=np.uint64)
    pad[:len(codes)] = codes
    sh = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
    return np.bitwise_or.reduce(pad.reshape(W, 32) << sh, axis=1)


def staircase_packed(L, q, s, seed=5, holes=0.02):
    """A packed alignment whose every distance is known in closed form
    (staircase_truth), numpy only.  One random base sequence of L codes; taxon
    t is the base with (code + s[t]) % 4 on the positions < q[t] (0 <= q[t] <=
    L, s[t] in 1..3): a staircase of prefixes, so taxa with the same (q, s)
    are identical and two taxa with q = L and different shifts differ
    everywhere.  Built from the four packed shifts of the base by word copies
    (and one mixed word per taxon), never an n x L code array.  The global
    include mask drops each position with p = holes; its tail past L is
    cleared as in clade_packed.  Returns (seqs n x W u64, W = L // 32 + 1;
    incs W u32, include bit of position p = bit 31 - p % 32 of word p // 32;
    the included count)."""
    q = np.asarray(q, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    assert q.shape == s.shape and q.ndim == 1
    assert ((q >= 0) & (q <= L)).all() and ((s >= 1) & (s <= 3)).all()
    n, W = len(q), L // 32 + 1
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, L, dtype=np.uint64)
    forms = [_pack_codes((base + np.uint64(k)) % np.uint64(4), W) for k in range(4)]
    seqs = np.empty((n, W), dtype=np.uint64)
    for t in range(n):
        wq, r = int(q[t]) // 32, int(q[t]) % 32
        f = forms[int(s[t])]
        seqs[t, :wq] = f[:wq]
        seqs[t, wq:] = forms[0][wq:]
        if r:   # the word the step falls in: its first r positions shifted
            hm = np.uint64(((1 << (2 * r)) - 1) << (64 - 2 * r))
            seqs[t, wq] = (f[wq] & hm) | (forms[0][wq] & ~hm)
    bits = np.zeros(W * 32, dtype=np.uint8)
    bits[:L] = rng.random(L) >= holes
    incs = np.packbits(bits).view(">u4").astype(np.uint32)
    return seqs, incs, int(bits.sum())


def _lt(M):
    """Packed LT (cell (i, j), j < i, at i (i - 1) / 2 + j) of a square matrix."""
    i, j = np.tril_indices(M.shape[0], -1)
    return np.ascontiguousarray(M[i, j], dtype=np.float64)


def adv_additive(n, seed):
    """Attacks the exact row sum's binade walk and the Q tie rules: path lengths in a random binary tree whose
    branches are 10**U(-6, 6), so every cherry ties in Q but for rounding and a row's contributions span many
    binades."""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    depth = np.zeros(n)                       # leaf to the root of its present cluster
    clusters = [np.array([t]) for t in range(n)]
    while len(clusters) > 1:
        a, b = rng.choice(len(clusters), 2, replace=False)
        A, B = clusters[a], clusters[b]
        la, lb = 10.0 ** rng.uniform(-6, 6, 2)
        depth[A] += la
        depth[B] += lb
        d = depth[A][:, None] + depth[B][None, :]
        M[np.ix_(A, B)] = d
        M[np.ix_(B, A)] = d.T
        clusters[min(a, b)] = np.concatenate((A, B))
        clusters.pop(max(a, b))
    return _lt(M)


def adv_line(n, seed):
    """Attacks updateD's clamp to zero and zero limbs: |x_i - x_j| of shuffled points on a line at scales 1e-3 ..
    1e3, where (D_ik + D_kj - D_ij) / 2 is exactly 0 or a rounding residue for most k."""
    rng = np.random.default_rng(seed)
    x = rng.random(n) * 10.0 ** rng.integers(-3, 4, n)
    x = rng.permutation(x)
    return _lt(np.abs(x[:, None] - x[None, :]))


def adv_dyadic(n, seed):
    """Attacks the row sum's order-independence shortcut and half-ulp ties: cells (0..8) * 2**-(0..60), non-metric,
    so no power of two bounds a row's sum under 2^53 units and many contributions are negative before the clamp."""
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    return rng.integers(0, 9, m) * np.ldexp(1.0, -rng.integers(0, 61, m))


def adv_dupes(n, seed):
    """Attacks the index tie rules: Euclidean distances of n points drawn with replacement from n // 8 distinct
    ones, so cells are zero, rows are identical and Q ties exactly."""
    rng = np.random.default_rng(seed)
    pts = rng.random((max(n // 8, 1), 8))[rng.integers(0, max(n // 8, 1), n)]
    sq = np.zeros((n, n))
    for k in range(pts.shape[1]):   # one dimension at a time: no n x n x dim array
        t = pts[:, k][:, None] - pts[:, k][None, :]
        sq += t * t
    return _lt(np.sqrt(sq))


def adv_grid(n, seed):
    """Attacks minQpair's replay table: cells (1..100) / 100, few distinct values and non-metric, so tens of rows
    qualify for a rescan at every join."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 101, n * (n - 1) // 2) / 100.0


ADVERSARIAL = {"additive": adv_additive, "line": adv_line, "dyadic": adv_dyadic, "dupes": adv_dupes,
               "grid": adv_grid}


def staircase_prefix(incs, L):
    """C[x] = included positions < x of a packed include mask, x = 0..L (int64)."""
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    bits = np.unpackbits(incs.astype(">u4").view(np.uint8))[:L]
    C = np.zeros(L + 1, dtype=np.int64)
    np.cumsum(bits, dtype=np.int64, out=C[1:])
    return C


def staircase_truth(incs, L, q, s):
    """The packed LT (cell (i, j), j < i, at i (i - 1) / 2 + j; int64) of the
    non-pair SNP distances of staircase_packed(L, q, s) under the global mask
    incs, from the mask alone: with C the prefix count of included positions,
    dist(a, b) = [s_a != s_b] C(min q) + C(max q) - C(min q)
    (below both steps the codes differ iff the shifts do; between the steps
    one taxon is shifted and the other is not)."""
    q = np.asarray(q, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    C = staircase_prefix(incs, L)
    i, j = np.tril_indices(len(q), -1)
    lo, hi = C[np.minimum(q[i], q[j])], C[np.maximum(q[i], q[j])]
    return (s[i] != s[j]) * lo + hi - lo


def staircase_pair_masks(incs, L, n, seed=6, empty=None):
    """Per-taxon masks for pair mode (n x W u32): the global holes of incs
    and-ed with one excluded interval per taxon (up to L / 8 positions long,
    anywhere); taxon `empty` (default n // 2) is excluded entirely, so every
    pair with it has no shared position and minLength yields -1."""
    incs = np.ascontiguousarray(incs, dtype=np.uint32)
    W = len(incs)
    rng = np.random.default_rng(seed)
    out = np.tile(incs, (n, 1))
    full = np.uint64(0xFFFFFFFF)
    for t in range(n):
        ln = int(rng.integers(1, max(L // 8, 1) + 1))
        a = int(rng.integers(0, L - ln + 1))
        b = a + ln                                   # positions [a, b) excluded
        wa, wb = a // 32, (b - 1) // 32
        keep = np.full(wb - wa + 1, 0, dtype=np.uint64)
        keep[0] |= (full << np.uint64(32 - a % 32)) & full if a % 32 else np.uint64(0)        # positions before a
        keep[-1] |= full >> np.uint64(b - wb * 32) if b - wb * 32 < 32 else np.uint64(0)      # positions from b on
        out[t, wa:wb + 1] &= keep.astype(np.uint32)
    out[n // 2 if empty is None else empty] = 0
    assert out.shape == (n, W)
    return out
