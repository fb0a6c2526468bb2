"""The dist kernels at forced split-K plans and at the f32-exact slice limit.

Which slice length a small shape gets from plan_split depends on the device's
CU count, and the clamp to the f32-exact slice (MFMA_KMAX words) needs shapes no
cheap test has.  Here CCG_DIST_SLICES forces the slice count, last_dist_plan()
reads the plan back so that every case asserts the path it meant to take, and
the truth is the closed form of tools/synth.staircase_packed (checked against
the oracle in test_staircase.py): it needs no code under test and its values
span 0 (identical taxa, the largest dot product) to the included count.

The four kernel choices are CCG_DIST_MFMA 0 (VALU tiles), 1 (128 x 128 MFMA)
and 2 with CCG_DIST_GLDS 0 (k_snp_mfma2) and 1 (k_snp_mfma3; pair mode runs
k_snp_mfma2_pair under both), as test_gpu.py::test_dist_mfma_equals_valu sets
them.  The plan rule (plan_split, snp.hip): the planes hold Wp words per taxon,
the included words rounded up to 16 (non-pair) or 8 (pair); a launcher cuts
them into chunks of kc words (8 for the 256 x 256 kernels and for pair mode, 16
for the non-pair 128 x 128 ones); a forced S becomes min(S, chunks) slices of
Wk = cdiv(chunks, S) kc words, clamped to the largest multiple of kc not above
MFMA_KMAX for the MFMA forms (not for the VALU tiles nor the 128 x 128 pair
form, which gives way to the VALU pair tiles at Wk >= MFMA_KMAX), and the slices
launched are cdiv(Wp, Wk).
"""
import numpy as np
import pytest

from tools.synth import staircase_packed, staircase_pair_masks, staircase_truth

pytestmark = pytest.mark.gpu

KMAX = 174762   # MFMA_KMAX: 3 * 32 * Wk < 2^24
MODES = ("0", "1", "2", "3")
ETS = (8, 4, 2, 1)
NORMS = (0, 1000)
BS = 2.0


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()
    for cache in (_sweep_data, _sweep_ref, _limit_data):   # the alignments made here (69 MB and more) end with the module
        cache.clear()


def cdiv(a, b):
    return -(-a // b)


def kc_kmax(mode, pair):
    """(the launcher's chunk, its slice clamp or 0) of a kernel choice."""
    if mode in ("2", "3"):
        return 8, KMAX
    if pair:
        return 8, 0
    return 16, KMAX if mode == "1" else 0


def plan_rule(Wp, kc, forced, kmax):
    """(S, Wk) plan_split documents for CCG_DIST_SLICES=forced."""
    chunks = Wp // kc
    Wk = cdiv(chunks, min(forced, chunks)) * kc
    if kmax and Wk > kmax:
        Wk = kmax // kc * kc
    return cdiv(Wp, Wk), Wk


def planes_words(L, pair):
    """Wp when no word of the mask is excluded entirely (asserted by the cases)."""
    W32 = (L + 31) // 32
    return cdiv(W32, 8) * 8 if pair else cdiv(W32, 16) * 16


def set_mode(monkeypatch, mode, forced):
    monkeypatch.setenv("CCG_DIST_MFMA", "2" if mode == "3" else mode)
    monkeypatch.setenv("CCG_DIST_GLDS", "1" if mode == "3" else "0")
    monkeypatch.setenv("CCG_DIST_SLICES", str(forced))
    for k in ("CCG_DIST_KC", "CCG_DIST_ORDER", "CCG_DIST_NOCOMPACT"):
        monkeypatch.delenv(k, raising=False)


class Msa:
    """A packed alignment in device memory and an output buffer or two."""

    def __init__(self, dev, seqs, incs, elems, et, want_n):
        import ccphylo_amd as cg
        self.dev, self.W, self.dt = dev, seqs.shape[1], cg.ETYPES[et]
        self.elems, self.et = elems, et
        self.ptrs = [dev.malloc(seqs.nbytes), dev.malloc(incs.nbytes), dev.malloc(max(elems, 1) * et)]
        if want_n:
            self.ptrs.append(dev.malloc(max(elems, 1) * et))
        self.ps, self.pi, self.pd = self.ptrs[:3]
        self.pn = self.ptrs[3] if want_n else None
        dev.h2d(self.ps, seqs)
        dev.h2d(self.pi, incs)

    def poison(self, elems=None):
        """0xA5 in every output byte: a cell no kernel writes cannot pass."""
        for p in (self.pd, self.pn):
            if p is not None:
                self.dev.h2d(p, np.full(max(self.elems if elems is None else elems, 1) * self.et, 0xA5, np.uint8))

    def fetch(self, p, elems=None):
        out = np.empty(self.elems if elems is None else elems, dtype=self.dt)
        if out.size:
            self.dev.d2h(out, p)
        return out

    def free(self):
        for p in self.ptrs:
            self.dev.free(p)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()


# ---------------------------------------------------------------- C2 / C3: the chunk sweep
SWEEP_N = 258   # a diagonal 256-tile, a full off-diagonal one, a two-row panel (three panels of the 128-tiles)


def sweep_L(T):
    return 32 * 8 * T - 5   # 8 T words, the last one partial


# (T, forced S): S <= T, the 8-word chunks of the alignment (the pair kernels' chunk count; the non-pair
# launchers see the words rounded up to 16, in chunks of 8 or 16: their plans take min(S, chunks))
SWEEP = [(T, S) for T in range(1, 13) for S in (1, 2, 3) if S <= T]
SWEEP_CASES = [(T, S, pair) for T, S in SWEEP for pair in (False, True)]
BAND_CASES = [(T, S, pair, world) for T in (1, 3, 5, 9) for S in (1, 3) for pair in (False, True) for world in (1, 3)]


def sweep_et_norm(T, S, pair):
    """et over 8, 4, 2, 1 and norm over 0, 1000 in turn across the cases (not a product)."""
    j = SWEEP.index((T, S)) if (T, S) in SWEEP else 3 * T + S
    return ETS[(j + pair) % 4], NORMS[(j // 4 + pair) % 2]


_sweep_data = {}


def sweep_data(T):
    """The staircase of one length, its closed-form truth and per-taxon masks (made once)."""
    if T in _sweep_data:
        return _sweep_data[T]
    L, n = sweep_L(T), SWEEP_N
    rng = np.random.default_rng(100 + T)
    # steps at every 32-, 256- and 512-position boundary +-1 (the word, the 8-word chunk, the 16-word chunk),
    # the ends, and random ones; where a long alignment has more word boundaries than taxa, every chunk
    # boundary stays and the word boundaries are a random subset
    ends = [0, 1, L - 1, L, L]
    chunk = [b + d for b in range(256, L + 2, 256) for d in (-1, 0, 1)]
    word = [b + d for b in range(32, L + 2, 32) if b % 256 for d in (-1, 0, 1)]
    room = n - 4 - len(ends) - len(chunk)
    if len(word) > room:
        word = [word[k] for k in sorted(rng.choice(len(word), room, replace=False))]
    q = [min(x, L) for x in ends + chunk + word]
    q += list(rng.integers(0, L + 1, n - 4 - len(q)))
    s = list(rng.integers(1, 4, n - 4))
    s[3], s[4] = 1, 2                     # q = L twice with different shifts: a pair that differs everywhere
    q, s = np.array(q + q[:4]), np.array(s + s[:4])   # four duplicated taxa: identical pairs
    order = rng.permutation(n)            # spread over both panels and every wave
    q, s = q[order], s[order]
    seqs, incs, inc = staircase_packed(L, q, s, seed=T, holes=0.02)
    assert (incs[:(L + 31) // 32] != 0).all()   # no word excluded entirely: the planes keep every word
    truth = staircase_truth(incs, L, q, s)
    assert (truth == 0).sum() >= 4 and truth.max() == inc
    pmask = staircase_pair_masks(incs, L, n, seed=200 + T)
    _sweep_data[T] = dict(L=L, n=n, seqs=seqs, incs=incs, inc=inc, truth=truth, pmask=pmask, ml=int(0.8 * L))
    return _sweep_data[T]


_sweep_ref = {}


def sweep_ref(T, pair, et, norm):
    """The expected (D, N) bytes: the closed form itself (non-pair, double, no norm), else the oracle's
    conversion of it (its double, un-normed matrix equals the closed form: asserted), or the oracle's
    fsacmpair on the per-taxon masks (pair)."""
    key = (T, pair, et, norm)
    if key in _sweep_ref:
        return _sweep_ref[key]
    from oracle import pyoracle
    d = sweep_data(T)
    if pair:
        D, N, _ = pyoracle.snp_ltd(d["seqs"], d["pmask"], d["n"], d["L"], pair=True, norm=norm, min_length=d["ml"],
                                   etype=et, byte_scale=BS, want_n=True)
        D8, _, _ = pyoracle.snp_ltd(d["seqs"], d["pmask"], d["n"], d["L"], pair=True, min_length=d["ml"])
        assert (D8 == -1).any() and (D8 == 0).any() and (D8 > 0).any()
    else:
        D0, _, inc = pyoracle.snp_ltd(d["seqs"], d["incs"], d["n"], d["L"])
        assert inc == d["inc"] and (D0 == d["truth"]).all()
        N = None
        if (et, norm) == (8, 0):
            D = d["truth"].astype(np.float64)
        else:
            D, _, _ = pyoracle.snp_ltd(d["seqs"], d["incs"], d["n"], d["L"], norm=norm, etype=et, byte_scale=BS)
    _sweep_ref[key] = (D, N)
    return D, N


def check_plan(plan, L, pair, mode, forced):
    """The plan read back is the one the case meant: the forced slice count, slices that cover the words
    with none to spare, whole chunks of this launcher, and the documented rule itself."""
    S, Wk = plan
    Wp = planes_words(L, pair)
    kc, kmax = kc_kmax(mode, pair)
    chunks = Wp // kc
    want = min(forced, chunks)
    # min(forced S, chunks) slices, except where equal slices of whole chunks cannot make that many: 4 chunks
    # in 3 slices are 2 + 2 (no multiple of kc lies in [4 kc / 3, 2 kc)), the only such case up to 12 chunks
    assert S == cdiv(chunks, cdiv(chunks, want)), (plan, Wp, kc, forced)
    assert S == want or (chunks, want) == (4, 3), (plan, Wp, kc, forced)
    assert S * Wk >= Wp > (S - 1) * Wk, (plan, Wp)
    assert Wk % kc == 0 and Wk >= kc, (plan, kc)
    assert plan == plan_rule(Wp, kc, forced, kmax), (plan, Wp, kc, forced)


@pytest.mark.parametrize("T,S,pair", SWEEP_CASES)
def test_dist_chunk_sweep(dev, monkeypatch, T, S, pair):
    """Every kernel choice at 1 to 12 chunks per tile cut into 1, 2 or 3 forced slices, full LT: D (and N in
    pair mode) byte for byte the closed form / the oracle, and the plan read back is the forced one."""
    d = sweep_data(T)
    et, norm = sweep_et_norm(T, S, pair)
    D, N = sweep_ref(T, pair, et, norm)
    n, L = d["n"], d["L"]
    msa = Msa(dev, d["seqs"], d["pmask"] if pair else d["incs"], n * (n - 1) // 2, et, pair)
    try:
        for mode in MODES:
            set_mode(monkeypatch, mode, S)
            msa.poison()
            inc = dev.snp_ltd_dev(msa.ps, msa.pi, n, L, msa.W, msa.pd, N_ptr=msa.pn, pair=pair, norm=norm,
                                  min_length=d["ml"] if pair else 1, etype=et, byte_scale=BS)
            plan = dev.last_dist_plan()
            assert same_bytes(msa.fetch(msa.pd), D), (mode, plan)
            if pair:
                assert same_bytes(msa.fetch(msa.pn), N), (mode, plan)
            else:
                assert inc == d["inc"]
            check_plan(plan, L, pair, mode, S)
    finally:
        msa.free()


def test_dist_chunk_sweep_covers_every_regime():
    """The (chunks of a full slice, chunks of the last slice) k_snp_mfma3 gets over SWEEP_CASES, from the
    documented rule (each case asserts that the plan it ran is that rule's): 1, 2 and 3 chunks (its prologue
    alone), 4 (no steady loop), 5 and >= 6 (steady loop), and a last slice shorter than the others."""
    seen = set()
    for T, S, pair in SWEEP_CASES:
        if pair:
            continue   # pair mode runs k_snp_mfma2_pair
        Wp = planes_words(sweep_L(T), False)
        Sp, Wk = plan_rule(Wp, 8, S, KMAX)
        seen.add((Wk // 8, (Wp - (Sp - 1) * Wk) // 8))
    counts = {c for pair_ in seen for c in pair_}
    assert {1, 2, 3, 4, 5} <= counts and any(c >= 6 for c in counts), sorted(seen)
    assert any(last < full for full, last in seen), sorted(seen)
    # the pair kernel and the 128 x 128 launchers likewise see a short last slice and one-chunk slices
    for mode, pair in (("2", True), ("1", False), ("0", True)):
        kc, kmax = kc_kmax(mode, pair)
        got = set()
        for T, S, p in SWEEP_CASES:
            if p == pair:
                Wp = planes_words(sweep_L(T), pair)
                Sp, Wk = plan_rule(Wp, kc, S, kmax)
                got.add((Wk // kc, (Wp - (Sp - 1) * Wk) // kc))
        assert any(full == 1 for full, _ in got) and any(last < full for full, last in got), (mode, pair, sorted(got))


@pytest.mark.parametrize("T,S,pair,world", BAND_CASES)
def test_dist_chunk_sweep_band(dev, monkeypatch, T, S, pair, world):
    """The same through ccg_snp_ltd_shard_dev (the BAND forms): each rank's rows at shard_row_offset equal
    the band extract of the same truth, as test_gpu_shard.py::test_dist_shard_layout compares them."""
    from ccphylo_amd import native as nt
    d = sweep_data(T)
    et, norm = sweep_et_norm(T, S, pair)
    D, _ = sweep_ref(T, pair, et, norm)
    n, L = d["n"], d["L"]
    elems = [nt.shard_elems(n, rank, world) for rank in range(world)]
    msa = Msa(dev, d["seqs"], d["pmask"] if pair else d["incs"], max(elems), et, False)
    try:
        for mode in MODES:
            set_mode(monkeypatch, mode, S)
            for rank in range(world):
                msa.poison()
                inc = dev.snp_ltd_shard_dev(msa.ps, msa.pi, n, L, msa.W, msa.pd, rank, world, norm=norm, etype=et,
                                            byte_scale=BS, pair=pair, min_length=d["ml"] if pair else 1)
                plan = dev.last_dist_plan()
                assert same_bytes(msa.fetch(msa.pd, elems[rank]), nt.shard_extract(D, n, rank, world)), (mode, rank)
                assert pair or inc == d["inc"]
                check_plan(plan, L, pair, mode, S)
    finally:
        msa.free()


# ---------------------------------------------------------------- C4: the f32-exact limit
LIMIT_N = 48            # one tile at either tile size
L_FULL = 5_592_320      # 174,760 words = 8 * 21,845: the longest slice of the 256 x 256 kernels, 3 * 32 * Wk = 16,776,960
L_OVER = 5_760_000      # 180,000 words: past MFMA_KMAX, the clamp cuts every MFMA form's tile in two
L_NONSPLIT = 5_592_064  # 174,752 words = 16 * 10,922: the longest row the non-pair planes hold without a split

# The plans the kernels must report at CCG_DIST_SLICES=1, (S, Wk) by (L, pair, mode).  At L_FULL the pair
# planes hold 174,760 words and the 256 x 256 pair kernel takes them in one slice (its non-SPLIT form).  The
# non-pair planes are padded to 16 words, 174,768 > MFMA_KMAX, so k_snp_mfma2 / k_snp_mfma3 cut them into the
# 174,760-word slice and an 8-word one (SPLIT): the identical pairs still accumulate 16,776,960 in slice 0,
# and L_NONSPLIT puts the non-SPLIT forms of those two kernels at the longest row they can get, 16,776,192.
LIMIT_PLANS = {
    (L_FULL, True, "2"): (1, 174760), (L_FULL, True, "3"): (1, 174760),
    (L_FULL, True, "1"): (1, 174760), (L_FULL, True, "0"): (1, 174760),
    (L_FULL, False, "2"): (2, 174760), (L_FULL, False, "3"): (2, 174760),
    (L_FULL, False, "1"): (2, 174752), (L_FULL, False, "0"): (1, 174768),
    (L_OVER, False, "2"): (2, 174760), (L_OVER, False, "3"): (2, 174760),
    (L_OVER, True, "2"): (2, 174760), (L_OVER, True, "3"): (2, 174760),
    (L_OVER, False, "1"): (2, 174752), (L_OVER, False, "0"): (1, 180000),
    (L_OVER, True, "1"): (1, 180000),   # k_snp_mfma_pair gives way to the VALU pair tiles
    (L_OVER, True, "0"): (1, 180000),
    (L_NONSPLIT, False, "2"): (1, 174752), (L_NONSPLIT, False, "3"): (1, 174752),
}
LIMIT_CASES = [(L, pair, et, norm) for L in (L_FULL, L_OVER) for pair in (False, True)
               for et, norm in ((8, 0), (4, 1000))]

_limit_data = {}


def limit_data(L):
    """48 staircase taxa of length L (69 MB; the latest length only is kept) and the references made from them."""
    if L in _limit_data:
        return _limit_data[L]
    _limit_data.clear()
    n = LIMIT_N
    rng = np.random.default_rng(L)
    q, s = [L, L, L, 0, 0], [1, 2, 1, 1, 3]   # (0, 1) differ everywhere; (0, 2) and (3, 4) are identical pairs
    for k, Wk in enumerate((174760, 174752)):
        for dlt in (-1, 0, 1):
            if 32 * Wk + dlt <= L:
                q.append(32 * Wk + dlt)
                s.append(1 + (k + dlt) % 3)
    q += list(rng.integers(0, L + 1, n - len(q)))
    s += list(rng.integers(1, 4, n - len(s)))
    q, s = np.array(q), np.array(s)
    seqs, incs, inc = staircase_packed(L, q, s, seed=L % 1000, holes=0.02)
    assert (incs[:(L + 31) // 32] != 0).all()
    truth = staircase_truth(incs, L, q, s)
    assert truth[1 * 0 // 2 + 0] == inc and truth[2 * 1 // 2 + 0] == 0 and truth[4 * 3 // 2 + 3] == 0
    # pair mode: taxa 0 and 2 (identical) include every position, so their dot product is 3 * 32 * Wk there too
    pmask = staircase_pair_masks(incs, L, n, seed=L % 997, empty=n // 2)
    full = np.full(L // 32 + 1, 0xFFFFFFFF, dtype=np.uint32)
    full[(L + 31) // 32:] = 0
    if L % 32:
        full[(L + 31) // 32 - 1] = (0xFFFFFFFF << (32 - L % 32)) & 0xFFFFFFFF
    pmask[0] = pmask[2] = full
    _limit_data[L] = dict(L=L, n=n, seqs=seqs, incs=incs, inc=inc, truth=truth, pmask=pmask, ml=int(0.8 * L), ref={})
    return _limit_data[L]


def limit_ref(d, pair, et, norm):
    key = (pair, et, norm)
    if key not in d["ref"]:
        from oracle import pyoracle
        if pair:
            D, N, _ = pyoracle.snp_ltd(d["seqs"], d["pmask"], d["n"], d["L"], pair=True, norm=norm,
                                       min_length=d["ml"], etype=et, byte_scale=BS, want_n=True, threads=8)
            assert N[2 * 1 // 2 + 0] == d["L"] and D[2 * 1 // 2 + 0] == 0 and (D == -1).any()
        elif (et, norm) == (8, 0):
            D, N = d["truth"].astype(np.float64), None
        else:
            D, N, _ = pyoracle.snp_ltd(d["seqs"], d["incs"], d["n"], d["L"], norm=norm, etype=et, byte_scale=BS,
                                       threads=8)
        d["ref"][key] = (D, N)
    return d["ref"][key]


def run_limit(dev, monkeypatch, L, pair, et, norm, modes):
    d = limit_data(L)
    D, N = limit_ref(d, pair, et, norm)
    n = d["n"]
    msa = Msa(dev, d["seqs"], d["pmask"] if pair else d["incs"], n * (n - 1) // 2, et, pair)
    try:
        for mode in modes:
            set_mode(monkeypatch, mode, 1)
            msa.poison()
            inc = dev.snp_ltd_dev(msa.ps, msa.pi, n, L, msa.W, msa.pd, N_ptr=msa.pn, pair=pair, norm=norm,
                                  min_length=d["ml"] if pair else 1, etype=et, byte_scale=BS)
            plan = dev.last_dist_plan()
            print(f"L={L} pair={pair} mode={mode} plan={plan} ms={dev.last_dist_ms():.1f}")
            assert same_bytes(msa.fetch(msa.pd), D), (mode, plan)
            if pair:
                assert same_bytes(msa.fetch(msa.pn), N), (mode, plan)
            else:
                assert inc == d["inc"]
            kc, kmax = kc_kmax(mode, pair)
            assert plan == LIMIT_PLANS[(L, pair, mode)] == plan_rule(planes_words(L, pair), kc, 1, kmax), (mode, plan)
    finally:
        msa.free()


@pytest.mark.parametrize("L,pair,et,norm", LIMIT_CASES)
def test_dist_f32_exact_limit(dev, monkeypatch, L, pair, et, norm):
    """One tile, one forced slice, rows at and past the f32-exact slice: identical pairs (dot = +3 * 32 * Wk,
    16,776,960 at Wk = 174,760, the largest value an accumulator may hold), a pair that differs everywhere,
    steps at 32 Wk and 32 Wk +- 1 for the two clamped slice lengths; every cell (and N) against the truth,
    and the plans of LIMIT_PLANS: at 180,000 words the MFMA forms split at the clamp, the VALU tiles do not,
    and the 128 x 128 pair form gives way to the VALU pair tiles.

    At L = 5,592,320 the 256 x 256 kernels report S = 1, Wk = 174,760 in pair mode only.  The non-pair planes
    are 174,768 words (rounded up to 16), so k_snp_mfma2 / k_snp_mfma3 report S = 2, Wk = 174,760: slice 0
    holds the 16,776,960, an 8-word slice follows (test_dist_f32_exact_limit_nonsplit has their non-SPLIT
    forms at the longest row those can get)."""
    run_limit(dev, monkeypatch, L, pair, et, norm, MODES)


@pytest.mark.parametrize("et,norm", [(8, 0), (4, 1000)])
def test_dist_f32_exact_limit_nonsplit(dev, monkeypatch, et, norm):
    """k_snp_mfma2 / k_snp_mfma3 without SPLIT at the longest non-pair row that needs no split: 174,752
    words, identical pairs accumulate 16,776,192."""
    run_limit(dev, monkeypatch, L_NONSPLIT, False, et, norm, ("2", "3"))
