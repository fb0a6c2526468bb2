"""GPU: the host halves of the engine's entry points at the smallest shapes that
take each of their allocation branches.

Every host-pointer entry allocates device memory, uploads, runs its
device-pointer twin's code and downloads; the dist keeps its bit planes, the
included count and the compacted word list either in memory of its own or, in a
CCG_CTX_NOSYNC context, in a workspace slot of the context.  The cases here run
each entry through both doors and compare bytes: host entry == device entry ==
the oracle of the entry's own test file.  Nothing here provokes a HIP failure:
the error exits are checked by construction."""
import ctypes as C
import sys

import numpy as np
import pytest

import dbscan_oracle as dbo
import linkage_oracle as lo
import meth_oracle as mo
import tsv_oracle as tso
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)

ETS = (8, 4, 2, 1)
BS = 2.0


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ dist
def msa(n, L, seed=1):
    """Packed rows, a global mask whose middle word is all zero (so the planes
    are compacted through a word list) and per-taxon masks below it."""
    rng = np.random.default_rng(seed * 1000 + n * 10 + L)
    W, nw = L // 32 + 1, (L + 31) // 32
    seqs = rng.integers(0, 2 ** 63, size=(n, W), dtype=np.uint64)
    g = np.zeros(W, np.uint32)
    g[:nw] = 0xFFFFFFFF
    if L % 32:
        g[nw - 1] = (0xFFFFFFFF << (32 - L % 32)) & 0xFFFFFFFF
    g[nw // 2] = 0
    holes = rng.integers(0, 2 ** 32, size=(n, W), dtype=np.uint64).astype(np.uint32) | np.uint32(0x77777777)
    return seqs, g, holes & g


_dist_ref = {}


def dist_ref(n, L, pair, et):
    """(seqs, incs, D, N, inc) of the oracle, once per case and left unchanged."""
    key = (n, L, pair, et)
    if key not in _dist_ref:
        from oracle import pyoracle
        seqs, g, pm = msa(n, L)
        incs = pm if pair else g
        D, N, inc = None, None, None   # n = 1: no pair to compare (the caller counts the mask itself)
        if n > 1:
            D, N, inc = pyoracle.snp_ltd(seqs, incs, n, L, pair=pair, norm=1000, etype=et, byte_scale=BS, want_n=pair)
        for x in (seqs, incs, D, N):
            if x is not None:
                x.setflags(write=False)
        _dist_ref[key] = (seqs, incs, D, N, inc)
    return _dist_ref[key]


def dist_host(d, n, L, pair, et):
    seqs, incs, _, _, _ = dist_ref(n, L, pair, et)
    return d.snp_ltd(seqs, incs, n, L, pair=pair, norm=1000, etype=et, byte_scale=BS, want_n=pair)


def dist_dev(d, n, L, pair, et):
    """The device-pointer entry on device copies; outputs pre-filled with 0xA5."""
    import ccphylo_amd as cg
    seqs, incs, _, _, _ = dist_ref(n, L, pair, et)
    m = n * (n - 1) // 2
    ptrs = [d.malloc(seqs.nbytes), d.malloc(incs.nbytes), d.malloc(max(m, 1) * et), d.malloc(max(m, 1) * et)]
    try:
        d.h2d(ptrs[0], seqs)
        d.h2d(ptrs[1], incs)
        for p in ptrs[2:]:
            d.h2d(p, np.full(max(m, 1) * et, 0xA5, np.uint8))
        inc = d.snp_ltd_dev(ptrs[0], ptrs[1], n, L, seqs.shape[1], ptrs[2], N_ptr=ptrs[3] if pair else None, pair=pair,
                            norm=1000, etype=et, byte_scale=BS)
        D, N = np.empty(m, cg.ETYPES[et]), np.empty(m, cg.ETYPES[et])
        if m:
            d.d2h(D, ptrs[2])
            d.d2h(N, ptrs[3])
        return D, (N if pair else None), inc
    finally:
        for p in ptrs:
            d.free(p)


def check_dist(d, n, L, pair, et):
    """host entry == device entry == oracle; returns the host entry's (D, N, inc)."""
    _, _, D0, N0, inc0 = dist_ref(n, L, pair, et)
    Dh, Nh, inch = dist_host(d, n, L, pair, et)
    Dd, Nd, incd = dist_dev(d, n, L, pair, et)
    assert same_bytes(Dh, Dd) and same_bytes(Dh, D0), (n, L, pair, et)
    if pair:
        assert same_bytes(Nh, Nd) and same_bytes(Nh, N0), (n, L, pair, et)
    else:
        assert inch == incd == inc0, (n, L, pair, et)
    return Dh, Nh, inch


@pytest.mark.parametrize("pair", [False, True], ids=["global", "pair"])
@pytest.mark.parametrize("et", ETS)
def test_dist_both_entries(dev, et, pair):
    """n = 5, 70 positions (three mask words, the middle one empty)."""
    _, incs, D0, _, _ = dist_ref(5, 70, pair, et)
    assert incs[..., 1].max() == 0 and D0.any()
    check_dist(dev, 5, 70, pair, et)


def test_dist_small_n(dev):
    """n = 1: no matrix, the included count alone (the device entry's lone count
    buffer, the host entry's host popcount); n = 2: one cell."""
    seqs, g, _ = msa(1, 70)
    want = int(sum(bin(int(w)).count("1") for w in g))
    for et in ETS:
        _, _, inc = dist_host(dev, 1, 70, False, et)
        assert inc == want
        D, _, inc = dist_dev(dev, 1, 70, False, et)
        assert inc == want and D.size == 0
        for pair in (False, True):
            check_dist(dev, 2, 70, pair, et)


def test_dist_row_range(dev):
    """ccg_snp_ltd on rows [2, 4) of n = 5: the cells of rows 2 and 3 are the
    full run's, every other cell keeps the caller's bytes."""
    import ccphylo_amd as cg
    from ccphylo_amd.native import SnpArgs
    n, L = 5, 70
    for et in ETS:
        for pair in (False, True):
            seqs, incs, D0, N0, _ = dist_ref(n, L, pair, et)
            m = n * (n - 1) // 2
            D = np.frombuffer(bytes([0xA5]) * (m * et), dtype=cg.ETYPES[et]).copy()
            N = D.copy()
            a = SnpArgs(n, L, seqs.shape[1], seqs.ctypes.data, incs.ctypes.data, int(pair), 1000, 1, 0, et, BS, 2, 4)
            inc = C.c_int(0)
            rc = dev.lib.ccg_snp_ltd(dev.h, C.byref(a), D.ctypes.data, N.ctypes.data if pair else None, C.byref(inc))
            assert rc == 0
            lo_, hi = 2 * 1 // 2, 4 * 3 // 2
            want = np.frombuffer(bytes([0xA5]) * (m * et), dtype=cg.ETYPES[et]).copy()
            want[lo_:hi] = D0[lo_:hi]
            assert same_bytes(D, want), (et, pair)
            if pair:
                want[lo_:hi] = N0[lo_:hi]
                assert same_bytes(N, want), (et, pair)


def test_dist_nosync_context(dev):
    """A CCG_CTX_NOSYNC context keeps the planes, the count and the word list
    in its workspace slot: the same bytes as the owned buffers give, then a
    matrix of two 256-row panels that grows the slot, then the small one again."""
    import ccphylo_amd as cg
    with cg.Device(0) as ns:
        ns.configure(nosync=True)
        for rnd in range(2):
            for et in ETS:
                for pair in (False, True):
                    for n in (5, 2):
                        Do, No, inco = dist_host(dev, n, 70, pair, et)
                        Dn, Nn, incn = check_dist(ns, n, 70, pair, et)
                        assert same_bytes(Do, Dn) and inco == incn
                        if pair:
                            assert same_bytes(No, Nn)
                _, _, inc = dist_dev(ns, 1, 70, False, et)
                assert inc == dist_host(dev, 1, 70, False, et)[2]
            if rnd == 0:
                for pair in (False, True):
                    check_dist(ns, 260, 70, pair, 8)


@pytest.mark.parametrize("pair", [False, True], ids=["global", "pair"])
def test_dist_forced_slices(dev, monkeypatch, pair):
    """CCG_DIST_SLICES=2 at 507 positions (16 words, test_gpu_dist_slices.py's
    T = 2): the split-K counts and the finish kernel, through both entries."""
    monkeypatch.setenv("CCG_DIST_SLICES", "2")
    for k in ("CCG_DIST_MFMA", "CCG_DIST_GLDS", "CCG_DIST_KC", "CCG_DIST_ORDER", "CCG_DIST_NOCOMPACT"):
        monkeypatch.delenv(k, raising=False)
    for et in ETS:
        check_dist(dev, 5, 507, pair, et)
        assert dev.last_dist_plan()[0] == 2


# ------------------------------------------------------------------ the other engines
def thrice(run):
    """run(device) twice on one fresh Device and once on another: three equal results; returns the first."""
    import ccphylo_amd as cg
    with cg.Device(0) as d:
        a, b = run(d), run(d)
    with cg.Device(0) as d:
        c = run(d)
    for x, y, z in zip(a, b, c):
        assert same_bytes(x, y) and same_bytes(x, z)
    return a


@pytest.fixture(scope="module")
def kma_files(tmp_path_factory):
    from gen_golden import kma_adversarial
    root = tmp_path_factory.mktemp("kma_host_paths")
    files = []
    for k in range(5):
        f = str(root / f"h{k}.mat")
        kma_adversarial(f, 100, seed=31, profile="wrap", k=k, gz=False)
        files.append(f)
    return files


@pytest.mark.parametrize("metric", ["cos", "nchi2"])   # cos alone allocates the row norms
@pytest.mark.parametrize("n", [1, 2, 5])
def test_kma_host_entry(dev, kma_files, n, metric):
    import torch
    import ccphylo_amd as cg
    from oracle import pyoracle
    K = cg.native.load_kma(kma_files[:n], "x")
    assert K["n"] == n
    m = n * (n - 1) // 2

    def run(d):
        D, N, fatal = d.kma_ltd(K, metric=metric, want_n=True)
        return D, N, np.int64(fatal)
    D, N, fatal = thrice(run)
    assert fatal == -1 and D.size == m and N.size == m
    if n == 1:
        return
    D0, N0, _, n0 = pyoracle.kma_dist(kma_files[:n], "x", metric=metric, want_n=True)
    assert n0 == n and same_bytes(D, D0) and same_bytes(N, N0)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    rec1, rec2, len1, len2 = up(K["rec1"]), up(K["rec2"]), up(K["len1"]), up(K["len2"])
    Dd = torch.zeros(m * 8, dtype=torch.uint8, device="cuda:0")
    Nd = torch.zeros(m * 8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert dev.kma_ltd_dev(n, rec1.data_ptr(), len1.data_ptr(), K["stride1"], rec2.data_ptr(), len2.data_ptr(),
                           K["stride2"], Dd.data_ptr(), Nd.data_ptr(), metric=metric) == -1
    assert Dd.cpu().numpy().tobytes() == D.tobytes() and Nd.cpu().numpy().tobytes() == N.tobytes()


@pytest.mark.parametrize("vtype", [8, 4])
@pytest.mark.parametrize("m", [1, 2, 5])
def test_vec_host_entry(dev, m, vtype):
    rng = np.random.default_rng(m)
    X = np.round(rng.uniform(-5, 5, (m, 3)), 3).astype(np.float32 if vtype == 4 else np.float64)
    D, = thrice(lambda d: (d.vec_ltd(X, "cos"),))
    assert D.size == m * (m - 1) // 2
    if m == 1:
        return
    assert same_bytes(D, tso.vec_ltd(X, "cos", 0.0))
    dX, dD = dev.malloc(X.nbytes), dev.malloc(D.nbytes)
    try:
        dev.h2d(dX, X)
        dev.vec_ltd_dev(dX, m, 3, dD, vtype=vtype, metric="cos")
        got = np.zeros_like(D)
        dev.d2h(got, dD)
    finally:
        dev.free(dX)
        dev.free(dD)
    assert same_bytes(got, D)


@pytest.mark.parametrize("et", ETS)
@pytest.mark.parametrize("n", [1, 2, 5])
def test_dbscan_host_entry(dev, n, et):
    rng = np.random.default_rng(10 * n + et)
    D = rng.integers(0, 6, n * (n - 1) // 2).astype(dbo.ETYPES[et])
    for minn in (1, 2):   # 2: border rows, the second pass over their cells
        N, Cl = thrice(lambda d: d.dbscan(D, n, 2.0, minn, et, 1.0)[:2])
        rN, rC, rk = dbo.dbscan(D, n, 2.0, minn, et, 1.0)
        assert (N == rN).all() and (Cl == rC).all()
        if n == 1:
            continue
        p = dev.malloc(D.nbytes)
        try:
            dev.h2d(p, D)
            N2, C2, k2, _ = dev.dbscan_dev(p, n, 2.0, minn, et, 1.0)
        finally:
            dev.free(p)
        assert same_bytes(N2, N) and same_bytes(C2, Cl) and k2 == rk


@pytest.mark.parametrize("pair", [False, True], ids=["global", "pair"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_meth_host_entry(dev, n, pair):
    L = 70
    tab = mo.strands_of("gAtc", "aA")
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, (n, L)).astype(np.uint8)
    codes[:, 30:34] = [2, 0, 3, 1]   # GATC across the word boundary
    W = L // 32 + 1
    seqs = np.array([mo.pack(c, W) for c in codes], dtype=np.uint64)
    _, g, pm = msa(n, L)
    incs = pm if pair else g
    want, wcnt, wfound = mo.mask_rows(seqs, incs, n, L, tab, pair)
    assert wfound > 0 and (want != incs).any()

    def run(d):
        out, cnt, found = d.meth_mask(seqs, incs, n, L, tab, pair=pair)
        return out, cnt, np.int64(found)
    out, cnt, found = thrice(run)
    assert found == wfound and same_bytes(out, want) and (cnt == wcnt).all()
    ds, di = dev.malloc(seqs.nbytes), dev.malloc(incs.nbytes)
    try:
        dev.h2d(ds, seqs)
        dev.h2d(di, incs)
        cnt2, found2 = dev.meth_mask_dev(ds, di, n, L, W, tab, pair=pair)
        back = np.zeros_like(incs)
        dev.d2h(back, di)
    finally:
        dev.free(ds)
        dev.free(di)
    assert found2 == wfound and same_bytes(back, out) and same_bytes(cnt2, cnt)


def _euclid(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 8))
    i, j = np.tril_indices(n, -1)
    return np.sqrt(((pts[i] - pts[j]) ** 2).sum(1))


@pytest.mark.parametrize("method", [0, 1, 2, lo.UPGMA, lo.CF, lo.FF, lo.MN],
                         ids=["nj", "dnj", "hnj", "upgma", "cf", "ff", "mn"])
@pytest.mark.parametrize("n", [3, 5])
def test_tree_host_entry(dev, n, method):
    """ccg_tree (and, for nj / dnj, ccg_tree_shard at world 1) == ccg_tree_dev == the oracle."""
    from oracle import pyoracle
    D = _euclid(n, 7 * n)

    def run(d):
        joins, fn, fd, _ = d.tree(D, n, method=method, exact=True)
        return joins, np.int64(fn), np.float64(fd)
    joins, fn, fd = thrice(run)
    rj, rfn, rfd = (pyoracle.tree if method <= 2 else lo.tree)(D, n, method=method)
    assert (fn, fd) == (rfn, rfd) and len(joins) == len(rj) and (joins == rj).all()
    p = dev.malloc(D.nbytes)
    try:
        dev.h2d(p, D)
        j2, fn2, fd2, _ = dev.tree_dev(p, n, method=method, exact=True)
    finally:
        dev.free(p)
    assert same_bytes(j2, joins) and (fn2, fd2) == (fn, fd)
    if method <= 1:
        j3, fn3, fd3, _ = dev.tree_shard(D, n, method=method, exact=True)
        assert same_bytes(j3, joins) and (fn3, fd3) == (fn, fd)
