"""GPU parity of every tree engine on adversarial distance matrices
(tools/synth.py ADVERSARIAL; tests/test_adv_matrices.py pins what makes each
kind hard): contributions over many binades (additive), clamp-boundary
residues and zero limbs (line), dyadic half-ulp ties that defeat the row
sum's order-independence shortcut (dyadic), zero cells and identical rows
(dupes), few distinct values with tens of qualifying rows per join (grid).

Every comparison is on whole join records (i, j, Li, Lj by bits) plus
(final_n, final_d): the single engine in its default and forced DNJ forms,
the sharded kernels at worlds 1, 2 and 3, and the linkage methods, against
oracle.pyoracle.tree (nj, dnj, hnj) and tests/linkage_oracle.py (upgma, cf,
ff, mn).  No tolerance anywhere."""
import os
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

import linkage_oracle as lo
from conftest import ROOT
from test_gpu import _euclid, _snp
from test_gpu_linkage import same_tree
from tools.synth import ADVERSARIAL

pytestmark = pytest.mark.gpu

SEED = 7
KINDS = ("additive", "line", "dyadic", "dupes", "grid")
NJ, DNJ, HNJ = 0, 1, 2
MNAMES = {NJ: "nj", DNJ: "dnj", HNJ: "hnj"}
N_OF = {NJ: 600, DNJ: 1100, HNJ: 1100}   # the oracle's NJ is cubic: 0.13 s at 600


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


_DATA, _REF = {}, {}


def data(kind, n):
    """One matrix per (kind, n), shared by every test (left unchanged)."""
    if (kind, n) not in _DATA:
        D = ADVERSARIAL[kind](n, SEED)
        D.setflags(write=False)
        _DATA[(kind, n)] = D
    return _DATA[(kind, n)]


# byte_scale per (kind, etype): the largest cell stays under the type's
# maximum (grid: cells <= 1; dupes: points of [0, 1)^8, cells < sqrt(8))
SCALES = {("grid", 2): 100.0, ("grid", 1): 100.0, ("dupes", 2): 20000.0, ("dupes", 1): 80.0}


def typed(kind, n, et):
    """(matrix as element type et, byte_scale), cached like data()."""
    key = (kind, n, et)
    if key not in _DATA:
        D = data(kind, n)
        bs = 1.0
        if et == 4:
            D = D.astype(np.float32)
        elif et in (2, 1):
            bs = SCALES[(kind, et)]
            top = 255 if et == 1 else 65535
            stored = D * bs + 0.5   # dtouc(d, 0.5) (bytescale.c)
            assert stored.max() < top, (kind, et, stored.max())   # nothing clips, nothing reads as missing
            D = stored.astype(np.uint8 if et == 1 else np.uint16)
        D.setflags(write=False)
        _DATA[key] = (D, bs)
    return _DATA[key]


def oracle(key, D, n, et=8, bs=1.0, method=DNJ, flags=0):
    """pyoracle.tree(..., stats=True), computed once per key."""
    from oracle import pyoracle
    key = (key, n, et, method, flags)
    if key not in _REF:
        _REF[key] = pyoracle.tree(D, n, etype=et, byte_scale=bs, method=method, flags=flags, stats=True)
    return _REF[key]


def same(got, ref, what):
    """Whole join records and the final pair, bit for bit."""
    (gj, gfn, gfd), (rj, rfn, rfd) = got[:3], ref[:3]
    assert len(gj) == len(rj), what
    bad = np.nonzero(gj != rj)[0]
    assert bad.size == 0, (what, "first differing join", int(bad[0]), gj[bad[0]], rj[bad[0]])
    assert (gfn, gfd) == (rfn, rfd), what


def rule_counters(st):
    from ccphylo_amd import native
    K = native.NKSTAT
    return int(st[10 + 2 * K]), int(st[11 + 2 * K])


# ------------------------------------------------------------ (a) defaults
@pytest.mark.parametrize("method", [NJ, DNJ, HNJ], ids=MNAMES.get)
@pytest.mark.parametrize("kind", KINDS)
def test_default_forms(dev, kind, method):
    n = N_OF[method]
    D = data(kind, n)
    same(dev.tree(D, n, method=method, exact=True), oracle(kind, D, n, method=method), (kind, MNAMES[method]))


@pytest.mark.parametrize("method", [NJ, DNJ], ids=MNAMES.get)
@pytest.mark.parametrize("kind,et", [(k, 4) for k in KINDS] + [(k, et) for k in ("grid", "dupes") for et in (2, 1)])
def test_default_forms_types(dev, kind, et, method):
    n = N_OF[method]
    D, bs = typed(kind, n, et)
    same(dev.tree(D, n, etype=et, byte_scale=bs, method=method, exact=True),
         oracle(kind, D, n, et, bs, method), (kind, et, MNAMES[method]))


@pytest.mark.parametrize("method", [NJ, DNJ, HNJ], ids=MNAMES.get)
@pytest.mark.parametrize("kind", ["dyadic", "line"])
def test_negative_limbs(dev, kind, method):
    """flags = 2 (limbLengthNeg): the lengths the clamp would have hidden."""
    n = N_OF[method]
    D = data(kind, n)
    same(dev.tree(D, n, method=method, flags=2, exact=True), oracle(kind, D, n, method=method, flags=2),
         (kind, MNAMES[method]))


# ------------------------------------------------- (b) forced DNJ forms
SMALL_UNITS = {"CCG_PREFOLD_N": "0", "CCG_SEG_MUL": "1"}
PRUNE = dict(SMALL_UNITS, CCG_S_SPLIT_N="100", CCG_S_BANDS="64", CCG_PRUNE_CELLS="0")
BOUNDS = dict(SMALL_UNITS, CCG_S_SPLIT_N="100", CCG_PRUNE_CELLS="0", CCG_LB_MIN_N="100")
WAVE, GROUPS = ("9", "4"), ("20", "21")   # scan modes: one row per wave (et 8), row groups (et 4)


def _knob_sets():
    """(name, environment, scan modes it runs under; (None,): the default scan).
    The knob sets of test_gpu.py's test_dnj_scan_prune, test_dnj_block_bounds,
    test_dnj_scan_tail_fold, test_exact_walk_forms and test_dnj_band_mode_small_n."""
    sets = []
    for prune, vblk, fold in (("1", "1", "1"), ("1", "0", "1"), ("2", "1", "0"), ("2", "0", "0"), ("0", "0", "0")):
        sets.append((f"prune{prune}_vblk{vblk}", dict(PRUNE, CCG_SCAN_PRUNE=prune, CCG_SCAN_VBLK=vblk,
                                                     CCG_SCAN_FOLD=fold), WAVE + GROUPS))
    sets.append(("prune2_nocmp", dict(PRUNE, CCG_SCAN_PRUNE="2", CCG_SCAN_VBLK="1", CCG_SCAN_FOLD="0",
                                      CCG_SCAN_CMP="0"), WAVE + GROUPS))
    for prune in ("2", "0"):
        for lb in ("1", "0"):
            sets.append((f"bounds_prune{prune}_lb{lb}", dict(BOUNDS, CCG_SCAN_PRUNE=prune, CCG_SCAN_LB=lb,
                                                             CCG_LB_GROUPS="0"), WAVE + GROUPS))
    sets.append(("bounds_prune0_lb1_groups", dict(BOUNDS, CCG_SCAN_PRUNE="0", CCG_SCAN_LB="1", CCG_LB_GROUPS="1"),
                 GROUPS))
    for fold in ("1", "0"):
        sets.append((f"tail_fold{fold}", dict(SMALL_UNITS, CCG_SCAN_FOLD=fold), WAVE + GROUPS))
    for allpre in ("1", "0"):
        sets.append((f"walk_allpre{allpre}", {"CCG_XS_ALLPRE": allpre}, (None,)))
    for top, bands in ((16, 64), (8, 32)):
        sets.append((f"band_top{top}_bands{bands}", {"CCG_S_SPLIT_N": "100", "CCG_S_TOP": str(top),
                                                     "CCG_S_BANDS": str(bands)}, (None,)))
    return sets


KNOBS = {name: env for name, env, _ in _knob_sets()}
FORCED_KINDS = ("additive", "dyadic", "dupes", "grid")


@pytest.mark.parametrize("knobs,mode,kind", [(name, mode, kind) for name, _, modes in _knob_sets() for mode in modes
                                              for kind in FORCED_KINDS], ids=lambda v: str(v))
def test_forced_dnj_forms(dev, monkeypatch, knobs, mode, kind):
    """Every knob set under every scan mode it has, on every kind (a quarter
    of a second each): a case that fails beside a passing neighbour (bounds
    off, prune 0, the other fold) names the layer that is wrong."""
    n = 2500
    et = 4 if mode in GROUPS else 8
    for k, v in KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    if mode is not None:
        monkeypatch.setenv("CCG_SCAN_WAVE", mode)
    D, bs = typed(kind, n, et) if et != 8 else (data(kind, n), 1.0)
    ref = oracle(kind, D, n, et, bs, DNJ)
    got = dev.tree(D, n, etype=et, byte_scale=bs, method=DNJ, exact=True, profile=True)
    same(got, ref, (knobs, mode, kind))
    # the rows and cells the reference's minQpair rescans, from the engine's replay decisions
    assert rule_counters(got[3]) == (int(ref[3][0]), int(ref[3][1])), (knobs, mode, kind)


# --------------------------------------------- (c) exact-sum engagement
@pytest.mark.parametrize("kind", KINDS)
def test_exact_sum_engaged(dev, kind):
    """The row sums of these matrices are not provable in any order: at least
    half the joins take the serial-order sum (stats[6 + 2 NKSTAT]), so the
    parity above is parity of the binade-segmented code, not of the shortcut.
    The share the serial chain carried (stats[7 + 2 NKSTAT]) depends on the
    tie-list caps and is printed only."""
    from ccphylo_amd import native
    K = native.NKSTAT
    n = N_OF[DNJ]
    D = data(kind, n)
    got = dev.tree(D, n, method=DNJ, exact=True, profile=True)
    same(got, oracle(kind, D, n, method=DNJ), kind)
    serial, chain = int(got[3][6 + 2 * K]), int(got[3][7 + 2 * K])
    print(f"exact-sum engagement {kind}: joins {len(got[0])} serial-order {serial} chain {chain} "
          f"chain share {chain / max(serial, 1):.3f}")
    assert serial >= len(got[0]) / 2, (kind, serial, len(got[0]))


# --------------------------------------------- (d) power-of-two scales
BOUNDED = dict(BOUNDS, CCG_SCAN_WAVE="9", CCG_SCAN_PRUNE="2", CCG_SCAN_LB="1", CCG_LB_GROUPS="0")


@pytest.mark.parametrize("form", ["default", "bounds"])
@pytest.mark.parametrize("method", [NJ, DNJ], ids=MNAMES.get)
@pytest.mark.parametrize("k", [-1008, -200, 200, 900])
@pytest.mark.parametrize("base", ["snp", "euc"])
def test_power_of_two_scales(dev, monkeypatch, base, k, method, form):
    """The same matrix times 2^k.  k = -1008 puts integer data under the
    shortcut's exponent guard, so the exact sum runs at the lowest normal
    exponents; +-200 and +900 push the float-typed block bounds past float
    range on both sides, where they must degrade to 0 or FLT_MAX and stay
    sound.  The oracle on the scaled matrix is the truth."""
    n = 700
    if (base, n) not in _DATA:
        _DATA[(base, n)] = {"snp": _snp, "euc": _euclid}[base](n, n)
        _DATA[(base, n)].setflags(write=False)
    key = (base, n, "ldexp", k)
    if key not in _DATA:
        _DATA[key] = np.ldexp(_DATA[(base, n)], k)
        _DATA[key].setflags(write=False)
    D = _DATA[key]
    assert np.isfinite(D).all() and (D[D > 0] >= np.finfo(np.float64).tiny).all()
    if form == "bounds":
        for name, v in BOUNDED.items():
            monkeypatch.setenv(name, v)
    same(dev.tree(D, n, method=method, exact=True), oracle((base, k), D, n, method=method),
         (base, k, MNAMES[method], form))


# ------------------------------------------------- (e) sharded kernels
@pytest.mark.parametrize("method", [NJ, DNJ, HNJ], ids=MNAMES.get)
@pytest.mark.parametrize("kind", KINDS)
def test_shard_world1(dev, monkeypatch, kind, method):
    n = 600
    D = data(kind, n)
    ref = oracle(kind, D, n, method=method)
    single = dev.tree(D, n, method=method, exact=True)
    same(single, ref, (kind, MNAMES[method], "single"))
    monkeypatch.setenv("CCG_SHARD_FORCE", "1")   # the sharded kernels, not the world-1 single engine
    same(dev.tree_shard(D, n, None, method=method, exact=True), single, (kind, MNAMES[method], "shard"))


def _rank_main(rank, world, port, kind, n, methods, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import ccphylo_amd as cg
    from ccphylo_amd import native as nt
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["CCG_SHARD_FORCE"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    D = ADVERSARIAL[kind](n, SEED)   # every rank makes the matrix itself
    dev = cg.Device(0)
    coll = nt.HostColl(dist)
    for method in methods:
        joins, fn, fd, _ = dev.tree_shard(D, n, coll, method=method, exact=True)
        np.save(os.path.join(out_dir, f"j{method}_{rank}.npy"), joins)
        np.save(os.path.join(out_dir, f"f{method}_{rank}.npy"), np.array([fn, fd]))
    dev.close()
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world, args, limit=240.0):
    """`world` rank processes (at most 3), joined within `limit` seconds or killed."""
    from test_gpu_shard import _free_port
    assert world <= 3
    ctx = mp.start_processes(_rank_main, args=(world, _free_port()) + args, nprocs=world, join=False,
                             start_method="spawn")
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5.0):
            assert time.monotonic() < deadline, f"rank processes still running after {limit} s"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join()


@pytest.mark.parametrize("kind", ["dyadic", "dupes"])
@pytest.mark.parametrize("world", [2, 3])
def test_shard_multiprocess(dev, tmp_path, world, kind):
    """Worlds 2 and 3 as rank processes on the one GPU over the host-staged
    transport; each world runs NJ and DNJ in the same processes."""
    n = 700
    D = data(kind, n)
    _run_ranks(world, (kind, n, (NJ, DNJ), str(tmp_path)))
    for method in (NJ, DNJ):
        ref = oracle(kind, D, n, method=method)
        same(dev.tree(D, n, method=method, exact=True), ref, (kind, MNAMES[method], "single"))
        for r in range(world):
            fn, fd = np.load(tmp_path / f"f{method}_{r}.npy")
            same((np.load(tmp_path / f"j{method}_{r}.npy"), int(fn), float(fd)), ref,
                 (kind, MNAMES[method], world, r))


# --------------------------------------------------- (f) linkage methods
LK = {v: k for k, v in lo.METHODS.items()}


@pytest.mark.parametrize("method", (lo.UPGMA, lo.CF, lo.FF, lo.MN), ids=LK.get)
@pytest.mark.parametrize("kind", KINDS)
def test_linkage(dev, kind, method):
    n = 600
    D = data(kind, n)
    st = same_tree(dev, D, n, method)
    if kind in ("dupes", "grid") and method in (lo.UPGMA, lo.FF):
        # the rows and cells UPGMApair rescanned (dnj.c:246)
        ref = lo.tree(D, n, method=method, stats=True)[3]
        assert (st[0], st[1]) == (ref[0], ref[1])
