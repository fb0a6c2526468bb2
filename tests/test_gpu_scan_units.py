"""The bounded rescan's unit length and grid: exact DNJ trees against the serial
oracle (joins, final pair, the reference-rule counters) however the rows are
cut into units and however many blocks walk them.

A run that keeps the block lower bounds (TreeBufs::lbm) cuts its rows into
units of DnjGrid::seg_lb cells (CCG_SEG_LB: a multiple of 64) and sizes the
compacted scan's grid to the blocks its context holds at once (CCG_SCAN_CMPB
overrides).  test_dnj_block_bounds' small-n setting, without CCG_SEG_MUL:

    CCG_SEG_LB 1024, 192   several units per row; at 192 a last unit shorter
                           than a 64-column block row, and bound loads that
                           start anywhere in a row's bound line
    CCG_SEG_LB unset       one unit per row at these n
    CCG_SCAN_CMPB 4        16 waves: every wave walks many units
    CCG_SCAN_CMPB unset    the occupancy-sized grid
    a 64-CU context        the grid sized to the mask's share

The cells a run loads (stats[1]) do not depend on the cut: a row needs the
same 64-column blocks whichever unit tests them, as long as the units begin at
multiples of 64.
"""
import numpy as np
import pytest

from test_gpu import _clade_ltd, _euclid

pytestmark = pytest.mark.gpu

SETTING = (("CCG_SCAN_WAVE", "9"), ("CCG_PREFOLD_N", "0"), ("CCG_S_SPLIT_N", "100"), ("CCG_PRUNE_CELLS", "0"),
           ("CCG_LB_MIN_N", "100"))
INPUTS = {"clade": (3000, 8), "euc": (2500, 8), "euc32": (2600, 4)}
# (CCG_SEG_LB, CCG_SCAN_CMPB); None: unset
CUTS = [("1024", None), ("192", None), (None, None), (None, "4"), ("192", "4")]

_cache = {}


def _input(kind):
    """The matrix and the oracle's tree of it (made once per module)."""
    if kind not in _cache:
        from oracle import pyoracle
        n, et = INPUTS[kind]
        D = _clade_ltd(n, n + 6) if kind == "clade" else _euclid(n, n + 7)
        if et == 4:
            D = D.astype(np.float32)
        _cache[kind] = (D, n, et, pyoracle.tree(D, n, etype=et, method=1, stats=True))
    return _cache[kind]


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()
    _cache.clear()


def _check(dev, kind, what):
    from ccphylo_amd import native
    K = native.NKSTAT
    D, n, et, (ref, rfn, rfd, rst) = _input(kind)
    got, fn, fd, st = dev.tree(D, n, etype=et, method=1, exact=True, profile=True)
    assert (fn, fd) == (rfn, rfd), what
    assert len(got) == len(ref) and (got == ref).all(), what
    assert (st[10 + 2 * K], st[11 + 2 * K]) == (int(rst[0]), int(rst[1])), what
    return st[1]


def _set(monkeypatch, seg, cmpb):
    for k, v in SETTING:
        monkeypatch.setenv(k, v)
    for k, v in (("CCG_SEG_LB", seg), ("CCG_SCAN_CMPB", cmpb)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    for k in ("CCG_SEG_MUL", "CCG_SCAN_LB", "CCG_SCAN_PRUNE", "CCG_LB_GROUPS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("kind", sorted(INPUTS))
def test_scan_unit_lengths(dev, monkeypatch, kind):
    """Every cut of CUTS builds the oracle's tree and loads the same cells."""
    cells = {}
    for seg, cmpb in CUTS:
        _set(monkeypatch, seg, cmpb)
        cells[(seg, cmpb)] = _check(dev, kind, (seg, cmpb))
    assert len(set(cells.values())) == 1, cells


def test_scan_units_masked_context(monkeypatch):
    """A context on 64 CUs (8 per XCD): the grid is the mask's share; the same tree."""
    import ccphylo_amd as cg
    _set(monkeypatch, None, None)
    with cg.Device(0) as d:
        d.configure(cu_mask=list(range(64)))
        _check(d, "clade", "64 CUs")
