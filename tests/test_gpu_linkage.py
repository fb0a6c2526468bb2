"""GPU parity of the tree methods upgma, cf, ff and mn (CCG_TREE_UPGMA / CF / FF /
MN): the gfx950 engine through the C-ABI and the `ccphylo` CLI against the
reference binary's golden vectors (tests/golden/golden_linkage.json) and,
join record by join record (i, j, Li, Lj bit for bit, final_n, final_d),
against the serial restatement tests/linkage_oracle.c, which
tests/test_linkage_oracle.py pins to the binary."""
import os
import subprocess

import numpy as np
import pytest

import linkage_oracle as lo
from conftest import GOLDEN
from linkage_oracle import golden_out, linkage_cases
from test_gpu import _clade_ltd, _euclid, _missing_ltd, _snp

pytestmark = pytest.mark.gpu

ALL = (lo.UPGMA, lo.CF, lo.FF, lo.MN)
MISSING_OK = (lo.UPGMA, lo.FF, lo.MN)
NAMES = {v: k for k, v in lo.METHODS.items()}


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def same_tree(dev, D, n, method, etype=8, bs=1.0, flags=0, **kw):
    """Engine joins == restatement joins as whole records; returns the engine's stats."""
    got, fn, fd, st = dev.tree(D, n, etype=etype, byte_scale=bs, method=method, flags=flags, exact=True, **kw)
    ref, rfn, rfd = lo.tree(D, n, etype=etype, byte_scale=bs, method=method, flags=flags)
    assert (fn, fd) == (rfn, rfd)
    assert len(got) == len(ref)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, (NAMES[method], n, int(bad[0]), got[bad[0]], ref[bad[0]])
    return st


def test_method_ids():
    import ccphylo_amd as cg
    assert (cg.CCG_TREE_UPGMA, cg.CCG_TREE_CF, cg.CCG_TREE_FF, cg.CCG_TREE_MN) == ALL


@pytest.mark.parametrize("case", linkage_cases(), ids=lambda c: c["name"])
def test_golden_engine(dev, case):
    import ccphylo_amd as cg
    path, method, et, bs, flags, prec = lo.parse_tree_args(case["args"])

    def run(D, n):
        joins, fn, fd, _ = dev.tree(D, n, etype=et, byte_scale=bs, method=method, flags=flags, exact=True)
        return joins, fn, fd
    trees = cg.newick_from_phylip(path, run, etype=et, byte_scale=bs, flags=flags, precision=prec)
    assert ("\n".join(trees) + "\n").encode() == golden_out(case)


@pytest.mark.parametrize("case", linkage_cases(("cf", "ff", "mn")), ids=lambda c: c["name"])
def test_golden_cli(case):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH] + list(case["args"]), cwd=GOLDEN, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout == golden_out(case)


@pytest.mark.parametrize("method", ALL, ids=lambda m: NAMES[m])
@pytest.mark.parametrize("n", [3, 4, 5, 17, 65, 257])
def test_small_n_vs_restatement(dev, method, n):
    for seed in (1, 2, 3):
        same_tree(dev, _euclid(n, 100 * n + seed), n, method)


_DATA = {}


def data(kind, n):
    """One matrix per (kind, n), shared by the methods (left unchanged)."""
    if (kind, n) not in _DATA:
        D = {"euc": _euclid, "snp": _snp, "clade": _clade_ltd, "miss": _missing_ltd}[kind](n, n)
        D.setflags(write=False)
        _DATA[(kind, n)] = D
    return _DATA[(kind, n)]


@pytest.mark.parametrize("method", ALL, ids=lambda m: NAMES[m])
@pytest.mark.parametrize("kind,n", [("euc", 600), ("euc", 1500), ("snp", 1500), ("clade", 1500)])
def test_vs_restatement(dev, method, kind, n):
    st = same_tree(dev, data(kind, n), n, method)
    if kind == "clade" and method in (lo.UPGMA, lo.FF):
        # UPGMApair's bounded rows were really rescanned (dnj.c:246): the path is not vacuous
        ref = lo.tree(data(kind, n), n, method=method, stats=True)[3]
        assert st[0] > 0 and st[1] > 0
        assert (st[0], st[1]) == (ref[0], ref[1])


@pytest.mark.parametrize("method", MISSING_OK, ids=lambda m: NAMES[m])
@pytest.mark.parametrize("n", [400, 1100])
def test_missing_vs_restatement(dev, method, n):
    same_tree(dev, data("miss", n), n, method)


@pytest.mark.parametrize("method", ALL, ids=lambda m: NAMES[m])
@pytest.mark.parametrize("et", [4, 2, 1])
def test_types_vs_restatement(dev, method, et):
    n = 700
    D = data("snp", n)
    bs = {4: 1.0, 2: 4.0, 1: 1.0}[et]
    if et == 4:
        Dt = D.astype(np.float32)
    else:
        Dt = np.clip(D * bs + 0.5, 0, 255 if et == 1 else 65535).astype(np.uint8 if et == 1 else np.uint16)
    same_tree(dev, Dt, n, method, etype=et, bs=bs)


@pytest.mark.parametrize("method", ALL, ids=lambda m: NAMES[m])
@pytest.mark.parametrize("n", [70, 300])
@pytest.mark.parametrize("et", [8, 1])
def test_all_equal_matrix(dev, method, n, et):
    """One repeated value: every comparison is a tie."""
    D = np.full(n * (n - 1) // 2, 200, dtype=lo.ETYPES[et])
    same_tree(dev, D, n, method, etype=et, bs=1.0)


@pytest.mark.parametrize("method", (lo.UPGMA, lo.FF), ids=lambda m: NAMES[m])
@pytest.mark.parametrize("blocks", ["1", "3", "4096"])
def test_rescan_grid_shapes(dev, monkeypatch, method, blocks):
    """k_lk_rescan with one block (each wave walks many listed rows), a few, and
    more waves than rows (CCG_LK_RESCAN_BLOCKS); n > 512: the head's and the
    pick's walks take several passes."""
    monkeypatch.setenv("CCG_LK_RESCAN_BLOCKS", blocks)
    n = 1100
    st = same_tree(dev, data("clade", n), n, method)
    assert st[0] > 0


@pytest.mark.parametrize("method", ALL, ids=lambda m: NAMES[m])
def test_negative_limbs(dev, method):
    """-f 2 (limbLengthNeg, nj.c:81)."""
    n = 600
    same_tree(dev, data("euc", n), n, method, flags=2)


def test_max_joins_prefix(dev):
    n = 600
    D = data("euc", n)
    full = dev.tree(D, n, method=lo.UPGMA)[0]
    pre, fn, fd, _ = dev.tree(D, n, method=lo.UPGMA, max_joins=100)
    assert len(pre) == 100 and fn == n - 100 and (pre == full[:100]).all()


def test_exact_flag_ignored_by_linkage(dev):
    """exact = 0 runs the exact path for upgma / cf / ff (include/ccphylo_amd.h)."""
    n = 257
    D = data("euc", n)
    for m in (lo.UPGMA, lo.CF, lo.FF):
        a = dev.tree(D, n, method=m, exact=False)[0]
        b = dev.tree(D, n, method=m, exact=True)[0]
        assert (a == b).all()


def test_refusals(dev):
    import ccphylo_amd as cg
    n = 80
    D = _missing_ltd(n, 5)
    assert (D < 0).any()
    with pytest.raises(cg.CcgError, match="not supported"):   # CCG_EUNSUP
        dev.tree(D, n, method=lo.CF)
    E = _euclid(n, 5)
    for m in ALL:
        with pytest.raises(cg.CcgError, match="not supported"):
            dev.tree_shard(E, n, None, method=m)
    with pytest.raises(cg.CcgError, match="invalid argument"):   # CCG_EINVAL: no fall-through to NJ
        dev.tree(E, n, method=7)
    with pytest.raises(cg.CcgError, match="invalid argument"):
        dev.tree(E, n, method=-1)


def test_cli_refuses_gpus_with_new_method():
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH, "tree", "-i", "test.phy.gz", "--gpus", "2", "-m", "ff"], cwd=GOLDEN,
                       capture_output=True, timeout=60)
    assert p.returncode != 0 and p.stdout == b""
    assert b"--gpus" in p.stderr and b"not supported" in p.stderr


def test_cli_method_help_lists_new_methods():
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH, "tree", "-M"], capture_output=True, timeout=60)
    assert p.returncode == 0
    for line in (b"# cf      \tK-means Closest First", b"# ff      \tK-means Furthest First",
                 b"# mn      \tMinimum Neighbors"):
        assert line in p.stdout


@pytest.mark.parametrize("method", ["cf", "ff", "mn"])
def test_cli_dist_tree_fused(tmp_path, method):
    """`dist --tree --tree_method M`: the Newick of `dist | tree -m M`."""
    import ccphylo_amd as cg

    def cli(args):
        p = subprocess.run([cg.CLI_PATH] + args, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stdout
    src = os.path.join(GOLDEN, "msa64.fsa")
    phy = tmp_path / "d.phy"
    phy.write_bytes(cli(["dist", "-i", src]))
    two_step = cli(["tree", "-i", str(phy), "-m", method])
    out = tmp_path / "t.nwk"
    cli(["dist", "-i", src, "--tree", str(out), "--tree_method", method])
    assert two_step and out.read_bytes() == two_step


def test_cli_dist_tree_refuses_gpus_with_new_method(tmp_path):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH, "dist", "-i", os.path.join(GOLDEN, "msa64.fsa"), "--tree", str(tmp_path / "t.nwk"),
                        "--tree_method", "mn", "--gpus", "2"], capture_output=True, timeout=60)
    assert p.returncode != 0
    assert b"--gpus" in p.stderr and b"not supported" in p.stderr
