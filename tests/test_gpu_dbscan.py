"""GPU: `ccphylo dbscan` on the gfx950 engine (ccg_dbscan / ccg_dbscan_dev, the
CLI subcommand and the fused `dist --dbscan`).  Neighbour counts, cluster ids
and the cluster count are integers: every comparison is exact, against the
reference's bytes (tests/golden/dbscan) or the serial restatement
(tests/dbscan_oracle.py).

The count kernel tiles the LT in blocks of TILE_ROWS x TILE_COLS cells
(DB_TR / DB_TC in ccphylo_amd/csrc/dbscan.hip); N_TILES lies past twice either."""
import os
import subprocess

import numpy as np
import pytest

import dbscan_oracle as dbo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TILE_ROWS, TILE_COLS = 128, 1024
N_TILES = 2 * TILE_COLS + TILE_ROWS + 1 + 20   # 2197: three column tiles, the last row tile partial
CASES = dbo.golden_cases()


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def cli(args, cwd=GOLDEN):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH] + args, cwd=cwd, capture_output=True, timeout=300)
    assert p.returncode == 0, (args, p.stderr.decode()[-2000:])
    return p.stdout


def check(dev, D, n, e, minn, etype=8, bs=1.0):
    """Engine == restatement, exactly; returns the engine's (N, C, nclust, stats) and the border-row count."""
    N, C, k, st = dev.dbscan(D, n, e, minn, etype, bs)
    rN, rC, rk, border = dbo.dbscan(D, n, e, minn, etype, bs, want_border=True)
    assert (N == rN).all(), (n, e, minn, etype)
    assert (C == rC).all(), (n, e, minn, etype)
    assert k == rk
    m = n * (n - 1) // 2
    assert st[0] == border
    if border == 0:
        assert st[1] == m      # the LT is read exactly once
    else:
        assert m <= st[1] <= m + border * (n - 1)   # a border row's scan stays in its row part
    return N, C, k, st, border


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_golden(case):
    assert cli(list(case["args"])) == case["bytes"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_engine_golden(dev, case):
    from ccphylo_amd import native
    e, minn, et, bs = dbo.case_options(case["args"])
    mats = native.load_phylip(os.path.join(GOLDEN, case["input"]), etype=et, byte_scale=bs)
    blocks = dbo.parse_table(case["bytes"])
    out = b""
    for (names, D), blk in zip(mats, blocks):
        N, C, k, _ = dev.dbscan(D, len(names), e, minn, et, bs)
        out += dbo.format_table(names, N, C, k, e, minn, header=blk[0])
    assert out == case["bytes"]


def test_cli_default_options_and_long_forms(tmp_path):
    """-e 10 -N 1 are the defaults; long options, -o, and the ignored -H / -T."""
    ref = cli(["dbscan", "-i", "snp300.phy", "-e", "10", "-N", "1"])
    assert cli(["dbscan", "-i", "snp300.phy"]) == ref
    import ccphylo_amd as cg
    names, D = cg.load_phylip(os.path.join(GOLDEN, "snp300.phy"))[0]
    N, C, k = dbo.dbscan(D, len(names), 10.0, 1)
    assert ref == dbo.format_table(names, N, C, k, 10.0, 1)
    out = tmp_path / "o.txt"
    assert cli(["dbscan", "--input", "snp300.phy", "--max_distance", "10", "--min_neighbors=1", "-H", "-T",
                str(tmp_path), "--output", str(out)]) == b""
    assert out.read_bytes() == ref
    p = subprocess.run([cg.CLI_PATH, "--help"], capture_output=True, timeout=60)
    assert b"dbscan" in p.stdout


# ----------------------------------------------------------- random matrices
def random_lt(rng, n, etype, half, missing):
    """Far cells in [6, 12), about four near cells (0..2) a row, so that -N 4 and -N 9 meet core, border and
    lonely rows at every n; half: every cell may carry + 0.5 (byteScale 2 for the integer types); missing: -1
    cells (etype 8 / 4), which are neighbours at every threshold used here."""
    m = n * (n - 1) // 2
    v = rng.integers(6, 12, m).astype(np.float64)
    near = rng.random(m) < min(0.5, 4.0 / max(n, 1))
    v[near] = rng.integers(0, 3, int(near.sum()))
    if half:
        v += rng.integers(0, 2, m) * 0.5
    bs = 1.0
    if etype <= 2:
        bs = 2.0 if half else 1.0
        return (v * bs).astype(dbo.ETYPES[etype]), bs
    if missing:
        v[rng.random(m) < min(0.2, 1.0 / max(n, 1))] = -1.0
    return v.astype(dbo.ETYPES[etype]), bs


@pytest.mark.parametrize("etype", [8, 4, 2, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129, 257, N_TILES])
def test_random_matrices(dev, n, etype):
    rng = np.random.default_rng(7 * n + etype)
    seen_border = 0
    for half in (False, True):
        for missing in ((False, True) if etype >= 4 else (False,)):
            D, bs = random_lt(rng, n, etype, half, missing)
            e = 2.0 if not half else 2.5     # cells equal to the threshold count
            for minn in (0, 1, 2, 4, 9):
                seen_border += check(dev, D, n, e, minn, etype, bs)[4]
    if n >= 64:
        assert seen_border > 0


# -------------------------------------------------------------- line, dupes
def test_line_matrix(dev):
    n = 4097
    i, j = np.tril_indices(n, -1)
    D = (i - j).astype(np.float64)
    N, C, k, st, _ = check(dev, D, n, 1.0, 1)
    assert k == 1 and (C == 0).all()                  # one chain n - 1 deep
    assert st[2] <= 3 + (n - 1).bit_length() + 1      # count, classify, <= ceil(log2 n) + 1 jumps, roots
    N, C, k, _, _ = check(dev, D, n, 0.0, 1)
    assert k == n and (N == 0).all()
    N, C, k, _, border = check(dev, D, n, 1.0, 3)     # no row has 3 neighbours: the ends and all between are border rows
    assert border == n and k == n and N[0] == N[n - 1] == 1
    N, C, k, _, border = check(dev, D, n, 1.0, 2)     # here the two ends are the border rows
    assert border == 2 and k == 1


def test_all_zero_matrix(dev):
    n = 1500
    for etype in (8, 1):
        D = np.zeros(n * (n - 1) // 2, dtype=dbo.ETYPES[etype])
        N, C, k, _, _ = check(dev, D, n, 0.0, 4, etype)
        assert (N == n - 1).all() and k == 1


# ---------------------------------------------------------- threshold edges
def lt_from(n, cells, fill):
    D = np.full(n * (n - 1) // 2, fill, dtype=np.float64)
    for (i, j), v in cells.items():
        D[i * (i - 1) // 2 + j] = v
    return D


def test_threshold_edges(dev):
    n = 70
    cells = {(5, 2): 3.25, (69, 68): 3.25, (40, 1): 3.2500000000000004}
    D = lt_from(n, cells, 9.0)
    N, C, k, _, _ = check(dev, D, n, 3.25, 1)         # equal counts, one ulp above does not
    assert N.sum() == 4 and N[40] == 0 and k == n - 2
    # float 0.1f = 0.100000001490116... is not <= 0.1
    Df = lt_from(n, {(5, 2): 0.1, (9, 3): 0.0999}, 9.0).astype(np.float32)
    N, C, k, _, _ = check(dev, Df, n, 0.1, 1, etype=4)
    assert N[5] == 0 and N[9] == 1 and N[3] == 1
    # u16 with byteScale 100: cell 325 is 3.25
    Ds = lt_from(n, {(5, 2): 325, (9, 3): 326}, 900).astype(np.uint16)
    N, C, k, _, _ = check(dev, Ds, n, 3.25, 1, etype=2, bs=100.0)
    assert N[5] == 1 and N[9] == 0
    # -1 cells: neighbours at -e -1, none at -e -2
    Dm = lt_from(n, {(5, 2): -1.0, (9, 3): -1.0}, 9.0)
    N, C, k, _, _ = check(dev, Dm, n, -1.0, 1)
    assert N.sum() == 4
    N, C, k, _, _ = check(dev, Dm, n, -2.0, 1)
    assert N.sum() == 0 and k == n


# ------------------------------------------------------- hand-built borders
def test_border_cases(dev):
    # row 1's only neighbour is row 3 (core, in its column part): it stays its own cluster with N > 0
    D = lt_from(4, {(3, 1): 0, (3, 2): 0}, 9.0)
    N, C, k, _, border = check(dev, D, 4, 1.0, 2)
    assert list(N) == [0, 1, 1, 2] and list(C) == [0, 1, 2, 1] and border == 2 and k == 3
    # row 4 (border): first row-neighbour 0 is not core, the later one, 2, is; row 2 (core) has the border row 1
    # as its first neighbour and takes its cluster
    D = lt_from(5, {(4, 0): 0, (4, 2): 0, (2, 1): 0, (3, 2): 0}, 9.0)
    N, C, k, _, border = check(dev, D, 5, 1.0, 3)
    assert list(N) == [1, 1, 3, 1, 2] and list(C) == [0, 1, 1, 1, 1] and border == 4
    # the same past one 64-column step of the border kernel
    n = 200
    D = lt_from(n, {(150, 3): 0, (150, 140): 0, (140, 70): 0, (141, 140): 0, (199, 140): 0}, 9.0)
    N, C, k, _, _ = check(dev, D, n, 1.0, 3)
    assert N[150] == 2 and N[140] == 4 and C[150] == C[140] == 70


def test_invalid_arguments(dev):
    from ccphylo_amd import native
    D = np.zeros(3)
    for n, etype, bs in ((0, 8, 1.0), (-1, 8, 1.0), (3, 3, 1.0), (3, 2, 0.0), (3, 1, 0.0)):
        for fn_ in (dev.lib.ccg_dbscan, dev.lib.ccg_dbscan_dev):   # refused before the pointer is looked at
            with pytest.raises(native.CcgError, match="invalid argument"):
                dev._dbscan(fn_, D.ctypes.data, n, 10.0, 1, etype, bs)
    N, C, k, st = dev.dbscan(np.zeros(0), 1)
    assert list(N) == [0] and list(C) == [0] and k == 1 and st[2] == 0
    N, C, k, st = dev.dbscan(np.array([3.0]), 2, 3.0, 1)
    assert list(N) == [1, 1] and list(C) == [0, 0] and k == 1


# ------------------------------------------- device buffer, determinism
def test_device_buffer_untouched_then_tree(dev):
    import ccphylo_amd as cg
    rng = np.random.default_rng(5)
    n = 300
    D, _ = random_lt(rng, n, 8, True, False)
    p = dev.malloc(D.nbytes)
    try:
        dev.h2d(p, D)
        N, C, k, _ = dev.dbscan_dev(p, n, 2.5, 4)
        rN, rC, rk = dbo.dbscan(D, n, 2.5, 4)
        assert (N == rN).all() and (C == rC).all() and k == rk
        back = np.empty_like(D)
        dev.d2h(back, p)
        assert back.tobytes() == D.tobytes()
        joins, fn, fd, _ = dev.tree_dev(p, n, method=cg.CCG_TREE_DNJ)
    finally:
        dev.free(p)
    rj, rfn, rfd, _ = dev.tree(D, n, method=cg.CCG_TREE_DNJ)
    assert joins.tobytes() == rj.tobytes() and fn == rfn and fd == rfd


def test_deterministic(dev):
    rng = np.random.default_rng(11)
    D, _ = random_lt(rng, N_TILES, 4, False, True)
    a = dev.dbscan(D, N_TILES, 2.0, 4, etype=4)
    b = dev.dbscan(D, N_TILES, 2.0, 4, etype=4)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2] and a[3][:3] == b[3][:3]


# ---------------------------------------------------------------- fused path
# (input, dist options, -e, -N): thresholds near the low quantiles of each matrix, so that clusters form and
# stay apart; msa64 with -f 3 -P 10 has missing (-1) cells, which are neighbours
FUSED = [("msa64.fsa", [], "50", "2"), ("msa64.fsa", ["-p"], "50", "4"), ("msa64.fsa", ["-W", "1000"], "25.9", "2"),
         ("msa64.fsa", ["-f", "3", "-P", "10"], "50", "2"),
         ("msa300.fsa", [], "3", "2"), ("msa300.fsa", ["-p"], "2", "4"), ("msa300.fsa", ["-W", "1000"], "12.61", "2"),
         ("msa300.fsa", ["-f", "3", "-P", "10"], "26", "2")]


@pytest.mark.parametrize("msa,opts,e,minn", FUSED, ids=[f[0][:-4] + "".join(f[1]) for f in FUSED])
def test_fused_dist_dbscan(tmp_path, msa, opts, e, minn):
    src = os.path.join(GOLDEN, msa)
    phy, out = tmp_path / "d.phy", tmp_path / "fused.txt"
    phy.write_bytes(cli(["dist", "-i", src] + opts))
    prec = ["-p"] if "-p" in opts else []
    two = cli(["dbscan", "-i", str(phy), "-e", e, "-N", minn] + prec)
    assert cli(["dist", "-i", src] + opts + ["--dbscan", str(out), "--max_distance", e, "--min_neighbors", minn]) == b""
    assert two and out.read_bytes() == two
    blk = dbo.parse_table(two)[0]
    print(msa, opts, "n", blk[1], "clusters", blk[2])
    assert 1 < blk[2] < blk[1]


@pytest.mark.parametrize("msa", ["msa64.fsa", "msa300.fsa"])
def test_fused_dbscan_and_tree(tmp_path, msa):
    src = os.path.join(GOLDEN, msa)
    phy, out, nwk = tmp_path / "d.phy", tmp_path / "fused.txt", tmp_path / "fused.nwk"
    phy.write_bytes(cli(["dist", "-i", src, "-W", "1000"]))
    e = "25.9" if msa == "msa64.fsa" else "12.61"
    two_db = cli(["dbscan", "-i", str(phy), "-e", e, "-N", "2"])
    two_tree = cli(["tree", "-i", str(phy)])
    cli(["dist", "-i", src, "-W", "1000", "--dbscan", str(out), "--max_distance", e, "--min_neighbors", "2",
         "--tree", str(nwk)])
    assert out.read_bytes() == two_db
    assert nwk.read_bytes() == two_tree


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["-s", "100"]], ids=["gpus2", "s100"])
def test_fused_refusals(tmp_path, extra):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH, "dist", "-i", os.path.join(GOLDEN, "msa64.fsa"), "--dbscan", str(tmp_path / "o.txt")]
                       + extra, capture_output=True, timeout=120)
    assert p.returncode != 0
    assert b"not supported" in p.stderr
    assert len([ln for ln in p.stderr.split(b"\n") if ln.strip()]) == 1
