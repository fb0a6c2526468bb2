"""GPU: `nwck2phy` and `phycmp` on the gfx950 engine (ccg_nwck_ltd / ccg_ltd_cmp,
their _dev forms, the two CLI subcommands and the fused `tree --phycmp`).

Replay: every cell bitwise equal to the restatement (tests/fit_oracle.py) and,
on the golden trees, to the reference's bytes (tests/golden/fit).  The splits
with up to PREFIX rows run in one block of PREFIX threads, every later split is
a launch of blocks of STEP threads (NW_PREFIX / NW_BLOCK in csrc/nwck.hip).

Comparison: every sum within 1e-13 sum|term| of math.fsum (the contract of
ccg_ltd_cmp; its pairwise reduction is bounded far below that), linf exact, two
runs bit-identical.  A thread takes VEC cells a pass, a block BLOCK * VEC, the
grid GRID * BLOCK * VEC (CMP_VEC / CMP_BLOCK / CMP_GRID in csrc/ltdcmp.hip); a
matrix has n(n-1)/2 cells, so each boundary is taken by the two n whose cell
counts lie closest on either side of it."""
import gzip
import json
import math
import os
import subprocess

import numpy as np
import pytest

import fit_oracle as fo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PREFIX, STEP = 1024, 256
VEC, BLOCK, GRID = 4, 256, 1024
FIT = os.path.join(GOLDEN, "fit")
with open(os.path.join(FIT, "fit.json")) as f:
    CASES = json.load(f)["cases"]
NWCK = [c for c in CASES if c["cmd"] == "nwck2phy"]
PHYCMP = [c for c in CASES if c["cmd"] == "phycmp"]
LIMBS = np.array([-1.0, -0.25, 0.0, 0.0, 0.125, 1.0, 2.0 / 3, 0.1, 3.3, 1e-7, 12345.678])


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def run(args, cwd=GOLDEN):
    import ccphylo_amd as cg
    return subprocess.run([cg.CLI_PATH] + args, cwd=cwd, capture_output=True, timeout=300)


def golden_out(case):
    if not case["out"]:
        return b""
    with gzip.open(os.path.join(FIT, case["out"])) as f:
        return f.read()


# ------------------------------------------------------------------ replay
def make_splits(shape, n, seed):
    """n - 1 splits of the given shape; limbs from LIMBS unless the shape fixes them"""
    from ccphylo_amd import native
    rng = np.random.default_rng(seed)
    sp = np.zeros(n - 1, dtype=native.SPLIT_DTYPE)
    s = np.arange(n - 1)
    sp["Li"] = rng.choice(LIMBS, n - 1)
    sp["Lj"] = rng.choice(LIMBS, n - 1)
    if shape == "caterpillar":       # the root keeps splitting: row 0 and column 0 every time
        sp["org"] = 0
        sp["Li"] = np.abs(sp["Li"])
        sp["Lj"] = np.abs(sp["Lj"])
    elif shape == "caterpillar_deep":   # the newest row splits: org = s, the longest row walk
        sp["org"] = s
    elif shape == "balanced":        # breadth first: org runs over the rows of each level
        sp["org"] = s - (1 << np.floor(np.log2(s + 1)).astype(np.int64)) + 1
        sp["Li"] = np.abs(sp["Li"]) + 0.5
        sp["Lj"] = np.abs(sp["Lj"]) + 0.5
    elif shape == "star":            # nwck2phy's own star: Li = 0, Lj as parsed
        sp["org"] = 0
        sp["Li"] = 0
    elif shape == "columns":         # org > 0 and small: long strided column walks
        sp["org"] = np.minimum(s, rng.integers(1, 8, n - 1))
    elif shape == "negative":        # Li < 0 / Lj < 0 / -1 propagation, any org
        sp["org"] = rng.integers(0, s + 1)
        sp["Li"] = rng.choice([-1.0, -0.5, 0.0, 1.5], n - 1)
        sp["Lj"] = rng.choice([-1.0, -2.5, 0.0, 0.75], n - 1)
    elif shape == "zero":
        sp["org"] = rng.integers(0, s + 1)
        sp["Li"] = 0
        sp["Lj"] = 0
    else:
        assert shape == "random"
        sp["org"] = rng.integers(0, s + 1)
    return sp


def as_list(sp):
    return [(int(o), float(a), float(b)) for o, a, b in sp]


SIZES = [2, 3, 4, STEP - 1, STEP, STEP + 1, 2 * STEP + STEP // 2 + 1,    # inside the one-block prefix
         PREFIX - 1, PREFIX, PREFIX + 1,     # the last split of n = PREFIX + 1 fills the block: no step launch yet
         PREFIX + 2,                         # the first step launch (m = PREFIX + 1 rows)
         PREFIX + STEP, PREFIX + STEP + 2]   # a step's last block full / one cell into the next
REPLAY = [(sh, n) for n in SIZES for sh in ("random", "negative")]
REPLAY += [(sh, n) for sh in ("caterpillar", "caterpillar_deep", "balanced", "star", "columns", "zero")
           for n in (4, STEP + 1, PREFIX + STEP + 2)]
REPLAY += [("random", 1500), ("columns", 2 * PREFIX + PREFIX // 2 + 1)]


@pytest.mark.parametrize("shape,n", REPLAY, ids=["%s-%d" % r for r in REPLAY])
def test_replay_bitwise(dev, shape, n):
    sp = make_splits(shape, n, 1000 + n)
    for et in (8, 4):
        want = fo.replay(as_list(sp), et) if n <= 4 else fo.replay_np(as_list(sp), et)
        got = dev.nwck_ltd(sp, et)
        assert got.dtype == want.dtype and (got.view(np.uint8) == want.view(np.uint8)).all(), (shape, n, et)
    ms, launches = dev.last_nwck()
    assert launches == 1 + max(0, n - 1 - PREFIX)


def test_replay_takes_both_roundings():
    """the float replay is not the double one rounded at the end"""
    sp = make_splits("random", 300, 3)
    a, b = fo.replay_np(as_list(sp), 4), fo.replay_np(as_list(sp), 8).astype(np.float32)
    assert (a != b).any()


@pytest.mark.parametrize("n", [2, PREFIX + 1, PREFIX + 2, 1500])
def test_replay_dev_entry(dev, n):
    sp = make_splits("random", n, 77)
    for et in (8, 4):
        want = fo.replay_np(as_list(sp), et)
        p = dev.malloc(want.nbytes + 64)
        try:
            guard = np.full(want.size + 64 // et, 7, dtype=want.dtype)
            dev.h2d(p, guard)
            dev.nwck_ltd_dev(sp, p, et)
            got = np.zeros_like(guard)
            dev.d2h(got, p)
        finally:
            dev.free(p)
        assert (got[:want.size].view(np.uint8) == want.view(np.uint8)).all()
        assert (got[want.size:] == 7).all()   # nothing behind the last row (the reference writes one cell past each)


def test_replay_refusals(dev):
    import ccphylo_amd as cg
    sp = make_splits("random", 10, 1)
    for et in (2, 1):
        with pytest.raises(cg.CcgError, match="not supported"):
            dev.nwck_ltd(sp, et)
    sp["org"][4] = 6   # row 6 does not exist at split 4
    with pytest.raises(cg.CcgError, match="invalid argument"):
        dev.nwck_ltd(sp, 8)
    assert dev.nwck_ltd(sp[:0], 8).size == 0


def parsed_lines(case):
    from ccphylo_amd import native
    with open(os.path.join(GOLDEN, case["args"][2]), "rb") as f:
        data = f.read()
    pos = 0
    while True:
        p = data.find(b"(", pos)
        e = data.find(b"\n", p) if p >= 0 else -1
        if e < 0:
            return
        try:
            yield native.newick_splits(data[pos:e])
        except native.CcgError:
            return
        pos = e + 1


@pytest.mark.parametrize("case", NWCK, ids=[c["name"] for c in NWCK])
def test_nwck2phy_golden(dev, case):
    """host entry, _dev entry and the CLI each give the reference's bytes"""
    flag = int(case["args"][case["args"].index("-f") + 1]) if "-f" in case["args"] else 1
    et = case["etype"]
    want = golden_out(case)
    host, devb = b"", b""
    for header, names, sp in parsed_lines(case):
        D = dev.nwck_ltd(sp, et)
        host += fo.print_phy(header, names, D, flag)
        p = dev.malloc(max(D.nbytes, 8))
        try:
            dev.nwck_ltd_dev(sp, p, et)
            D2 = np.zeros_like(D)
            dev.d2h(D2, p)
        finally:
            dev.free(p)
        devb += fo.print_phy(header, names, D2, flag)
    assert host == want
    assert devb == want
    p = run(list(case["args"]))
    assert (p.returncode, p.stderr.decode("latin-1")) == (case["rc"], case["stderr"])
    assert p.stdout == want


# ------------------------------------------------------------------ comparison
def n_around(cells):
    """the two n whose n(n-1)/2 lie closest below (or at) and above `cells`"""
    n = int((1 + math.isqrt(1 + 8 * cells)) // 2)
    while n * (n - 1) // 2 > cells:
        n -= 1
    return [n, n + 1]


CMP_N = sorted(set([2, 3, 12, 400] + n_around(VEC) + n_around(BLOCK * VEC)))
CMP_BIG = [(1500, 8), (1500, 4)] + [(n, et) for n, et in zip(n_around(GRID * BLOCK * VEC), (8, 4))]
_refs = {}


def matrices(n, et, seed=0):
    rng = np.random.default_rng(n * 10 + et + seed)
    m = n * (n - 1) // 2
    dt = np.float64 if et == 8 else np.float32
    A = (rng.random(m) * 10).astype(dt)
    B = (A * (1 + 0.3 * rng.standard_normal(m))).astype(dt)
    A[rng.random(m) < 0.05] = -1          # missing cells are plain numbers
    B[rng.random(m) < 0.05] = -1
    same = rng.random(m) < 0.1             # chi2 skips a == b
    B[same] = A[same]
    return A, B


def reference(n, et, permname):
    """(A, B, perm, sums, magnitudes), computed once"""
    key = (n, et, permname)
    if key not in _refs:
        A, B = matrices(n, et)
        rng = np.random.default_rng(n)
        perm = {"none": None, "identity": np.arange(n), "reversal": np.arange(n)[::-1].copy(),
                "random": rng.permutation(n)}[permname]
        Bp = B if perm is None else fo.permute_lt(B, n, perm)
        _refs[key] = (A, B, perm) + fo.cmp_sums(A, Bp, et)
    return _refs[key]


def check_sums(got, want, mags):
    for k in fo.SUM_NAMES:
        if k == "linf":
            assert got[k] == want[k]
        else:
            assert abs(got[k] - want[k]) <= 1e-13 * mags[k], (k, got[k], want[k], mags[k])


@pytest.mark.parametrize("permname", ["none", "identity", "reversal", "random"])
@pytest.mark.parametrize("et", [8, 4])
@pytest.mark.parametrize("n", CMP_N)
def test_cmp_sums(dev, n, et, permname):
    A, B, perm, want, mags = reference(n, et, permname)
    got, met = dev.ltd_cmp(A, B, n, et, perm)
    check_sums(got, want, mags)
    again, _ = dev.ltd_cmp(A, B, n, et, perm)
    assert [np.float64(got[k]).tobytes() for k in fo.SUM_NAMES] == [np.float64(again[k]).tobytes() for k in fo.SUM_NAMES]
    cells = n * (n - 1) // 2
    for k in fo.METRIC_NAMES:
        w = fo.metric(got, cells, k)
        assert met[k] == w or (math.isnan(met[k]) and math.isnan(w))
    if permname == "identity":
        none, _ = dev.ltd_cmp(A, B, n, et, None)
        assert none == got   # the same cells in the same order


@pytest.mark.parametrize("n,et", CMP_BIG, ids=["%d-%d" % c for c in CMP_BIG])
def test_cmp_sums_grid_pass(dev, n, et):
    """one side and the other of a whole pass of the grid, and 1500 taxa; device pointers"""
    permname = "random" if n == 1500 else "none"
    A, B, perm, want, mags = reference(n, et, permname)
    pa, pb = dev.malloc(A.nbytes), dev.malloc(B.nbytes)
    try:
        dev.h2d(pa, A)
        dev.h2d(pb, B)
        got, _ = dev.ltd_cmp_dev(pa, pb, n, et, perm)
        again, _ = dev.ltd_cmp_dev(pa, pb, n, et, perm)
        A2, B2 = np.zeros_like(A), np.zeros_like(B)
        dev.d2h(A2, pa)
        dev.d2h(B2, pb)
    finally:
        dev.free(pa)
        dev.free(pb)
    check_sums(got, want, mags)
    assert got == again
    assert (A2.view(np.uint8) == A.view(np.uint8)).all() and (B2.view(np.uint8) == B.view(np.uint8)).all()
    host, _ = dev.ltd_cmp(A, B, n, et, perm)
    assert host == got


def test_cmp_refusals(dev):
    import ccphylo_amd as cg
    A, B = matrices(12, 8)
    for bad in ([0] * 12, list(range(11)) + [12], list(range(11)) + [-1], [1, 1] + list(range(2, 12))):
        with pytest.raises(cg.CcgError, match="invalid argument"):
            dev.ltd_cmp(A, B, 12, 8, bad)
    with pytest.raises(cg.CcgError, match="not supported"):
        dev.ltd_cmp(A.astype(np.uint16), B.astype(np.uint16), 12, 2)
    with pytest.raises(cg.CcgError, match="invalid argument"):
        dev.ltd_cmp(A[:0], B[:0], 1, 8)


@pytest.mark.parametrize("case", PHYCMP, ids=[c["name"] for c in PHYCMP])
def test_phycmp_golden(case):
    p = run(list(case["args"]))
    assert (p.returncode, p.stdout.decode(), p.stderr.decode()) == (case["rc"], case["stdout"], case["stderr"])


def test_phycmp_flags_and_one_entry(tmp_path):
    case, = [c for c in PHYCMP if c["name"] == "perturbed"]
    lines = case["stdout"].splitlines(True)
    p = run(["phycmp", "-i"] + case["files"])
    assert p.returncode == 0 and p.stdout.decode() == lines[0]          # -f defaults to 1
    p = run(["phycmp", "-f", "40", "-o", str(tmp_path / "o")] + case["files"])   # files as non-options
    assert p.returncode == 0 and p.stdout == b""
    assert open(tmp_path / "o").read() == lines[3] + lines[5]
    one = tmp_path / "one.phy"
    one.write_text("         1\nsolo\n         1\nsolo\n")
    p = run(["phycmp", "-i", str(one)])
    assert p.returncode == 1 and p.stdout == b"" and b"one entry" in p.stderr


def test_phycmp_by_name():
    """a shuffled copy of the second matrix gives the lines of the unshuffled pair"""
    for suffix, popt in (("", []), ("_p", ["-p"])):
        case, = [c for c in PHYCMP if c["name"] == "missing" + suffix]
        p = run(["phycmp", "-f", "127", "--by_name"] + popt + ["-i", "miss80.phy", "fit/in_miss80_pert_shuf.phy.gz"])
        assert (p.returncode, p.stdout.decode()) == (0, case["stdout"]), p.stderr
        p = run(["phycmp", "-f", "127", "--by_name"] + popt + ["-i"] + case["files"])
        assert (p.returncode, p.stdout.decode()) == (0, case["stdout"])
    # the tree's matrix of the same taxa, in split order: maps; the plain comparison refuses it
    p = run(["phycmp", "--by_name", "-i", "miss80.phy", "fit/miss80_dnj.phy.gz"])
    assert p.returncode == 0 and p.stdout.startswith(b"cos:\t")
    p = run(["phycmp", "-i", "miss80.phy", "fit/miss80_dnj.phy.gz"])
    assert (p.returncode, p.stderr) == (1, b"Matrices has different entries.\n")


def test_phycmp_by_name_refusals(tmp_path):
    with gzip.open(os.path.join(FIT, "in_miss80_pert_shuf.phy.gz")) as f:
        rows = f.read().split(b"\n")
    first, second = rows[1].split(b"\t")[0], rows[2].split(b"\t")[0]
    other, twice = tmp_path / "other.phy", tmp_path / "twice.phy"
    other.write_bytes(b"\n".join([rows[0], b"nobody"] + rows[2:]))
    twice.write_bytes(b"\n".join([rows[0], second] + rows[2:]))
    p = run(["phycmp", "--by_name", "-i", "miss80.phy", str(other)])
    assert p.returncode == 1 and p.stdout == b"" and b"in one matrix only" in p.stderr and first in p.stderr
    p = run(["phycmp", "--by_name", "-i", "miss80.phy", str(twice)])
    assert p.returncode == 1 and p.stdout == b"" and b"repeats" in p.stderr and second in p.stderr


# ------------------------------------------------------------------ fused
def test_tree_phycmp_fused(dev, tmp_path):
    from ccphylo_amd import native
    t, f = str(tmp_path / "t.nwk"), str(tmp_path / "fit.txt")
    p = run(["tree", "-i", "euc400.phy.gz", "-m", "dnj", "-o", t, "--phycmp", f, "--phycmp_flag", "127"])
    assert p.returncode == 0, p.stderr
    with open(os.path.join(GOLDEN, "euc400_dnj.out"), "rb") as g:
        assert open(t, "rb").read() == g.read()          # the tree is the golden tree
    fused = open(f).read()
    assert fused.count("\n") == 7
    # the same through the text: nwck2phy (all digits kept), then phycmp --by_name
    phy = str(tmp_path / "t.phy")
    assert run(["nwck2phy", "-i", t, "-o", phy, "-x", "30"]).returncode == 0
    p = run(["phycmp", "-f", "127", "--by_name", "-i", "euc400.phy.gz", phy])
    assert (p.returncode, p.stdout.decode()) == (0, fused), p.stderr
    # the same through Python: parse, replay, map by name, compare
    (names, A), = native.load_phylip(os.path.join(GOLDEN, "euc400.phy.gz"))
    line = open(t, "rb").read().rstrip(b"\n")
    _, leaves, sp = native.newick_splits(line)
    W = dev.nwck_ltd(sp, 8)
    row = {nm: k for k, nm in enumerate(leaves)}
    perm = [row[nm.encode()] for nm in names]
    sums, met = dev.ltd_cmp(A, W, len(names), 8, perm)
    assert fo.phycmp_lines(sums, len(A), 127) == fused
    assert "".join("%s:\t%f\n" % (k, met[k]) for k in fo.METRIC_NAMES) == fused
    # a tree of Euclidean points distorts them (path lengths are no Euclidean metric) but follows them
    assert met["l1"] > 0 and met["p"] > 0.5
    # --phycmp_flag defaults to 1
    p = run(["tree", "-i", "euc400.phy.gz", "-m", "dnj", "-o", t, "--phycmp", f])
    assert p.returncode == 0 and open(f).read() == fused.splitlines(True)[0]


def test_tree_phycmp_two_matrices_and_float(tmp_path):
    t, f = str(tmp_path / "t.nwk"), str(tmp_path / "fit.txt")
    p = run(["tree", "-i", "multi.phy", "-m", "dnj", "-o", t, "--phycmp", f, "--phycmp_flag", "65"])
    assert p.returncode == 0, p.stderr
    with open(os.path.join(GOLDEN, "multi_dnj.out"), "rb") as g:
        assert open(t, "rb").read() == g.read()
    lines = open(f).read().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["cos", "p", "cos", "p"]
    p = run(["tree", "-i", "euc400.phy.gz", "-p", "-o", t, "--phycmp", f, "--phycmp_flag", "127"])
    assert p.returncode == 0, p.stderr
    with open(os.path.join(GOLDEN, "euc400_p.out"), "rb") as g:
        assert open(t, "rb").read() == g.read()
    assert open(f).read().count("\n") == 7


def test_tree_phycmp_refuses_after_the_tree(tmp_path):
    t, f = str(tmp_path / "t.nwk"), str(tmp_path / "fit.txt")
    p = run(["tree", "-i", "miss80.phy", "-m", "nj", "-o", t, "--phycmp", f])
    with open(os.path.join(GOLDEN, "miss80_nj.out"), "rb") as g:
        assert open(t, "rb").read() == g.read()          # the tree is kept
    assert p.returncode != 0
    case, = [c for c in NWCK if c["name"] == "miss80_nj"]
    assert case["stderr"].encode("latin-1") in p.stderr  # nwck2phy's own message for that string
    assert open(f).read() == ""
