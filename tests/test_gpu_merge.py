"""GPU: `merge` on the gfx950 engine (ccg_ltd_merge / _dev, ccg_ltd_merge_close /
_dev, the `ccphylo merge` subcommand and its fused --tree).

Engine: D and N bitwise equal (compared as integers, so the sign of zero
counts) to the restatement (tests/merge_oracle.py) after every batch and after
the close, under the scatter form (plan 1), the gather form (plan 2) and the
automatic choice (plan 0).  A thread owns VEC cells and a block BLOCK * VEC
(MRG_VEC / MRG_BLOCK in csrc/merge.hip), a call takes up to MAX_SRC sources
(MRG_MAX_SRC); a union of n rows has n(n-1)/2 cells, so each boundary is taken
by the two n whose cell counts lie closest on either side of it.

CLI: every golden of tests/golden/merge byte for byte; outside the envelope in
which the reference is reliable (a first matrix of more than 63 entries, more
than 126 names), against the restatement."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import merge_oracle as mo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

VEC, BLOCK, MAX_SRC = 4, 256, 16
MERGE = os.path.join(GOLDEN, "merge")
with open(os.path.join(MERGE, "merge.json")) as f:
    CASES = json.load(f)["cases"]
VALUES = np.array([0.0, -1.0, 2.0 / 3.0, 1e-7, 12345.678, 1e-40, 0.25, 17.0, -0.0, 99.999999])   # 1e-40: a float subnormal
WEIGHTS = np.array([0.0, 1.0, 2.0, 1500.0, 0.5, 123456.0, 3.0, 1e-3])
UINT = {8: np.uint64, 4: np.uint32}


def sizes_around(cells):
    """the two n whose cell counts lie closest below-or-at and above `cells`"""
    n = 2
    while mo.tri(n + 1) <= cells:
        n += 1
    return [n, n + 1]


SIZES = sorted({2, 3, *sizes_around(VEC), *sizes_around(BLOCK * VEC), *sizes_around(2 * BLOCK * VEC)})
assert SIZES == [2, 3, 4, 45, 46, 64, 65]


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def run(args, cwd=GOLDEN):
    import ccphylo_amd as cg
    return subprocess.run([cg.CLI_PATH] + args, cwd=cwd, capture_output=True, timeout=300)


def gz_read(name):
    with gzip.open(os.path.join(MERGE, name), "rb") as f:
        return f.read()


def bits(a):
    return a.view(UINT[a.dtype.itemsize])


# ------------------------------------------------------------------ engine
PATTERNS = ("identity", "reversed", "perm", "subset", "disjoint", "interleaved", "one", "two")


def make_idx(pattern, n_prev, n, rng):
    """the union rows of one source of a batch that grows the union from n_prev to n rows"""
    new = np.arange(n_prev, n)
    if pattern == "identity":
        return np.arange(n)
    if pattern == "reversed":
        return np.arange(n)[::-1]
    if pattern == "perm":
        return rng.permutation(n)
    if pattern == "subset":                      # a strict subset, in random order
        return rng.permutation(n)[:max(1, n // 2)]
    if pattern == "disjoint" and len(new):       # none of the rows any earlier batch saw
        return rng.permutation(new)
    if pattern == "interleaved" and len(new) and n_prev:   # new rows between old ones
        k = min(len(new), n_prev)
        out = np.empty(2 * k, dtype=np.int64)
        out[0::2], out[1::2] = rng.permutation(n_prev)[:k], new[:k]
        return out
    if pattern == "one":
        return rng.permutation(n)[:1]
    return rng.permutation(n)[:2]                # "two", and the patterns a batch without growth cannot form


def make_batches(n, K, et, weighted, seed):
    """[(n_prev, n_b, [(d, w, idx)])]: K sources in calls of up to MAX_SRC, the union growing to n"""
    rng = np.random.default_rng(seed)
    dt = mo.DTYPES[et]
    nb = -(-K // MAX_SRC)
    grow = [max(2, n - (n // 3) * (nb - 1 - b)) for b in range(nb)]   # n_b, the last one n
    out, n_prev, k = [], 0, 0
    for b in range(nb):
        srcs = []
        for _ in range(min(MAX_SRC, K - b * MAX_SRC)):
            idx = make_idx(PATTERNS[(k + seed) % len(PATTERNS)], n_prev, grow[b], rng).astype(np.int32)
            cells = mo.tri(len(idx))
            d = rng.choice(VALUES, cells).astype(dt)
            w = rng.choice(WEIGHTS, cells).astype(dt) if weighted else None
            srcs.append((d, w, idx))
            k += 1
        out.append((n_prev, grow[b], srcs))
        n_prev = grow[b]
    return out


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("K", [1, MAX_SRC, MAX_SRC + 1, 2 * MAX_SRC + 1])
@pytest.mark.parametrize("weighted", [True, False], ids=["w", "jl"])
@pytest.mark.parametrize("et", [8, 4], ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_engine_matches_restatement_bitwise(dev, n, et, weighted, K, first):
    import ccphylo_amd as cg
    dt = mo.DTYPES[et]
    batches = make_batches(n, K, et, weighted, seed=1000 * n + K + et)
    got = {p: (np.full(mo.tri(n), 7, dtype=dt), np.full(mo.tri(n), 7, dtype=dt)) for p in (0, 1, 2)}   # 7: the call zero-fills
    D, N = np.zeros(0, dtype=dt), np.zeros(0, dtype=dt)
    for b, (n_prev, n_b, srcs) in enumerate(batches):
        D, N = mo.grow(D, n_b), mo.grow(N, n_b)
        for s, (d, w, idx) in enumerate(srcs):
            mo.apply(D, N, d, w, idx, first=first and b == 0 and s == 0)
        cells = mo.tri(n_b)
        any_cell = any(len(idx) > 1 for _, _, idx in srcs)
        for p, (Dg, Ng) in got.items():
            dev.ltd_merge(Dg, Ng, n_b, srcs, n_prev, etype=et, weighted=weighted, first=first and b == 0, plan=p)
            taken = dev.last_merge_plan()
            assert taken == 0 if not any_cell else taken == p if p else taken in (1, 2)
            assert (bits(Dg[:cells]) == bits(D)).all() and (bits(Ng[:cells]) == bits(N)).all(), (b, p)
            assert (Dg[cells:] == 7).all() and (Ng[cells:] == 7).all()      # nothing past the union's rows
    Dc = mo.close(D, N)
    for p, (Dg, Ng) in got.items():
        dev.ltd_merge_close(Dg, Ng, n, etype=et)
        assert (bits(Dg) == bits(Dc)).all() and (bits(Ng) == bits(N)).all(), p
    assert cg.MERGE_MAX_SRC == MAX_SRC


def test_interleaved_and_disjoint_patterns_are_formed():
    """the generator does produce the growth patterns (they fall back where a batch cannot form them)"""
    rng = np.random.default_rng(0)
    d = make_idx("disjoint", 40, 65, rng)
    assert d.min() >= 40 and len(d) == 25
    i = make_idx("interleaved", 40, 65, rng)
    assert (i[0::2] < 40).all() and (i[1::2] >= 40).all() and len(set(i)) == len(i)
    assert len(i) == 50 and len(make_idx("interleaved", 0, 65, rng)) == 2     # no old rows: falls back
    n_prevs = [b[0] for b in make_batches(65, 2 * MAX_SRC + 1, 8, True, 1)]
    assert n_prevs[0] == 0 and n_prevs == sorted(set(n_prevs)) and len(n_prevs) == 3   # the union grows between batches


@pytest.mark.parametrize("et", [8, 4], ids=["f64", "f32"])
def test_close_divides_correctly_rounded_and_keeps_denormals(dev, et):
    dt = mo.DTYPES[et]
    tiny = np.finfo(dt).smallest_subnormal
    num = np.array([1, 2, 1e-40 if et == 4 else 5e-310, tiny * 3, 1, -0.0, 5, 0, 12345.678, 7, 1e-7, -3], dtype=dt)
    den = np.array([3, 3, 3, 2, 0, 2, -0.0, 0, 2.0 / 3.0, 7, 3, 1500], dtype=dt)
    for n in (2, 3, 4, 5):                       # 1, 3, 6, 10 cells: short tails and one whole vector
        cells = mo.tri(n)
        D, N = num[:cells].copy(), den[:cells].copy()
        want = mo.close(D, N)
        dev.ltd_merge_close(D, N, n, etype=et)
        assert (bits(D) == bits(want)).all() and (bits(N) == bits(den[:cells])).all()
    assert want[0] == dt(1) / dt(3) and want[2] != 0 and want[4] == -1 and want[6] == -1


@pytest.mark.parametrize("et,weighted", [(8, True), (4, False)])
def test_two_runs_give_identical_bits(dev, et, weighted):
    dt = mo.DTYPES[et]
    outs = []
    for _ in range(2):
        D, N = np.zeros(mo.tri(65), dtype=dt), np.zeros(mo.tri(65), dtype=dt)
        for n_prev, n_b, srcs in make_batches(65, 2 * MAX_SRC + 1, et, weighted, seed=77):
            dev.ltd_merge(D, N, n_b, srcs, n_prev, etype=et, weighted=weighted, first=n_prev == 0)
        dev.ltd_merge_close(D, N, 65, etype=et)
        outs.append((bits(D).copy(), bits(N).copy()))
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()


def test_errors_leave_the_union_untouched(dev):
    from ccphylo_amd import native
    lib = dev.lib
    n = 6
    D0 = np.arange(mo.tri(n), dtype=np.float64) + 0.5
    d = np.ones(3)
    keep = []

    def call(idx_lists, etype=8, nsrc=None, n_prev=n):
        a = native.MergeArgs(etype=etype, weighted=1, first=0, plan=0, nsrc=len(idx_lists) if nsrc is None else nsrc,
                             n_prev=n_prev)
        for s, idx in enumerate(idx_lists[:native.MERGE_MAX_SRC]):
            idx = np.asarray(idx, dtype=np.int32)
            keep.append(idx)
            a.src[s] = native.MergeSrc(d.ctypes.data, d.ctypes.data, len(idx), idx.ctypes.data)
        D, N = D0.copy(), D0.copy() * 2
        rc = lib.ccg_ltd_merge(dev.h, C.byref(a), D.ctypes.data, N.ctypes.data, n)
        assert (D == D0).all() and (N == D0 * 2).all()
        return rc, lib.ccg_strerror(-4)

    rc, msg = call([[0, 3, 3]])
    assert rc == -1 and b"repeated" in msg
    rc, msg = call([[0, 1, n]])
    assert rc == -1 and b"outside the union" in msg
    rc, msg = call([[0, 1, -1]])
    assert rc == -1 and b"outside the union" in msg
    rc, msg = call([], nsrc=0)
    assert rc == -1 and b"nsrc" in msg
    rc, msg = call([[0, 1, 2]] * MAX_SRC, nsrc=MAX_SRC + 1)
    assert rc == -1 and b"nsrc" in msg
    rc, msg = call([[0, 1, 2]], n_prev=n + 1)
    assert rc == -1 and b"n_prev" in msg
    for et in (2, 1):
        rc, msg = call([[0, 1, 2]], etype=et)
        assert rc == -5 and b"short / byte" in msg
    assert call([[0, 1, 2]], etype=3)[0] == -1
    D = D0.copy()
    assert lib.ccg_ltd_merge_close(dev.h, D.ctypes.data, D.ctypes.data, n, 2) == -5 and (D == D0).all()


def test_valid_call_after_the_refusals_still_works(dev):
    """the same sources as the refusals' fixture, valid: D changes as the restatement says"""
    D, N = np.zeros(mo.tri(6)), np.zeros(mo.tri(6))
    De, Ne = D.copy(), N.copy()
    src = (np.array([1.5, 2.5, 3.5]), np.array([2.0, 0.0, 4.0]), np.array([5, 0, 3], dtype=np.int32))
    dev.ltd_merge(D, N, 6, [src], 0, first=True)
    mo.apply(De, Ne, *src, first=True)
    assert (bits(D) == bits(De)).all() and (bits(N) == bits(Ne)).all() and dev.last_merge_ms() >= 0


def test_cells_past_2_to_31_through_the_dev_entries(dev):
    """a float union of 65 600 rows (2.15e9 cells, 8.6 GB a buffer) zeroed on the device by the first
    call (n_prev = 0); one 3-row source whose three cells all lie past index 2^31, under each plan;
    only those cells and three neighbours are read back, and no large host array exists"""
    n = 65600
    cells = mo.tri(n)
    idx = np.array([0, n - 2, n - 1], dtype=np.int32)
    f = mo.union_cells(idx)
    assert cells > 2 ** 31 and (f > 2 ** 31).all() and f[2] == cells - 1
    sel = [int(x) for x in f] + [int(f[0]) + 1, int(f[1]) + 1, int(f[2]) - 1]
    d = np.array([2.0 / 3.0, 1e-7, 12345.678, 0, 0, 0, 0, 0], dtype=np.float32)     # 32 bytes each
    w = np.array([3.0, 1500.0, 0.5, 0, 0, 0, 0, 0], dtype=np.float32)
    ptrs = [dev.malloc(cells * 4), dev.malloc(cells * 4), dev.malloc(d.nbytes), dev.malloc(w.nbytes)]
    Dp, Np, dp, wp = ptrs

    def read(base):
        out = np.zeros(len(sel), dtype=np.float32)
        for k, c in enumerate(sel):
            dev.d2h(out[k:k + 1], base + 4 * c)
        return out
    try:
        dev.h2d(dp, d)
        dev.h2d(wp, w)
        De, Ne = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        for k, plan in enumerate((2, 1, 0)):
            dev.ltd_merge_dev(Dp, Np, n, [(dp, wp, idx)], 0 if k == 0 else n, etype=4, plan=plan)
            assert dev.last_merge_plan() == (plan or 1)          # three cells beside 2e9: the scatter form
            De, Ne = De + d[:3] * w[:3], Ne + w[:3]
            gd, gn = read(Dp), read(Np)
            assert (bits(gd[:3]) == bits(De)).all() and (bits(gn[:3]) == bits(Ne)).all(), plan
            assert (bits(gd[3:]) == 0).all() and (bits(gn[3:]) == 0).all(), plan
        dev.ltd_merge_close_dev(Dp, Np, n, etype=4)
        gd = read(Dp)
        assert (bits(gd[:3]) == bits(De / Ne)).all() and (gd[3:] == -1).all()
    finally:
        for p in ptrs:
            dev.free(p)


# ------------------------------------------------------------------ CLI
def cli_args(c, tmp):
    args = ["merge", "-i", os.path.join(MERGE, c["name"] + ".phy.gz")] + c["opts"]
    if c["weights"]:
        args += ["-w", os.path.join(MERGE, c["name"] + ".w.phy.gz")]
    for f in c["files"]:
        args += ["-" + f, os.path.join(tmp, f)]
    return args


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_cli_reproduces_golden_bytes(c, tmp_path):
    p = run(cli_args(c, str(tmp_path)))
    assert (p.returncode, p.stderr.decode()) == (c["rc"], c["stderr"])
    got = {"stdout": p.stdout}
    for f in c["files"]:
        if (tmp_path / f).exists():
            got[f] = (tmp_path / f).read_bytes()
    assert got == {k: (gz_read(v) if v else b"") for k, v in c["outputs"].items()}


def phy_text(names, cells, fmt="%.4f"):
    out = ["%10d\n" % len(names)]
    k = 0
    for i, nm in enumerate(names):
        out.append(nm + "".join("\t" + fmt % c for c in cells[k:k + i]) + "\n")
        k += i
    return "".join(out)


def random_file(sets, rng, lo=0.0, hi=50.0):
    return "".join(phy_text(s, rng.uniform(lo, hi, mo.tri(len(s)))) for s in sets)


@pytest.mark.parametrize("shape", ["first200", "names1500"])
@pytest.mark.parametrize("popt", [[], ["-p"]], ids=["f64", "f32"])
def test_cli_outside_the_reference_envelope(shape, popt, tmp_path):
    rng = np.random.default_rng(len(shape) + len(popt))
    names = ["smp%04d" % k for k in range(1500)]
    if shape == "first200":      # a first matrix of 200 entries, then new names: the reference writes past its matrices
        sets = [names[:200], list(rng.permutation(names[100:320])), names[310:330] + names[:5]]
    else:                        # 1500 names over 6 matrices: the reference's table registers names twice
        sets = [list(rng.permutation(names[250 * k:250 * k + 250] + names[:40 * k:7])) for k in range(6)]
    dtext, wtext = random_file(sets, rng), random_file(sets, rng, 1, 3000)
    (tmp_path / "d.phy").write_text(dtext)
    (tmp_path / "w.phy").write_text(wtext)
    et = 4 if popt else 8
    if shape == "first200":
        p = run(["merge", "-i", str(tmp_path / "d.phy")] + popt)
        rc, err, dt, _ = mo.run(dtext.encode(), None, et)
        assert (p.returncode, p.stderr) == (rc, err) and p.stdout == dt
    p = run(["merge", "-i", str(tmp_path / "d.phy"), "-w", str(tmp_path / "w.phy"), "-n", str(tmp_path / "n"),
             "-o", str(tmp_path / "o"), "-x", "12"] + popt)
    rc, err, dt, nt = mo.run(dtext.encode(), wtext.encode(), et, precision=12)
    assert (p.returncode, p.stderr, p.stdout) == (rc, err, b"")
    assert (tmp_path / "o").read_bytes() == dt and (tmp_path / "n").read_bytes() == nt
    assert dt.startswith(b"%10d\n" % len({s for t in sets for s in t}))


@pytest.mark.parametrize("method", ["dnj", "nj"])
@pytest.mark.parametrize("popt", [[], ["-p"]], ids=["f64", "f32"])
def test_cli_fused_tree_equals_the_pipeline(method, popt, tmp_path):
    rng = np.random.default_rng(11)
    names = ["t%03d" % k for k in range(90)]
    sets = [names[:50], list(rng.permutation(names[20:90])), list(rng.permutation(names))[:60], names[::-1]]
    (tmp_path / "d.phy").write_text(random_file(sets, rng, 1, 50))
    (tmp_path / "w.phy").write_text(random_file(sets, rng, 1, 3000))
    base = ["merge", "-i", str(tmp_path / "d.phy"), "-w", str(tmp_path / "w.phy")] + popt
    p = run(base + ["-o", str(tmp_path / "m.phy"), "-n", str(tmp_path / "n.phy")])
    assert p.returncode == 0, p.stderr
    t = run(["tree", "-i", str(tmp_path / "m.phy"), "-m", method] + popt)
    assert t.returncode == 0 and t.stdout.count(b";") == 1
    f = run(base + ["--tree", str(tmp_path / "t.nwk"), "--tree_method", method])
    assert (f.returncode, f.stdout) == (0, b""), f.stderr
    assert (tmp_path / "t.nwk").read_bytes() == t.stdout
    # with -o the text is written as well, the same bytes
    f = run(base + ["--tree", "-", "--tree_method", method, "-o", str(tmp_path / "m2.phy")])
    assert f.returncode == 0 and f.stdout == t.stdout
    assert (tmp_path / "m2.phy").read_bytes() == (tmp_path / "m.phy").read_bytes()


def test_cli_refusals(tmp_path):
    for o in (["-s"], ["-b", "10"], ["--short_precision"]):
        p = run(["merge", "-i", os.path.join(MERGE, "plain3.phy.gz")] + o)
        assert p.returncode == 1 and p.stdout == b"" and b"merge -s / -b is not supported" in p.stderr
    (tmp_path / "dup.phy").write_text(phy_text(["a", "b", "c"], [1, 2, 3]) + phy_text(["c", "q", "a", "q"], [1, 2, 3, 4, 5, 6]))
    p = run(["merge", "-i", str(tmp_path / "dup.phy")])
    assert p.returncode == 1 and p.stdout == b""
    assert b'matrix 2 holds the name "q" twice, on rows 2 and 4' in p.stderr
    p = run(["merge", "-i", os.path.join(MERGE, "plain3.phy.gz"), "--tree", "-", "--tree_method", "upgma"])
    assert p.returncode == 1 and b"--tree_method" in p.stderr


def test_cli_help_texts():
    h = run(["merge", "-h"])
    assert h.returncode == 0 and h.stdout.startswith(b"#CCPhylo merges matrices from a multi Phylip file into one matrix\n")
    assert h.stdout.count(b"\n") == 16 and b"nucleotides_weights" in h.stdout
    F = run(["merge", "-F"])
    assert F.returncode == 0 and F.stdout.startswith(b"# Format flags output, add them to combine them.\n#\n#   1:\tRelaxed Phylip\n")
