"""GPU: `ccphylo tsv2phy` on the gfx950 engine (ccg_vec_ltd / ccg_vec_ltd_dev,
the CLI subcommand and the fused `tsv2phy --tree`).

Every cell is the reference's serial chain over the columns, so the engine's
LT must equal the restatement's (tests/tsv_oracle.py, itself pinned to the
reference's bytes by test_tsv_oracle.py) BITWISE for cos, chi2, bc, l1, l2,
linf and p, for double and float rows; the CLI's bytes must equal the
reference's (tests/golden/tsv).  l<n> goes through pow(): rtol 1e-12, the
project's rule for pow metrics (tests/test_gpu_kma.py: positive terms, one
closing pow).

The pair kernel tiles the pairs in blocks of T x T (VEC_T_SMALL = 32 up to 3072
rows, VEC_T_BIG = 64 above; CCG_VEC_TILE forces one) and walks the columns in
LDS chunks of K = VEC_K = 32 (ccphylo_amd/csrc/vec.hip).  Sizes per form:
m in {2, 3, T-1, T, T+1, 2T + T/2 + 1} (diagonal, off-diagonal and partial
tiles, every lane of the register tile), n in {1, 2, K-1, K, K+1, 2K+3}."""
import os
import subprocess

import numpy as np
import pytest

import tsv_oracle as tso
from tsv_oracle import CASES, PHY, TSV, case_bytes, case_options

pytestmark = pytest.mark.gpu

TILES = (32, 64)
K = 32
NS = (1, 2, K - 1, K, K + 1, 2 * K + 3)
SIGNED = ("l1", "l2", "linf", "cos", "p")
TREES = [c for c in CASES if "tree" in c]


def ms_of(T):
    return (2, 3, T - 1, T, T + 1, 2 * T + T // 2 + 1)


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


@pytest.fixture
def tile(request):
    """Forces the tile form of the parametrised T for one test."""
    old = os.environ.get("CCG_VEC_TILE")
    os.environ["CCG_VEC_TILE"] = str(request.param)
    yield request.param
    if old is None:
        del os.environ["CCG_VEC_TILE"]
    else:
        os.environ["CCG_VEC_TILE"] = old


def cli(args, cwd=TSV, ok=True):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH] + args, cwd=cwd, capture_output=True, timeout=300)
    if ok:
        assert p.returncode == 0, (args, p.stderr.decode()[-2000:])
    return p


_TABLES = {}


def table(m, n, signed):
    """Three decimals per entry (float rows differ from double rows); from 3
    rows up the last row repeats row 0 and row 1 is all zero."""
    key = (m, n, signed)
    if key not in _TABLES:
        rng = np.random.default_rng(1000 * m + 10 * n + signed)
        X = np.round(rng.uniform(-5, 5, (m, n)) if signed else rng.uniform(0, 10, (m, n)), 3)
        if m >= 3:
            X[m - 1] = X[0]
            X[1] = 0
        X.setflags(write=False)
        _TABLES[key] = X
    return _TABLES[key]


_ORACLE = {}


def oracle(m, n, metric, vtype):
    key = (m, n, metric, vtype)
    if key not in _ORACLE:
        X = table(m, n, metric in SIGNED)
        kind, ex = tso.parse_metric(metric)
        r = tso.vec_ltd(X.astype(np.float32) if vtype == 4 else X, kind, ex)
        # the one non-finite case of these tables: p on float rows with n = 1, where the float square minus the
        # double one leaves a negative "variance" (the reference prints -nan there)
        assert np.isfinite(r).all() or (metric == "p" and vtype == 4 and n == 1 and not np.isinf(r).any())
        r.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def same_bits(a, b):
    """Bitwise equal; a NaN matches a NaN of either sign (the sign of a generated NaN is not pinned)."""
    nan = np.isnan(b)
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(bits)[~nan], b.view(bits)[~nan])


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("case", PHY, ids=[c["name"] for c in PHY])
def test_cli_golden(case):
    out = cli(list(case["args"])).stdout
    ref = case_bytes(case)
    if tso.parse_metric(case_options(case["args"])["d"])[0] != "ln":
        assert out == ref
        return
    (m, a), (rm, b) = tso.parse_phy(out), tso.parse_phy(ref)
    assert m == rm
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", PHY, ids=[c["name"] for c in PHY])
def test_engine_golden(dev, case):
    import ccphylo_amd as cg
    o = case_options(case["args"])
    X = cg.load_tsv(os.path.join(TSV, o["inp"]), o["sep"], o["vtype"])
    D = dev.vec_ltd(X, o["d"])
    ref = case_bytes(case)
    if tso.parse_metric(o["d"])[0] == "ln":
        np.testing.assert_allclose(D, tso.parse_phy(ref)[1], rtol=1e-12, atol=0)
    else:
        assert tso.format_phy(D, X.shape[0], o["flag"], o["prec"]) == ref


# ------------------------------------------------------------ random tables
@pytest.mark.parametrize("vtype", [8, 4])
@pytest.mark.parametrize("metric", tso.METRICS)
@pytest.mark.parametrize("tile", TILES, indirect=True)
def test_random_tables_bitwise(dev, tile, metric, vtype):
    for m in ms_of(tile):
        for n in NS:
            X = table(m, n, metric in SIGNED)
            if vtype == 4:
                X = X.astype(np.float32)
            ref = oracle(m, n, metric, vtype)
            D = dev.vec_ltd(X, metric)
            assert dev.last_vec_plan() == (tile, K)
            assert same_bits(D, ref), (tile, metric, vtype, m, n, int((D != ref).sum()))
            D4 = dev.vec_ltd(X, metric, etype=4)
            assert D4.dtype == np.float32 and same_bits(D4, ref.astype(np.float32)), (tile, metric, vtype, m, n)


@pytest.mark.parametrize("vtype", [8, 4])
@pytest.mark.parametrize("metric", ["l3", "l2.5"])
@pytest.mark.parametrize("tile", TILES, indirect=True)
def test_random_tables_pow(dev, tile, metric, vtype):
    for m in (3, tile + 1, 2 * tile + tile // 2 + 1):
        for n in (1, K - 1, 2 * K + 3):
            X = table(m, n, metric in SIGNED)
            if vtype == 4:
                X = X.astype(np.float32)
            D = dev.vec_ltd(X, metric)
            np.testing.assert_allclose(D, oracle(m, n, metric, vtype), rtol=1e-12, atol=0)


def test_default_form_follows_the_table_size(dev):
    """Up to 3072 rows the small tile (every CU has work from about 1000 rows up), above it the large one."""
    assert "CCG_VEC_TILE" not in os.environ
    for m, want in ((3072, 32), (3073, 64)):
        X = table(m, 2, True)
        D = dev.vec_ltd(X, "l1")
        assert dev.last_vec_plan() == (want, K)
        i, j = np.tril_indices(m, -1)
        ref = np.abs(X[i, 0] - X[j, 0]) + np.abs(X[i, 1] - X[j, 1])   # two columns: one sum, no order to keep
        assert same_bits(D, ref)
    assert dev.vec_ltd(table(1, 5, True), "cos").size == 0 and dev.last_vec_plan() == (0, 0)
    assert dev.last_vec_ms() == 0


# ------------------------------------------------------------ further cases
def test_host_and_device_calls_agree_and_stride(dev):
    m, n, stride = 81, 35, 41
    X = table(m, n, True)
    wide = np.full((m, stride), 777.0)
    wide[:, :n] = X
    for metric in ("cos", "p", "linf"):
        ref = dev.vec_ltd(X, metric)
        assert same_bits(ref, oracle(m, n, metric, 8))
        assert dev.last_vec_ms() > 0
        assert same_bits(dev.vec_ltd(wide[:, :n], metric), ref)   # a host view with a row stride of 41
        dX, dD = dev.malloc(wide.nbytes), dev.malloc(ref.nbytes)
        try:
            dev.h2d(dX, wide)
            dev.vec_ltd_dev(dX, m, n, dD, stride=stride, metric=metric)
            assert dev.last_vec_ms() > 0
            got = np.zeros_like(ref)
            dev.d2h(got, dD)
        finally:
            dev.free(dX)
            dev.free(dD)
        assert same_bits(got, ref)


def test_invalid_arguments(dev):
    import ccphylo_amd as cg
    X = table(5, 4, True)
    with pytest.raises(cg.CcgError):
        dev.vec_ltd(X, 9)                      # unknown metric id
    with pytest.raises(cg.CcgError):
        dev.vec_ltd(X, "cos", etype=2)         # CCG_EUNSUP
    with pytest.raises(cg.CcgError):
        dev.vec_ltd(np.zeros((5, 0)), "cos")   # n < 1
    with pytest.raises(cg.CcgError):
        dev.vec_ltd(X, cg.CCG_VEC_LN)          # exponent 0
    with pytest.raises(ValueError):
        cg.vec_metric("l0")
    assert cg.vec_metric("l2.5") == (cg.CCG_VEC_LN, 2.5) and cg.vec_metric("p") == (cg.CCG_VEC_PEARSON, 0.0)


@pytest.mark.parametrize("case", TREES, ids=[c["name"] for c in TREES])
def test_fused_tree(case, tmp_path):
    """tsv2phy --tree == tsv2phy -x 17 -o P, then tree -i P == the reference's `tsv2phy -x 17 | tree`."""
    o = case_options(case["args"])
    opts = ["-i", o["inp"], "-d", o["d"]] + (["-p"] if o["vtype"] == 4 else [])
    nwk, phy, two = tmp_path / "t.nwk", tmp_path / "p.phy", tmp_path / "two.nwk"
    assert cli(["tsv2phy"] + opts + ["--tree", str(nwk), "--tree_method", case["tree"]]).stdout == b""
    assert cli(["tsv2phy"] + opts + ["-x", "17", "-o", str(phy)]).stdout == b""
    cli(["tree", "-i", str(phy), "-m", case["tree"], "-o", str(two)])
    assert nwk.read_bytes() == two.read_bytes() == case_bytes(case)


def test_fused_tree_with_output_and_f0(tmp_path):
    """-o beside --tree writes the Phylip text too; -f 0 pads the names in the text, not in the tree."""
    nwk, phy = tmp_path / "t.nwk", tmp_path / "p.phy"
    cli(["tsv2phy", "-i", "tree30.tsv", "-f", "0", "-x", "17", "--tree", str(nwk), "-o", str(phy)])
    assert phy.read_bytes() == cli(["tsv2phy", "-i", "tree30.tsv", "-f", "0", "-x", "17"]).stdout
    two = cli(["tree", "-i", str(phy), "-x", "17"]).stdout
    assert nwk.read_bytes() == two
    p = cli(["tsv2phy", "-i", "two.tsv", "--tree", str(nwk)], ok=False)
    assert p.returncode != 0 and b"at least 3 rows" in p.stderr


def test_cli_long_forms(tmp_path):
    ref = cli(["tsv2phy", "-i", "pos12.tsv", "-d", "bc", "-x", "12", "-p"]).stdout
    out = tmp_path / "o.phy"
    assert cli(["tsv2phy", "--input", "pos12.tsv", "--distance=bc", "--print_precision", "12", "--float_precision",
                "-H", "-T", str(tmp_path), "--output", str(out)]).stdout == b""
    assert out.read_bytes() == ref
    with open(os.path.join(TSV, "pos12.tsv"), "rb") as f:
        p = subprocess.run([__import__("ccphylo_amd").CLI_PATH, "tsv2phy", "-d", "bc", "-x12", "-p"], stdin=f,
                           capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout == ref


@pytest.mark.parametrize("opts", [["-s"], ["-b"], ["-d", "nope"], ["-d", "l0"], ["-d", "lx"]], ids="_".join)
def test_cli_refusals(opts):
    p = cli(["tsv2phy", "-i", "mix12.tsv"] + opts, ok=False)
    assert p.returncode != 0 and p.stdout == b""
    if opts[0] != "-d":
        assert b"not supported" in p.stderr
    elif opts[1] == "nope":
        assert p.stderr == b"Invalid value parsed at \"--distance\".\n"
    elif opts[1] == "lx":
        assert p.stderr == b"Invalid value parsed at \"--distance ln\".\n"
