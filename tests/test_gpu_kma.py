"""GPU parity of count-matrix (KMA *.mat) distances, ccg_kma_ltd:
bit-exact against the reference's golden vectors and the oracle, through the
C-ABI and through the CLI.  l<n> / nl<n> go through pow(), which the GPU
math library does not round like glibc (parity of pow itself is unpinned):
l<n> compares within 1e-12 relative.  nl<n> raises the FIRST difference
without |.| (matcmp.c:113), so a position's sum can cancel to about +-1e-20,
where a one-ulp difference of pow decides between a cube root of ~1e-7 and
NaN (excluded): nl<n> compares within 1e-6 relative.

The multi-tile tests below run on adversarial file sets
(gen_golden.kma_adversarial) written once per module: 70 samples x 700 rows
are three tile rows (32 + 32 + 6) with diagonal and off-diagonal tiles, every
lane of the 2 x 2 register tile, 22 LDS chunks with a partial last one, and
pair bounds that differ inside a tile.  Their reference is the oracle
(pyoracle.kma_dist), itself pinned to the reference binary by the golden
kma_wrap_* / kma_zero_* cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden_bytes, golden_cases, parse_kma_args

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)


def _pow_metric(m):
    return m[0] == "l" and m[1:].isdigit() or m.startswith("nl") and m[2:].isdigit()


def _pow_rtol(m):
    return 1e-6 if m.startswith("nl") else 1e-12


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def _phylip_values(text):
    vals = []
    for line in text.decode().splitlines()[1:]:
        vals += [float(v) for v in line.split("\t")[1:]]
    return np.array(vals)


@pytest.mark.parametrize("case", golden_cases("kma"), ids=lambda c: c["name"])
def test_kma_golden_engine(dev, case):
    import ccphylo_amd as cg
    from test_oracle_golden import kma_phylip
    o = parse_kma_args(case["args"])
    K = cg.native.load_kma(o["files"], o["tmpl"], min_depth=o["minDepth"], min_length=o["minLength"],
                           min_cov=o["minCov"])
    D, N, fatal = dev.kma_ltd(K, metric=o["metric"], norm=o["norm"], min_depth=o["minDepth"],
                              min_length=o["minLength"], min_cov=o["minCov"], etype=o["et"], byte_scale=o["bs"],
                              want_n=o["nout"])
    assert fatal == -1
    got = kma_phylip(o, D, N, K["include"], K["n"])
    if _pow_metric(o["metric"]):
        np.testing.assert_allclose(_phylip_values(got), _phylip_values(golden_bytes(case)),
                                   rtol=_pow_rtol(o["metric"]))
    else:
        assert got == golden_bytes(case)


@pytest.mark.parametrize("case", golden_cases("kma"), ids=lambda c: c["name"])
def test_kma_golden_cli(case):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH] + case["args"], cwd=GOLDEN, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    m = parse_kma_args(case["args"])["metric"]
    if _pow_metric(m):
        np.testing.assert_allclose(_phylip_values(p.stdout), _phylip_values(golden_bytes(case)), rtol=_pow_rtol(m))
    else:
        assert p.stdout == golden_bytes(case)


@pytest.mark.parametrize("nsamp,L,metric,et", [(41, 20000, "cos", 8), (37, 9000, "c", 4), (70, 4000, "nbc", 8),
                                               (33, 6000, "chi2", 2), (35, 5000, "nchi2", 8), (40, 5000, "l2", 8)])
def test_kma_random_vs_oracle(dev, tmp_path, nsamp, L, metric, et):
    """More samples than one 32 x 32 tile, insertion rows, low-depth rows."""
    import random
    import ccphylo_amd as cg
    from gen_golden import kma_sample
    from oracle import pyoracle
    rng = random.Random(nsamp * L)
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    files = []
    for k in range(nsamp):
        f = str(tmp_path / f"r{k}.mat.gz")
        kma_sample(f, [("x", ref)], seed=1000 + k, depth=20 if k % 5 else 12, ins=0.003 if k % 7 == 3 else 0.0)
        files.append(f)
    bs = 10.0 if et <= 2 else 1.0
    D0, N0, inc, n = pyoracle.kma_dist(files, "x", metric=metric, etype=et, byte_scale=bs, want_n=True)
    K = cg.native.load_kma(files, "x")
    D, N, fatal = dev.kma_ltd(K, metric=metric, etype=et, byte_scale=bs, want_n=True)
    assert fatal == -1 and K["n"] == n and (K["include"] == inc).all()
    assert np.array_equal(D, D0) and np.array_equal(N, N0)


def test_kma_fatal_pair(dev, tmp_path):
    """A later sample whose rows with ref != '-' fail the thresholds that its
    rows with '-' passed: the reference exits(1) at the first such pair."""
    import ccphylo_amd as cg
    from gen_golden import kma_sample
    ref = "ACGT" * 200
    files = []
    for k in range(4):
        f = str(tmp_path / f"f{k}.mat.gz")
        kma_sample(f, [("x", ref)], seed=k, depth=30, ins=0.0)
        files.append(f)
    # sample 1: shallow rows + deep insertion rows (counted by FileBuffLoadMat's nNucs only)
    with open(str(tmp_path / "f1.mat"), "w") as fh:
        fh.write("#x\n")
        for b in ref:
            fh.write(b + "\t1\t0\t0\t0\t0\t0\n-\t40\t0\t0\t0\t0\t0\n")
        fh.write("\n")
    files[1] = str(tmp_path / "f1.mat")
    K = cg.native.load_kma(files, "x")
    _, _, fatal = dev.kma_ltd(K)
    assert fatal >= 0
    p = subprocess.run([cg.CLI_PATH, "dist", "-i"] + files + ["-r", "x"], capture_output=True, timeout=120)
    assert p.returncode == 1 and p.stdout == b""
    assert b"did not exceed threshold" in p.stderr


# ---------------------------------------------------------------- adversarial
ADV_N, ADV_L = 70, 700
ADV_DEPTH = {"wrap": 15, "zero": 0, "plain": 15}   # profile -> min_depth (-E)
ADV_METRICS = ["cos", "c", "l1", "l2", "linf", "chi2", "nchi2", "nc", "bc", "nbc", "nl1", "nl2", "nlinf", "l3",
               "nl3"]


def _write_set(root, profile, n, L, seed, tag=None):
    from gen_golden import kma_adversarial
    files = []
    for k in range(n):
        f = str(root / (f"{tag or profile}{k}.mat" + (".gz" if k % 2 else "")))
        kma_adversarial(f, L, seed=seed, profile=profile, k=k, gz=bool(k % 2))
        files.append(f)
    return files


class _Adv:
    """The module's file sets, their loader views and the oracle's matrices,
    each made once and handed out read-only."""

    def __init__(self, root):
        self.root = root
        self.files = {p: _write_set(root, p, ADV_N, ADV_L, seed=30) for p in ADV_DEPTH}
        self.files["edge"] = _write_set(root, "wrap", 65, 100, seed=31, tag="edge")
        self._K, self._O = {}, {}

    def K(self, profile):
        import ccphylo_amd as cg
        if profile not in self._K:
            self._K[profile] = cg.native.load_kma(self.files[profile], "x", min_depth=ADV_DEPTH[profile])
        return self._K[profile]

    def oracle(self, profile, metric, et=8, **kw):
        from oracle import pyoracle
        key = (profile, metric, et, tuple(sorted(kw.items())))
        if key not in self._O:
            kw.setdefault("min_depth", ADV_DEPTH[profile])
            D, N, inc, n = pyoracle.kma_dist(self.files[profile], "x", metric=metric, etype=et,
                                             byte_scale=10.0 if et <= 2 else 1.0, want_n=True, **kw)
            assert n == len(self.files[profile]) and inc.all()
            D.flags.writeable = N.flags.writeable = False
            self._O[key] = (D, N)
        return self._O[key]


@pytest.fixture(scope="module")
def adv(tmp_path_factory):
    return _Adv(tmp_path_factory.mktemp("kma_adv"))


def _bad_share(D):
    """Share of the cells of a double matrix that are negative or not finite."""
    return float((~np.isfinite(D) | (D < 0)).mean())


@pytest.mark.parametrize("et", [8, 4, 2, 1])
@pytest.mark.parametrize("profile,metric", [(p, m) for p in ADV_DEPTH for m in ADV_METRICS
                                            if m != "nl3" or p == "plain"])
def test_kma_all_metrics_multi_tile(dev, adv, profile, metric, et):
    """Every metric x element type on the three profiles, D and N.  u16 / u8
    run with byte_scale 10, so inf, -1 and values beyond the type's range go
    through the integer store.  nl3 runs on "plain" only; its N is not
    asserted (module docstring) but counted and printed."""
    # the inputs do what they are here for (on the oracle's double matrices)
    D8, N8 = adv.oracle(profile, metric)
    assert not np.isnan(D8).any()
    assert _bad_share(D8) <= 1 / 3
    if profile in ("wrap", "plain"):
        assert ((D8 == -1) & (N8 > 0)).any()      # cmpMats' early -1: N keeps a row total
    if profile == "zero" and metric == "nlinf":
        assert np.isinf(D8).any()
    if profile == "wrap" and metric == "cos":
        assert (N8 != adv.oracle("wrap", "l1")[1]).any()   # positions dropped by the signed norm
    K = adv.K(profile)
    D0, N0 = adv.oracle(profile, metric, et)
    D, N, fatal = dev.kma_ltd(K, metric=metric, min_depth=ADV_DEPTH[profile], etype=et,
                              byte_scale=10.0 if et <= 2 else 1.0, want_n=True)
    assert fatal == -1 and K["n"] == ADV_N
    if not _pow_metric(metric):
        assert D.tobytes() == D0.tobytes() and N.tobytes() == N0.tobytes()
    elif metric == "l3":
        np.testing.assert_allclose(D, D0, rtol=1e-12, atol=0)
        assert N.tobytes() == N0.tobytes()
    else:
        print(f"nl3 plain etype {et}: {int((N != N0).sum())} of {N.size} N cells differ")
        np.testing.assert_allclose(D, D0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("et", [8, 2])
@pytest.mark.parametrize("metric", ["cos", "nbc"])
def test_kma_thresholds_multi_tile(dev, adv, metric, et):
    """-W 1000 with -E, -L and -C raised together on "plain": at depth 18 a
    pair keeps 226 .. 421 of its 700 positions (median 368), every sample
    still passes on its own, and the included-row rule (rowsInc < minLength
    || rowsInc < minCov * len, matcmp.c:486) at 0.52 * 700 = 364 rows turns
    about a quarter of the pairs to -1 and leaves the others."""
    import ccphylo_amd as cg
    th = dict(min_depth=18, min_length=350, min_cov=0.52)
    D0, N0 = adv.oracle("plain", metric, et, norm=1000, **th)
    D8, N8 = adv.oracle("plain", metric, 8, norm=1000, **th)
    assert ((D8 == -1) & (N8 == 0)).any() and (D8 >= 0).any()
    K = cg.native.load_kma(adv.files["plain"], "x", **th)
    D, N, fatal = dev.kma_ltd(K, metric=metric, norm=1000, etype=et, byte_scale=10.0 if et <= 2 else 1.0,
                              want_n=True, **th)
    assert fatal == -1 and K["n"] == ADV_N
    assert D.tobytes() == D0.tobytes() and N.tobytes() == N0.tobytes()


def test_kma_fatal_index(dev, adv):
    """Two fatal column samples (5 and 40) among 70: candidates for the first
    fatal pair lie in several tiles, and the engine reports the smallest flat
    index i(i-1)/2 + j among them, (6, 5) = 20 -- where the reference, filling
    row by row, exits."""
    import ccphylo_amd as cg
    from oracle import pyoracle
    bad = str(adv.root / "fatal.mat")
    with open(bad, "w") as fh:   # test_kma_fatal_pair's sample: shallow rows + deep insertion rows
        fh.write("#x\n")
        for b in ("ACGT" * ADV_L)[:ADV_L]:
            fh.write(b + "\t1\t0\t0\t0\t0\t0\n-\t40\t0\t0\t0\t0\t0\n")
        fh.write("\n")
    files = list(adv.files["plain"])
    files[5] = files[40] = bad
    with pytest.raises(RuntimeError):
        pyoracle.kma_dist(files, "x")
    K = cg.native.load_kma(files, "x")
    assert K["n"] == ADV_N
    _, _, fatal = dev.kma_ltd(K)
    assert fatal == 20
    p = subprocess.run([cg.CLI_PATH, "dist", "-i"] + files + ["-r", "x"], capture_output=True, timeout=120)
    assert p.returncode == 1 and p.stdout == b""


@pytest.mark.parametrize("metric", ["cos", "nchi2"])
@pytest.mark.parametrize("n", [2, 3, 32, 33, 64, 65])
def test_kma_tile_edges(dev, adv, n, metric):
    """Sample counts at and around the 32-sample tile side."""
    import ccphylo_amd as cg
    from oracle import pyoracle
    files = adv.files["edge"][:n]
    D0, N0, inc, n0 = pyoracle.kma_dist(files, "x", metric=metric, want_n=True)
    K = cg.native.load_kma(files, "x")
    D, N, fatal = dev.kma_ltd(K, metric=metric, want_n=True)
    assert fatal == -1 and K["n"] == n0 == n and D.size == n * (n - 1) // 2
    assert D.tobytes() == D0.tobytes() and N.tobytes() == N0.tobytes()


def test_kma_single_sample(dev, adv):
    import ccphylo_amd as cg
    K = cg.native.load_kma(adv.files["edge"][:1], "x")
    D, N, fatal = dev.kma_ltd(K, want_n=True)
    assert K["n"] == 1 and D.size == 0 and N.size == 0 and fatal == -1


@pytest.mark.parametrize("et", [8, 1])
@pytest.mark.parametrize("metric", ["cos", "bc"])
def test_kma_dev_entry_equals_host_entry(dev, adv, metric, et):
    """ccg_kma_ltd_dev (what bench.py's kma extra times) on device copies of
    the loader's views gives ccg_kma_ltd's bytes, with and without N."""
    import torch
    K = adv.K("wrap")
    n, m = K["n"], K["n"] * (K["n"] - 1) // 2
    bs = 10.0 if et <= 2 else 1.0
    assert K["stride1"] != K["stride2"]
    D0, N0, fatal0 = dev.kma_ltd(K, metric=metric, etype=et, byte_scale=bs, want_n=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    rec1, rec2, len1, len2 = up(K["rec1"]), up(K["rec2"]), up(K["len1"]), up(K["len2"])
    for want_n in (True, False):
        Dd = torch.zeros(m * et, dtype=torch.uint8, device="cuda:0")
        Nd = torch.zeros(m * et, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        fatal = dev.kma_ltd_dev(n, rec1.data_ptr(), len1.data_ptr(), K["stride1"], rec2.data_ptr(), len2.data_ptr(),
                                K["stride2"], Dd.data_ptr(), Nd.data_ptr() if want_n else None, metric=metric,
                                etype=et, byte_scale=bs)
        assert fatal == fatal0 == -1
        assert Dd.cpu().numpy().tobytes() == D0.tobytes()
        assert Nd.cpu().numpy().tobytes() == (N0.tobytes() if want_n else bytes(m * et))
