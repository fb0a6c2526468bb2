"""CPU: the host layer of `nwck2phy` / `phycmp` -- ccq_newick_splits against
the literal restatement (tests/fit_oracle.py), its refusals, ccq_cmp_metric
against the reference's printed lines, and the exported symbols."""
import ctypes as C
import json
import os
import subprocess
import time

import numpy as np
import pytest

import fit_oracle as fo
from conftest import GOLDEN

FIT = os.path.join(GOLDEN, "fit")
with open(os.path.join(FIT, "fit.json")) as f:
    CASES = json.load(f)["cases"]


def both(line):
    """(restatement, host) results of one line, an exception as ('invalid' | 'refused', text)"""
    from ccphylo_amd import native
    try:
        h, names, sp = fo.parse_line(line)
        py = (h, names, [(o, float(a), float(b)) for o, a, b in sp])
    except fo.InvalidLimb as e:
        py = ("invalid", "Invalid limb length at node:\t" + e.args[0])
    except fo.Refused:
        py = ("refused",)
    try:
        h, names, sp = native.newick_splits(line)
        c = (h, names, [(int(o), float(a), float(b)) for o, a, b in sp])
    except native.CcgError as e:
        c = ("invalid", str(e)) if e.code == 1 else ("refused",)
        assert e.code in (1, -1)
    return py, c


def lines_of(path):
    with open(path, "rb") as f:
        data = f.read()
    pos = 0
    while True:
        p = data.find(b"(", pos)
        e = data.find(b"\n", p) if p >= 0 else -1
        if e < 0:
            return
        yield data[pos:e]
        pos = e + 1


def test_every_golden_line():
    inputs = sorted({c["args"][2] for c in CASES if c["cmd"] == "nwck2phy"})
    inputs += sorted(f for f in os.listdir(GOLDEN) if f.endswith(".out") and f not in inputs
                     and open(os.path.join(GOLDEN, f), "rb").read(1) in (b"(", b">"))
    seen = 0
    for inp in inputs:
        for line in lines_of(os.path.join(GOLDEN, inp)):
            py, c = both(line)
            assert py == c, inp
            seen += 1
    assert seen >= 20


def fmt_limb(rng):
    k = rng.integers(0, 8)
    if k == 0:
        return ""
    if k == 1:
        return ":%d" % rng.integers(0, 10)            # one digit: not found in a node kept one byte short
    if k == 2:
        return ":-%.9f" % rng.random()
    if k == 3:
        return ":0.000000000"
    return ":%.9f" % (rng.random() * 10)


def random_tree(rng, leaves, multi):
    """a Newick line of `leaves` leaves: binary, or with nodes of up to 5 children"""
    nodes = ["t%d%s" % (i, "x" * int(rng.integers(0, 3))) for i in range(leaves)]
    while len(nodes) > (1 if not multi else min(len(nodes), int(rng.integers(1, 4)))):
        k = min(len(nodes), 2 if not multi else int(rng.integers(2, 6)))
        idx = sorted(rng.choice(len(nodes), k, replace=False), reverse=True)
        kids = [nodes.pop(i) for i in idx]
        nodes.append("(" + ",".join(c + fmt_limb(rng) for c in kids) + ")")
        if len(nodes) == 1:
            break
    if len(nodes) > 1:
        return "(" + ",".join(c + fmt_limb(rng) for c in nodes) + ");"
    return nodes[0] + ";"


def test_random_trees():
    rng = np.random.default_rng(11)
    kinds = {"ok": 0, "invalid": 0, "refused": 0}
    sizes = [2, 3, 4, 5, 7, 16, 33, 64, 100, 200, 300] + [int(x) for x in rng.integers(2, 301, 60)]
    for leaves in sizes:
        for multi in (False, True):
            line = random_tree(rng, leaves, multi).encode()
            py, c = both(line)
            assert py == c, line
            kinds[py[0] if isinstance(py[0], str) else "ok"] += 1
    assert all(kinds.values()), kinds


def test_well_formed_trees_parse():
    """every child with a limb of 9 decimals, as `tree` writes it: no refusal"""
    rng = np.random.default_rng(12)
    for leaves in (3, 10, 150, 300):
        nodes = ["n%d" % i for i in range(leaves)]
        while len(nodes) > 3:
            a, b = sorted(rng.choice(len(nodes), 2, replace=False), reverse=True)
            x, y = nodes.pop(a), nodes.pop(b)
            nodes.append("(%s:%.9f,%s:%.9f)" % (x, rng.random(), y, rng.random()))
        line = ("(" + ",".join("%s:%.9f" % (c, rng.random()) for c in nodes) + ");").encode()
        py, c = both(line)
        assert py == c and len(c) == 3 and len(c[1]) == leaves
        assert sorted(c[1]) == sorted(b"n%d" % i for i in range(leaves))


def caterpillar(n, left=True):
    s = "c0:1.000000000"
    for i in range(1, n - 1):
        s = ("(%s,c%d:%.9f):0.500000000" if left else "(c%d:%.9f,%s):0.500000000") % \
            ((s, i, 1 + i / 7) if left else (i, 1 + i / 7, s))
    return ("(%s,c%d:2.000000000);" % (s, n - 1)).encode()


def test_caterpillar_3000():
    from ccphylo_amd import native
    for left in (True, False):
        line = caterpillar(3000, left)
        py, c = both(line)
        assert py == c and len(c[1]) == 3000
    # one pass over the text: 30 000 leaves (1 MB) take milliseconds; a walk of the
    # remaining text per split, 3e10 byte steps, would take far longer than the bound
    line = caterpillar(30000)
    t0 = time.perf_counter()
    _, names, sp = native.newick_splits(line)
    dt = time.perf_counter() - t0
    assert len(names) == 30000 and dt < 2.0, dt


@pytest.mark.parametrize("line,node", [(b"(A:1,BB);", "BB"), (b"(A,B);", "A"), (b"(s1,s2);", "s2"),
                                       (b"((a:1.5,b:2.5):1.0,(c1,d1):2.0,e:1.25);", "d1")])
def test_refuses_where_the_reference_is_undefined(line, node):
    from ccphylo_amd import native
    with pytest.raises(fo.Refused):
        fo.parse_line(line)
    with pytest.raises(native.CcgError) as e:
        native.newick_splits(line)
    assert e.value.code == -1
    assert str(e.value).endswith("at node:\t" + node)


def test_invalid_limb_message_is_the_references():
    from ccphylo_amd import native
    case, = [c for c in CASES if c["name"] == "miss80_nj"]
    line, = lines_of(os.path.join(GOLDEN, "miss80_nj.out"))
    with pytest.raises(native.CcgError) as e:
        native.newick_splits(line)
    assert e.value.code == 1 and str(e.value) + "\n" == case["stderr"]


def test_other_refusals():
    from ccphylo_amd import native
    for line in (b"no tree here", b"()", b"(A:1.0,B:2.0", b"(a(b,c)d:1.5,e:2.5);"):
        with pytest.raises(native.CcgError) as e:
            native.newick_splits(line)
        assert e.value.code == -1, line
        with pytest.raises(fo.Refused):
            fo.parse_line(line)


def test_malformed_lines_agree():
    """unbalanced and empty nodes: whatever the literal walk does, the tables do"""
    for line in (b"(,)", b"(,,,)", b"((((x)", b"(a))b(c,d)", b"(a,b))c,d)", b"x(a:1.5,(b:2.5)", b"(:,:)", b"(a:,b:)",
                 b"((a,b),(c,d))", b"(a)(b)", b"(A)b)c(d,e)", b"((a:1.25,b:2.5)", b"(a:1.25,b:2.5))", b"(a:1.5,b:2.5)x)",
                 b"((aa:1.25,bb:2.5):1.0,((cc:1.0,dd:2.0):1.5,(ee:1.0,ff:2.0):1.5))", b"(a b:1.5,'c,d':2.5,e:3.5)"):
        py, c = both(line)
        assert py == c, line


def test_cmp_metric_closes_to_the_references_lines():
    from ccphylo_amd import native
    done = 0
    for case in CASES:
        if case["cmd"] != "phycmp" or case["rc"]:
            continue
        (n1, A), (n2, B) = [m for f in case["files"] for m in native.load_phylip(os.path.join(GOLDEN, f),
                                                                                 etype=case["etype"])]
        n = len(n1)
        cells = n * (n - 1) // 2
        s, _ = fo.cmp_sums(A, B, case["etype"])
        _, met = native.cmp_close(s, cells)
        lines = "".join("%s:\t%s\n" % (k, "-nan" if np.isnan(met[k]) and np.signbit(met[k]) else "%f" % met[k])
                        for k in native.CMP_METRICS)
        assert lines == case["stdout"], case["name"]
        for k in native.CMP_METRICS:
            want = fo.metric(s, cells, k)
            assert met[k] == want or (np.isnan(met[k]) and np.isnan(want)), (case["name"], k)
        done += 1
    assert done == 10


def test_print_phycmp_writes_the_flagged_lines(tmp_path):
    from ccphylo_amd import native
    lib = native.host_lib()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    s = native.CmpSums(*[float(k + 1) for k in range(11)])
    for flag in (1, 127, 2 | 16, 64):
        p = str(tmp_path / ("f%d" % flag))
        fh = libc.fopen(p.encode(), b"wb")
        lib.ccq_print_phycmp(fh, C.byref(s), 10, flag)
        libc.fclose(fh)
        _, met = native.cmp_close(s, 10)
        want = "".join("%s:\t%f\n" % (k, met[k]) for b, k in enumerate(native.CMP_METRICS) if flag & (1 << b))
        assert open(p).read() == want


def test_symbols_exported():
    from ccphylo_amd import native
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"ccg_nwck_ltd", "ccg_nwck_ltd_dev", "ccg_ltd_cmp", "ccg_ltd_cmp_dev", "ccg_last_nwck",
            "ccg_last_cmp_ms"} <= exported(native.ENGINE_PATH)
    assert {"ccq_newick_splits", "ccq_newick_splits_free", "ccq_read_nwck", "ccq_cmp_metric",
            "ccq_print_phycmp"} <= exported(native.HOST_PATH)
    assert native.SPLIT_DTYPE.itemsize == 24 and native.SPLIT_DTYPE.fields["Li"][1] == 8
    assert C.sizeof(native.CmpSums) == 88


def test_cli_without_a_gpu_paths():
    """what the command line decides before it opens a GPU: help bytes, refusals, the three validation errors"""
    from ccphylo_amd import native
    def run(*a):
        return subprocess.run([native.CLI_PATH] + list(a), cwd=GOLDEN, capture_output=True, timeout=60)
    for cmd in ("nwck2phy", "phycmp"):
        for o in ("-s", "-b"):
            p = run(cmd, o, "-i", "fit/star.nwk")
            assert p.returncode == 1 and b"not implemented" in p.stderr and p.stdout == b""
        assert run(cmd, "-h").returncode == 0 and run(cmd, "-h").stdout.startswith(b"#")
    assert run("nwck2phy", "-F").stdout == b"Format flags output format, add them to combine them.\n#\n# 1:\tRelaxed Phylip\n#\n"
    for case in CASES:
        if case["cmd"] == "phycmp" and case["rc"]:
            p = run(*case["args"])
            assert (p.returncode, p.stdout.decode(), p.stderr.decode()) == (case["rc"], "", case["stderr"]), case["name"]
    p = run("phycmp", "--by_name", "-i", "miss80.phy", "test.phy.gz")
    assert p.returncode == 1 and p.stderr == b"Matrices differ in size.\n"
    p = run("tree", "-i", "test.phy.gz", "--phycmp", os.devnull, "--gpus", "2")
    assert p.returncode == 1 and b"not implemented" in p.stderr
    p = run("frobnicate")
    assert p.returncode == 1 and b"nwck2phy, phycmp" in p.stderr
    # a refused line and the reference's own exit, both before any GPU work (no matrix precedes them)
    p = run("nwck2phy", "-i", "miss80_nj.out")
    case, = [c for c in CASES if c["name"] == "miss80_nj"]
    assert (p.returncode, p.stdout, p.stderr.decode()) == (1, b"", case["stderr"])
