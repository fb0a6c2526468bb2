#!/usr/bin/env python3
"""Measures the two engine paths behind `nwck2phy` / `phycmp` / `tree --phycmp`:

    python tools/fit_bench.py [--sizes 10000,50000] [--out profiles/fit_bench.json]

Replay (ccg_nwck_ltd_dev, double): device time (HIP events around its kernels)
and kernel launches for a caterpillar and for a random balanced tree at each
size, the better of two runs.  The trees are written as Newick text with
9-decimal limbs and parsed by ccq_newick_splits (timed).  At the first size the
reference binary (oracle/_ref/ccphylo nwck2phy, where it was built) converts
the same file on this host, wall time, its Phylip text going to /dev/null --
that includes its text output, which the replay's device time does not.
Column walks: thread k > org of a split touches cell (k, org), a strided walk
of the packed LT.  `column_cells` counts those cells and `column_line_bytes`
charges each a 128-byte line read and written back, beside `cell_bytes`, the 8
bytes per cell touched that a dense layout would move.  These two are counted
from the split list, not read from hardware counters.

Comparison (ccg_ltd_cmp_dev, double, no perm, at the last size): the time of
its two kernels beside a plain 16-byte streaming read-and-sum of the same two
buffers (tools/micro/stream_sum.hip).  Needs an MI355X; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
LINE = 128


def caterpillar(n):
    parts = ["(c0:1.000000000,c1:%.9f)" % 1.5]
    for i in range(2, n - 1):
        parts.append(":0.500000000,c%d:%.9f)" % (i, 1 + (i % 97) / 7))
    return ("(" * (n - 1) + parts[0][1:] + "".join(parts[1:]) + ":0.250000000,c%d:2.000000000);" % (n - 1)).encode()


def balanced(n, rng):
    nodes = ["t%d" % i for i in rng.permutation(n)]
    limb = rng.random(2 * n + 8) * 3 + 0.001
    k = 0
    while len(nodes) > 3:
        nxt = []
        for a in range(0, len(nodes) - 1, 2):
            nxt.append("(%s:%.9f,%s:%.9f)" % (nodes[a], limb[k], nodes[a + 1], limb[k + 1]))
            k += 2
        if len(nodes) & 1:
            nxt.append(nodes[-1])
        nodes = nxt
    return ("(" + ",".join("%s:%.9f" % (c, limb[k + i]) for i, c in enumerate(nodes)) + ");").encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.json"))
    a = ap.parse_args()
    import torch
    import ccphylo_amd as cg
    from ccphylo_amd import native
    from dbscan_bench import stream_lib, timed
    dev = cg.Device(0)
    sizes = [int(x) for x in a.sizes.split(",")]
    rng = np.random.default_rng(1)
    replay = []
    for n in sizes:
        for shape, text in (("caterpillar", caterpillar(n)), ("balanced", balanced(n, rng))):
            t0 = time.perf_counter()
            _, names, sp = native.newick_splits(text)
            parse_s = time.perf_counter() - t0
            assert len(names) == n
            m = np.arange(1, n)
            col = int((m - 1 - sp["org"]).sum())
            res = {"n": n, "shape": shape, "text_bytes": len(text), "parse_ms": parse_s * 1e3,
                   "cells_touched": int(2 * m.sum()), "cell_bytes": int(2 * m.sum()) * 8,
                   "column_cells": col, "column_line_bytes": col * 2 * LINE}
            res["column_over_cell_bytes"] = res["column_line_bytes"] / res["cell_bytes"]
            D = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            runs = []
            for _ in range(2):
                dev.nwck_ltd_dev(sp, D.data_ptr(), 8)
                runs.append(dev.last_nwck())
            res["device_ms"] = min(r[0] for r in runs)
            res["launches"] = runs[0][1]
            res["us_per_launch"] = res["device_ms"] * 1e3 / res["launches"]
            del D
            if n == sizes[0] and os.path.exists(REF):
                with tempfile.NamedTemporaryFile(suffix=".nwk") as f:
                    f.write(text + b"\n")
                    f.flush()
                    t0 = time.perf_counter()
                    p = subprocess.run([REF, "nwck2phy", "-i", f.name, "-o", os.devnull], capture_output=True)
                    res["reference_wall_s"] = time.perf_counter() - t0
                    res["reference_rc"] = p.returncode
            replay.append(res)
            print(json.dumps(res), flush=True)
    # comparison against a streaming read of both buffers
    n = sizes[-1]
    cells = n * (n - 1) // 2
    gen = torch.Generator(device="cuda").manual_seed(n)
    A = torch.rand(cells, dtype=torch.float64, device="cuda", generator=gen) * 10
    B = A * (1 + 0.1 * torch.rand(cells, dtype=torch.float64, device="cuda", generator=gen))
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        sums, _ = dev.ltd_cmp_dev(A.data_ptr(), B.data_ptr(), n, 8)
        ms.append(dev.last_cmp_ms())
    assert abs(sums["l1"] - float((A - B).abs().sum().item())) <= 1e-9 * sums["l1"]
    lib = stream_lib()
    acc = torch.zeros(1, dtype=torch.int64, device="cuda")
    nbytes = cells * 8 // 16 * 16

    def both():
        lib.stream_sum(A.data_ptr(), nbytes, acc.data_ptr(), 2048)
        lib.stream_sum(B.data_ptr(), nbytes, acc.data_ptr(), 2048)
    s, reps = timed(both, lib.stream_sync)
    cmp = {"n": n, "etype": 8, "bytes": 2 * cells * 8, "cmp_ms": min(ms[1:]), "cmp_ms_runs": ms,
           "cmp_TBps": 2 * cells * 8 / (min(ms[1:]) * 1e-3) / 1e12,
           "stream_ms": s * 1e3, "stream_reps": reps, "stream_TBps": 2 * cells * 8 / s / 1e12}
    cmp["cmp_over_stream"] = cmp["cmp_ms"] / cmp["stream_ms"]
    print(json.dumps(cmp), flush=True)
    dev.close()
    out = {"device": torch.cuda.get_device_name(0), "line_bytes": LINE, "replay": replay, "compare": cmp}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
