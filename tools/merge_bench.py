#!/usr/bin/env python3
"""Measures the engine behind `ccphylo merge` (ccg_ltd_merge_dev):

    python tools/merge_bench.py [--n 20000] [--out profiles/merge_bench.json]

Device time (HIP events around the call's kernels, the better of three runs) of
K = 16 weighted double sources into a union of --n rows:
  identity   every source holds all rows, in the union's order
  perm       every source holds all rows, each under its own random permutation
  subset10   every source holds a random 10 % of the rows, in random order
each under the scatter form (plan 1) and the gather form (plan 2), the gather
form also as 16 calls of one source (every call walks the union again).
Beside each time stands the byte count the form must move by its own model,
with E = 8 bytes, U the union's cells and S the batch's source cells:
  gather   4 E U per call (D and N read and written) + 2 E S (d and w read)
  scatter  2 E S (d and w read) + 4 E S (D and N read-modify-written in place)
(the index tables, 4 bytes a lookup and mostly cache hits, are left out), and
the time a plain streaming read-and-write (tools/micro/stream_rw.hip) takes
for that byte count at the rate it reaches on this device in this run.

Crossover of the automatic plan: 16 random-subset sources whose cells are a
share r of the union's, r swept; the r at which the gather form overtakes the
scatter form (log-linear between the bracketing points) is what MRG_CROSSOVER
in csrc/merge.hip is set from.

End to end: the CLI beside the reference binary (oracle/_ref/ccphylo, where it
was built) on one weighted input inside the reference's envelope (126 names, 16
matrices), wall time, with the CLI's own device time (CCPHYLO_MERGE_TIMES).
Needs an MI355X; there is no fallback."""
import argparse
import ctypes as C
import gzip
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MICRO = os.path.join(ROOT, "tools", "micro")
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
K, E = 16, 8


def rw_lib():
    so = os.path.join(MICRO, "libstream_rw.so")
    src = os.path.join(MICRO, "stream_rw.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-shared",
                        "-fPIC", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.stream_rw.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    return lib


def tri(n):
    return n * (n - 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    a = ap.parse_args()
    import torch
    import ccphylo_amd as cg
    from dbscan_bench import timed
    dev = cg.Device(0)
    n = a.n
    U = tri(n)
    rng = np.random.default_rng(n)
    gen = torch.Generator(device="cuda").manual_seed(n)
    D = torch.zeros(U, dtype=torch.float64, device="cuda")
    N = torch.zeros(U, dtype=torch.float64, device="cuda")
    # distinct buffers per source: a shared one would be a cache hit from the second source on
    ds = [torch.rand(U, dtype=torch.float64, device="cuda", generator=gen) for _ in range(K)]
    ws = [torch.rand(U, dtype=torch.float64, device="cuda", generator=gen) for _ in range(K)]
    torch.cuda.synchronize()

    # ---- the yardstick: bytes moved per second by a plain read-and-write stream
    lib = rw_lib()
    nbytes = U * E // 16 * 16
    s, reps = timed(lambda: lib.stream_rw(D.data_ptr(), nbytes, 2048), lib.stream_sync)
    rw_rate = 2 * nbytes / s
    D.zero_()
    torch.cuda.synchronize()
    yard = {"buffer_bytes": nbytes, "bytes_moved": 2 * nbytes, "ms": s * 1e3, "reps": reps, "TBps": rw_rate / 1e12}
    print(json.dumps({"stream_rw": yard}), flush=True)

    def run(idxs, plan, batch):
        """device ms of the K sources, `batch` a call, the better of three runs"""
        m = len(idxs[0])
        best = None
        for _ in range(3):
            ms = 0.0
            for k0 in range(0, K, batch):
                srcs = [(ds[k].data_ptr(), ws[k].data_ptr(), idxs[k]) for k in range(k0, k0 + batch)]
                dev.ltd_merge_dev(D.data_ptr(), N.data_ptr(), n, srcs, n, etype=8, weighted=True, plan=plan)
                assert dev.last_merge_plan() == plan
                ms += dev.last_merge_ms()
            best = ms if best is None else min(best, ms)
        S = K * tri(m)
        calls = K // batch
        model = (4 * E * U * calls + 2 * E * S) if plan == cg.MERGE_GATHER else 6 * E * S
        return {"plan": plan, "batch": batch, "rows": m, "source_cells": S, "device_ms": best, "model_bytes": model,
                "model_TBps": model / (best * 1e-3) / 1e12, "stream_rw_ms": model / rw_rate * 1e3,
                "over_stream_rw": best / (model / rw_rate * 1e3)}

    patterns = {
        "identity": [np.arange(n, dtype=np.int32) for _ in range(K)],
        "perm": [rng.permutation(n).astype(np.int32) for _ in range(K)],
        "subset10": [rng.permutation(n)[:n // 10].astype(np.int32) for _ in range(K)],
    }
    device = []
    for name, idxs in patterns.items():
        for plan, batch in ((cg.MERGE_SCATTER, K), (cg.MERGE_GATHER, K), (cg.MERGE_GATHER, 1)):
            r = dict(pattern=name, **run(idxs, plan, batch))
            device.append(r)
            print(json.dumps(r), flush=True)

    # ---- the two forms agree bit for bit (from a zeroed union, n_prev = 0)
    D2, N2 = torch.empty_like(D), torch.empty_like(N)
    srcs = [(ds[k].data_ptr(), ws[k].data_ptr(), patterns["subset10"][k]) for k in range(K)]
    dev.ltd_merge_dev(D.data_ptr(), N.data_ptr(), n, srcs, 0, etype=8, weighted=True, first=True, plan=cg.MERGE_SCATTER)
    dev.ltd_merge_dev(D2.data_ptr(), N2.data_ptr(), n, srcs, 0, etype=8, weighted=True, first=True, plan=cg.MERGE_GATHER)
    same = bool(torch.equal(D.view(torch.int64), D2.view(torch.int64)) and torch.equal(N.view(torch.int64), N2.view(torch.int64)))
    assert same
    del D2, N2

    # ---- the crossover: source cells / union cells at which gather overtakes scatter
    sweep = []
    for r in (0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.4, 0.8):
        m = max(2, int(round(n * math.sqrt(r / K))))
        idxs = [rng.permutation(n)[:m].astype(np.int32) for _ in range(K)]
        sc, ga = run(idxs, cg.MERGE_SCATTER, K), run(idxs, cg.MERGE_GATHER, K)
        row = {"rows": m, "ratio": K * tri(m) / U, "scatter_ms": sc["device_ms"], "gather_ms": ga["device_ms"]}
        sweep.append(row)
        print(json.dumps(row), flush=True)
    cross = None
    for lo, hi in zip(sweep, sweep[1:]):
        a0, a1 = math.log(lo["scatter_ms"] / lo["gather_ms"]), math.log(hi["scatter_ms"] / hi["gather_ms"])
        if a0 < 0 <= a1:   # scatter faster at lo, gather at hi
            t = -a0 / (a1 - a0)
            cross = math.exp(math.log(lo["ratio"]) + t * (math.log(hi["ratio"]) - math.log(lo["ratio"])))
    del ds, ws, D, N
    torch.cuda.empty_cache()
    dev.close()

    # ---- end to end beside the reference, inside its envelope
    e2e = None
    with gzip.open(os.path.join(ROOT, "tests", "golden", "merge", "edge126.phy.gz"), "rt") as f:
        lines = f.read().split("\n")
    names = [ln.split("\t")[0] for ln in lines[65:65 + 126]]   # 126 names the reference is known to keep
    assert len(set(names)) == 126

    def phy(order, vals):
        out, k = ["%10d\n" % len(order)], 0
        for i, nm in enumerate(order):
            out.append(nm + "".join("\t%.6f" % v for v in vals[k:k + i]) + "\n")
            k += i
        return "".join(out)
    sets = [names[:63]] + [list(rng.permutation(names)) for _ in range(K - 1)]
    with tempfile.TemporaryDirectory() as tmp:
        dp, wp = os.path.join(tmp, "d.phy"), os.path.join(tmp, "w.phy")
        with open(dp, "w") as f:
            f.write("".join(phy(s, rng.uniform(0, 100, tri(len(s)))) for s in sets))
        with open(wp, "w") as f:
            f.write("".join(phy(s, rng.integers(1, 5000, tri(len(s))).astype(float)) for s in sets))
        args = ["merge", "-i", dp, "-w", wp, "-o", os.path.join(tmp, "o"), "-n", os.path.join(tmp, "nn")]
        env = dict(os.environ, CCPHYLO_MERGE_TIMES="1")
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            p = subprocess.run([cg.CLI_PATH] + args, capture_output=True, env=env)
            walls.append(time.perf_counter() - t0)
        assert p.returncode == 0, p.stderr
        dev_ms = float(p.stderr.decode().split("# merge:")[1].split("ms")[0])
        with open(os.path.join(tmp, "o"), "rb") as f:
            ours = f.read()
        e2e = {"names": 126, "matrices": K, "input_bytes": os.path.getsize(dp) + os.path.getsize(wp),
               "cli_wall_s": min(walls), "cli_wall_runs": walls, "cli_device_ms": dev_ms,
               "device_share_of_wall": dev_ms * 1e-3 / min(walls),
               "note": "the CLI's wall time is process start, opening the GPU and parsing two text files; "
                       "the device time is the batch's and the close's kernels"}
        if os.path.exists(REF):
            rw = []
            for _ in range(3):
                t0 = time.perf_counter()
                q = subprocess.run([REF] + args, capture_output=True)
                rw.append(time.perf_counter() - t0)
            with open(os.path.join(tmp, "o"), "rb") as f:
                theirs = f.read()
            e2e.update(reference_wall_s=min(rw), reference_rc=q.returncode, same_bytes=ours == theirs)
    print(json.dumps(e2e), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "n": n, "sources": K, "etype": 8, "stream_rw": yard,
           "device_time": device, "forms_bitwise_equal": same, "crossover_sweep": sweep, "crossover_ratio": cross,
           "end_to_end": e2e}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
