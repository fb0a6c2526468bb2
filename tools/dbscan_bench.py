#!/usr/bin/env python3
"""Times dbscan's count pass (k_dbscan_count, the one read of the LT) against
a plain 16-byte streaming read-and-sum kernel over the same device buffer
(tools/micro/stream_sum.hip), at n = 20k and 50k, f64 and f32:

    python tools/dbscan_bench.py [--sizes 20000,50000] [--out profiles/dbscan_bench.json]

Cells are uniform integers 0..199 (SNP-like).  The count pass is timed at
-e 10 (about 5.5 % of the cells are neighbours: compare, LDS histogram and row
heads) and at -e -2 (no neighbour: compare and row heads only), which tells
the histogram's cost from the rest.  Every figure is LT bytes over the time of
back-to-back launches that end in a device synchronise (a window of at least
0.3 s after a warm-up); the fraction is of the 6.29 TB/s measured copy rate.
Needs an MI355X; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MICRO = os.path.join(ROOT, "tools", "micro")
COPY_RATE = 6.29e12   # MI355X measured float4 copy rate, bytes / s


def stream_lib():
    so = os.path.join(MICRO, "libstream_sum.so")
    src = os.path.join(MICRO, "stream_sum.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-shared",
                        "-fPIC", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.stream_sum.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    return lib


def timed(enqueue, sync, window=0.3):
    """Seconds per call of `enqueue`, back to back, over at least `window` s."""
    for _ in range(3):
        enqueue()
    sync()
    reps = 4
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        sync()
        dt = time.perf_counter() - t0
        if dt >= window or reps >= 4096:
            return dt / reps, reps
        reps *= 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,50000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_bench.json"))
    a = ap.parse_args()
    import torch
    import ccphylo_amd as cg
    from ccphylo_amd import native   # noqa: F401  (binds the engine to torch's HIP runtime)
    dev = cg.Device(0)
    dev.configure(nosync=True)   # launches go back to back: torch's work is synchronised before the first one
    lib = stream_lib()
    acc = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = []
    for n in (int(x) for x in a.sizes.split(",")):
        m = n * (n - 1) // 2
        gen = torch.Generator(device="cuda").manual_seed(n)
        cells = torch.randint(0, 200, (m,), dtype=torch.int16, device="cuda", generator=gen)
        Nd = torch.zeros(n, dtype=torch.int32, device="cuda")
        fd = torch.zeros(n, dtype=torch.int32, device="cuda")
        for etype, dt in ((8, torch.float64), (4, torch.float32)):
            D = cells.to(dt)
            torch.cuda.synchronize()
            nbytes = m * etype
            res = {"n": n, "etype": etype, "lt_bytes": nbytes}
            for tag, e in (("count_e10", 10.0), ("count_none", -2.0)):
                s, reps = timed(lambda: dev.dbscan_count_dev(D.data_ptr(), n, Nd.data_ptr(), fd.data_ptr(), e, etype),
                                dev.sync)
                res[tag] = {"ms": s * 1e3, "reps": reps, "TBps": nbytes / s / 1e12, "of_copy_rate": nbytes / s / COPY_RATE}
            # check the pass against torch on the way: the sum of N is twice the neighbour cells
            dev.dbscan_count_dev(D.data_ptr(), n, Nd.data_ptr(), fd.data_ptr(), 10.0, etype)
            dev.sync()
            assert int(Nd.sum().item()) == 2 * int((cells <= 10).sum().item())
            vec_bytes = nbytes // 16 * 16
            s, reps = timed(lambda: lib.stream_sum(D.data_ptr(), vec_bytes, acc.data_ptr(), 2048), lib.stream_sync)
            res["stream_sum"] = {"ms": s * 1e3, "reps": reps, "TBps": nbytes / s / 1e12, "of_copy_rate": nbytes / s / COPY_RATE}
            res["count_over_stream"] = res["count_e10"]["ms"] / res["stream_sum"]["ms"]
            res["count_none_over_stream"] = res["count_none"]["ms"] / res["stream_sum"]["ms"]
            res["within_2x"] = res["count_over_stream"] <= 2.0
            rows.append(res)
            print(json.dumps(res), flush=True)
            del D
    dev.close()
    out = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12,
           "cells": "uniform integers 0..199", "results": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
