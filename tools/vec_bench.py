#!/usr/bin/env python3
"""Times the tsv2phy pair kernel (ccg_vec_ltd_dev; ccg_last_vec_ms = pre-pass +
pair kernel, HIP events) for cos and bc on double and float rows, at 50 000 x
4096 (a 1.6 GB table, a 10 GB LT) and 2000 x 4096:

    python tools/vec_bench.py [--shapes 50000x4096,2000x4096] [--out profiles/vec_bench.json]

Every figure is also given as pair-columns per second (m(m-1)/2 * n over the
time) and as a fraction of the chip's measured issue rate of plain v_mul_f64 +
v_add_f64 pairs (tools/micro/f64_rate.hip: 16 chains per lane from registers):
a cos pair-column IS one such pair, so that fraction is the kernel's distance
from the f64 vector unit's limit; a bc pair-column is two adds, a compare and a
select (and a float add with -p).  The reference binary (oracle/_ref/ccphylo,
where it was built) is timed on a bounded 512-row sample of the same table and
scaled by the pair count, as bench.py's cpu_baseline does.
Needs an MI355X; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MICRO = os.path.join(ROOT, "tools", "micro")
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
SAMPLE_ROWS = 512


def rate_lib():
    so = os.path.join(MICRO, "libf64_rate.so")
    src = os.path.join(MICRO, "f64_rate.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3",
                        "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.f64_pair_rate.restype = C.c_double
    lib.f64_pair_rate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return lib


def reference_sample(X, metric, vtype):
    """Wall seconds of the reference on the first SAMPLE_ROWS rows (None without the binary)."""
    if not os.path.exists(REF):
        return None
    rows = X[:SAMPLE_ROWS].double().cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sample.tsv")
        with open(path, "w") as f:
            f.write("\t".join("c%d" % k for k in range(rows.shape[1])) + "\n")
            for r in rows:
                f.write("\t".join("%.3f" % v for v in r) + "\n")
        t0 = time.perf_counter()
        subprocess.run([REF, "tsv2phy", "-i", path, "-d", metric, "-o", os.path.join(d, "o.phy")] +
                       (["-p"] if vtype == 4 else []), check=True, capture_output=True)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x4096,2000x4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vec_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import ccphylo_amd as cg
    from ccphylo_amd import native   # noqa: F401  (binds the engine to torch's HIP runtime)
    dev = cg.Device(0)
    lib = rate_lib()
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    rin = torch.rand(2048, dtype=torch.float64, device="cuda")
    rout = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rates = [lib.f64_pair_rate(rin.data_ptr(), rout.data_ptr(), cus * 16, 20000) for _ in range(3)]
    pair_rate = max(rates)
    assert pair_rate > 0
    print(json.dumps({"f64_mul_add_pairs_per_s": pair_rate, "runs": rates, "cus": cus}), flush=True)
    rows = []
    ref_cache = {}   # one sample run per (metric, vtype): the samples have one size
    for m, n in ((int(p) for p in s.split("x")) for s in a.shapes.split(",")):
        gen = torch.Generator(device="cuda").manual_seed(m)
        X8 = (torch.rand((m, n), dtype=torch.float64, device="cuda", generator=gen) * 10).mul_(1000).round_().div_(1000)
        D = torch.empty(m * (m - 1) // 2, dtype=torch.float64, device="cuda")
        for vtype in (8, 4):
            X = X8 if vtype == 8 else X8.float()
            torch.cuda.synchronize()
            for metric in ("cos", "bc"):
                ms = []
                for _ in range(a.reps + 1):   # the first run warms up
                    dev.vec_ltd_dev(X.data_ptr(), m, n, D.data_ptr(), vtype=vtype, metric=metric)
                    ms.append(dev.last_vec_ms())
                best = min(ms[1:])
                steps = m * (m - 1) // 2 * n
                res = {"m": m, "n": n, "vtype": vtype, "metric": metric, "tile": dev.last_vec_plan()[0],
                       "vec_ms": best, "runs_ms": ms[1:], "pair_columns_per_s": steps / (best * 1e-3),
                       "of_f64_mul_add_rate": steps / (best * 1e-3) / pair_rate}
                if (metric, vtype) not in ref_cache:
                    ref_cache[(metric, vtype)] = reference_sample(X8, metric, vtype)
                ref_s = ref_cache[(metric, vtype)]
                if ref_s is not None:
                    sample_pairs = SAMPLE_ROWS * (SAMPLE_ROWS - 1) // 2
                    res["reference_sample_s"] = ref_s
                    res["reference_scaled_s"] = ref_s * (m * (m - 1) // 2) / sample_pairs
                    res["speedup_over_reference"] = res["reference_scaled_s"] / (best * 1e-3)
                rows.append(res)
                print(json.dumps(res), flush=True)
        del D, X8
    dev.close()
    out = {"device": torch.cuda.get_device_name(0), "cus": cus, "f64_mul_add_pairs_per_s": pair_rate,
           "f64_mul_add_pairs_per_s_runs": rates, "table": "uniform 0..10, three decimals",
           "reference_sample_rows": SAMPLE_ROWS, "results": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
