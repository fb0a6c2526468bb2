#!/usr/bin/env python3
"""Times `dist -y`'s motif masking kernel (k_meth, one pass over the packed
alignment) against a plain streaming read of the same device buffer
(tools/micro/stream_sum.hip, the yardstick of tools/dbscan_bench.py), the
end-to-end CLI cost of `-y`, and -- where the checker binary oracle/_ref/ccphylo
is present -- the reference's own `dist -y` minus `dist` on a bounded sample:

    python tools/meth_bench.py [--taxa 10000 --length 5000000] [--out profiles/meth_bench.json]

Rows are uniform random bases; the motif table is three records of lengths 4,
5 and 6 (gAtc, ccWgg, gaNNtc: 6 strands).  The kernel and the streaming read
are timed the same way: back-to-back launches that end in a synchronise, over a
window of at least 0.3 s after a warm-up (the engine runs on its own stream, so
this brackets exactly its launches); the figure is packed-row bytes over that
time.  Needs an MI355X; there is no fallback."""
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
MOTIFS = b">dam\ngAtc\n>dcm\nccWgg\n>six\ngaNNtc\n"


def write_msa(path, n, L, rng):
    anc = rng.integers(0, 4, L, dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for t in range(n):
            s = anc.copy()
            at = rng.integers(0, L, max(L // 500, 1))
            s[at] = rng.integers(0, 4, len(at), dtype=np.uint8)
            f.write(b">t%d\n" % t + lut[s].tobytes() + b"\n")


def wall(cmd, reps=2):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taxa", type=int, default=10000)
    ap.add_argument("--length", type=int, default=5000000)
    ap.add_argument("--cli-taxa", type=int, default=2000)
    ap.add_argument("--cli-length", type=int, default=100000)
    ap.add_argument("--ref-taxa", type=int, default=256)
    ap.add_argument("--ref-length", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meth_bench.json"))
    a = ap.parse_args()
    import torch
    import ccphylo_amd as cg
    from ccphylo_amd import native
    from dbscan_bench import COPY_RATE, stream_lib, timed
    tmp = tempfile.mkdtemp(prefix="meth_bench_")
    mpath = os.path.join(tmp, "motifs.fa")
    with open(mpath, "wb") as f:
        f.write(MOTIFS)
    tab = native.load_motifs(mpath)
    assert len(tab) == 6 and sorted(set(int(x) for x in tab["len"])) == [4, 5, 6]
    dev = cg.Device(0)
    dev.configure(nosync=True)
    lib = stream_lib()
    n, L = a.taxa, a.length
    W = L // 32 + 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    seqs = torch.empty((n, W), dtype=torch.int64, device="cuda")
    step = max(1, (1 << 28) // W)
    for t0 in range(0, n, step):   # in pieces: randint's temporaries stay small
        shape = seqs[t0:t0 + step].shape
        hi = torch.randint(0, 2 ** 32, shape, dtype=torch.int64, device="cuda", generator=gen)
        seqs[t0:t0 + step] = (hi << 32) | torch.randint(0, 2 ** 32, shape, dtype=torch.int64, device="cuda", generator=gen)
        del hi
    seqs[:, L // 32] = 0 if L % 32 == 0 else seqs[:, L // 32] & (-1 << (2 * (32 - L % 32)))   # left-aligned tail
    nbytes = n * W * 8
    acc = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = {"taxa": n, "length": L, "stride_words": W, "packed_bytes": nbytes, "strands": int(len(tab)),
           "strand_lengths": [int(x) for x in tab["len"]]}
    for pair in (False, True):
        incs = torch.full((n, W) if pair else (W,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cnt, found = dev.meth_mask_dev(seqs.data_ptr(), incs.data_ptr(), n, L, W, tab, pair=pair)
        # uniform bases: a strand of m fixed bases matches a start with probability 4^-m (ccWgg: 2 * 4^-5, gaNNtc: 4^-4)
        expect = n * L * 2 * (4.0 ** -4 + 2 * 4.0 ** -5 + 4.0 ** -4)
        assert abs(found - expect) < 0.01 * expect, (found, expect)
        s, reps = timed(lambda: dev.meth_mask_dev(seqs.data_ptr(), incs.data_ptr(), n, L, W, tab, pair=pair,
                                                  want_counts=False), dev.sync)
        res["pair" if pair else "nonpair"] = {"ms": s * 1e3, "reps": reps, "TBps": nbytes / s / 1e12,
                                              "of_copy_rate": nbytes / s / COPY_RATE, "matches": int(found),
                                              "inc_count_0": int(cnt[0])}
        del incs
    s, reps = timed(lambda: lib.stream_sum(seqs.data_ptr(), nbytes // 16 * 16, acc.data_ptr(), 2048), lib.stream_sync)
    res["stream_sum"] = {"ms": s * 1e3, "reps": reps, "TBps": nbytes / s / 1e12, "of_copy_rate": nbytes / s / COPY_RATE}
    for k in ("nonpair", "pair"):
        res[k + "_over_stream"] = res[k]["ms"] / res["stream_sum"]["ms"]
    print(json.dumps(res), flush=True)
    del seqs
    dev.close()
    out = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "rows": "uniform random bases",
           "motifs": MOTIFS.decode(), "kernel": res}
    # ---- the CLI end to end: -y loads the motifs, uploads the packed rows once more and masks
    rng = np.random.default_rng(3)
    msa = os.path.join(tmp, "cli.fsa")
    write_msa(msa, a.cli_taxa, a.cli_length, rng)
    base = [cg.CLI_PATH, "dist", "-i", msa, "-o", os.path.join(tmp, "d.phy")]
    t_plain, t_meth = wall(base), wall(base + ["-y", mpath])
    out["cli"] = {"taxa": a.cli_taxa, "length": a.cli_length, "packed_bytes": a.cli_taxa * (a.cli_length // 32 + 1) * 8,
                  "dist_s": t_plain, "dist_y_s": t_meth, "y_cost_s": t_meth - t_plain}
    print(json.dumps(out["cli"]), flush=True)
    # ---- the reference's own cost on this host's CPU, for scale
    ref = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
    if os.path.exists(ref):
        small = os.path.join(tmp, "ref.fsa")
        write_msa(small, a.ref_taxa, a.ref_length, rng)
        rb = [ref, "dist", "-i", small, "-o", os.path.join(tmp, "r.phy")]
        r_plain, r_meth = wall(rb), wall(rb + ["-y", mpath])
        cost = r_meth - r_plain
        out["reference_cpu"] = {"taxa": a.ref_taxa, "length": a.ref_length, "dist_s": r_plain, "dist_y_s": r_meth,
                                "y_cost_s": cost, "y_cost_ns_per_base": cost / (a.ref_taxa * a.ref_length) * 1e9,
                                "scaled_to_kernel_size_s": cost / (a.ref_taxa * a.ref_length) * n * L}
        print(json.dumps(out["reference_cpu"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name in os.listdir(tmp):
        os.unlink(os.path.join(tmp, name))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
