"""Where a chunk of k_snp_mfma3's main loop spends its cycles: runs the headline
dist once on the stamps engine (make -C ccphylo_amd stamps, CCG_DIST_STAMPS in
snp.hip) and prints, per part of a chunk, the median over workgroups of the
s_memtime cycles per chunk, for wave 0 and wave 3, and each part's share.  The
stamps fence the schedule and drain the LDS reads in flight: the shares are
the record, not the length.

    CCPHYLO_AMD_ENGINE=ccphylo_amd/lib/libccphylo_amd_stamps.so python tools/dist_stamps.py [n] [L] [cus]
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARTS = ["step 0", "step 1", "step 2", "step 3 up to the wait", "wait + barrier", "component 1 of step 3",
         "rest of step 3"]


def main():
    import numpy as np
    import torch
    import ccphylo_amd as cg
    from bench import make_headline_alignment
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 5_000_000
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 192
    out = os.path.join(tempfile.mkdtemp(), "stamps.bin")
    os.environ["CCG_DIST_STAMPS_OUT"] = out
    seqs, incs, W = make_headline_alignment(torch, n, L)
    D = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device="cuda")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    dev = cg.Device(0)
    if k < ncu:
        dev.configure(cu_mask=list(range(ncu - k, ncu)), nosync=True)
    dev.snp_ltd_dev(seqs.data_ptr(), incs.data_ptr(), n, L, W, D.data_ptr())
    ms = dev.last_dist_ms()
    dev.close()
    st = np.fromfile(out, dtype=np.uint64).reshape(-1, 2, 8).astype(np.float64)
    st = st[st[:, 0, 7] > 0]
    per = st[:, :, :7] / st[:, :, 7:8]   # cycles per chunk
    print(f"k_snp_mfma3 chunk stamps: n={n} L={L} on {k} CUs, {len(st)} workgroups x {int(st[0, 0, 7])} stamped chunks, "
          f"stamped launch {ms:.0f} ms (not a timing)")
    print(f"{'part':28s} {'wave 0: cycles/chunk':>22s} {'share':>7s} {'wave 3: cycles/chunk':>22s} {'share':>7s}")
    med = np.median(per, axis=0)
    for i, name in enumerate(PARTS):
        print(f"{name:28s} {med[0, i]:22.0f} {med[0, i] / med[0].sum():7.3f} {med[1, i]:22.0f} "
              f"{med[1, i] / med[1].sum():7.3f}")
    print(f"{'chunk':28s} {med[0].sum():22.0f} {'':7s} {med[1].sum():22.0f}")


if __name__ == "__main__":
    main()
