"""GPU parity of k_snp_mfma3's stage ring: the default dist path against the
VALU tile kernel (CCG_DIST_MFMA=0), bit for bit on the output bytes, at the
chunk counts per launch item where the 4-stage LDS ring, the counted waits
and the DMA pieces issued between the MFMAs of a chunk's last step can go
wrong.

The host pads the plane width Wp to 16 words, so a whole row is an even
number C = Wp / 8 of 8-word chunks; an item of 1, 3 or 5 chunks exists only
as a split-K slice.  With n = 300 (three 256 x 256 tiles: one partial, one on
the diagonal) the host plan (snp_launch_mfma2) splits as far as it may:
S = C / 4 slices of Wk = 8 ceil(C / S) words, then S = ceil(Wp / Wk).  SLICES
below lists the chunks per slice that gives; the test recomputes the plan for
the device it runs on and asserts them, so the cases are what the kernel sees:

    1 chunk            land(0) with vmcnt(0), the peeled last chunk alone
    2 and 3 chunks     a prologue shorter than the ring; vmcnt(8), then (0)
    4 chunks           exactly the ring: every open is one of the last three
    5 and 6 chunks     the steady loop once and twice: the first wrap, the
                       pieces of chunks 4 and 5 issued between MFMAs
    5, 5, 4 / 5, 5, 5, 3 / 5, 5, 5, 5, 2 / 5 x 5, 1
                       unequal slices: the last slice's Wl differs from Wk
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 300
TILES = 3
# C = Wp / 8 -> chunks per split-K slice (one entry: S = 1, no split)
SLICES = {2: [2], 4: [4], 6: [6], 8: [4, 4], 10: [5, 5], 14: [5, 5, 4], 18: [5, 5, 5, 3], 22: [5, 5, 5, 5, 2],
          26: [5, 5, 5, 5, 5, 1]}


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def _plan(Wp, slots):
    """snp_launch_mfma2's split-K plan for TILES tiles: the chunks of each slice."""
    chunks = Wp // 8
    S = 1
    if TILES < 16 * slots:
        S = min(-(-16 * slots // TILES), chunks // 4)
        S = max(S, 1)
    Wk = -(-chunks // S) * 8
    S = -(-Wp // Wk)
    return [(min(Wk, Wp - s * Wk)) // 8 for s in range(S)]


def _alignment(L):
    rng = np.random.default_rng(N + L)
    W = L // 32 + 1
    seqs = rng.integers(-2**62, 2**62, (N, W), dtype=np.int64)
    seqs[:, : W // 3] = seqs[0, : W // 3]
    inc = np.full(W, -1, dtype=np.int32)
    inc[(L + 31) // 32:] = 0
    if L % 32:
        inc[(L + 31) // 32 - 1] = ((0xFFFFFFFF << (32 - L % 32)) & 0xFFFFFFFF) - (1 << 32)
    inc[W // 2] &= 0x0F0F0F0F   # one masked word in the middle (it stays: no word is excluded whole)
    return seqs, inc, W


# L = 256 C - 177 is 8 C - 5 words, the last one partial: Wp = 8 C.  L = 256 k - 17, k = 1 .. 9, is 8 k words
# (Wp / 8 = 2, 2, 4, 4, 6, 6, 8, 8, 10): the same plans at other row lengths and tail masks
LENGTHS = [256 * C - 177 for C in sorted(SLICES)] + [256 * k - 17 for k in range(1, 10)]


@pytest.mark.parametrize("et", [8, 4])
@pytest.mark.parametrize("L", LENGTHS)
def test_dist_ring_equals_valu(dev, monkeypatch, L, et):
    import torch
    W32 = (L + 31) // 32
    Wp = -(-W32 // 16) * 16
    C = Wp // 8
    assert _plan(Wp, torch.cuda.get_device_properties(0).multi_processor_count) == SLICES[C]
    seqs, inc, W = _alignment(L)
    s_d = torch.from_numpy(seqs).cuda()
    i_d = torch.from_numpy(inc).cuda()
    out = {}
    for mode in ("valu", "default"):
        if mode == "valu":
            monkeypatch.setenv("CCG_DIST_MFMA", "0")
        else:
            monkeypatch.delenv("CCG_DIST_MFMA", raising=False)
        monkeypatch.delenv("CCG_DIST_GLDS", raising=False)
        monkeypatch.delenv("CCG_DIST_KC", raising=False)
        monkeypatch.delenv("CCG_DIST_ORDER", raising=False)
        D = torch.zeros(N * (N - 1) // 2, dtype={8: torch.float64, 4: torch.float32}[et], device="cuda")
        dev.snp_ltd_dev(s_d.data_ptr(), i_d.data_ptr(), N, L, W, D.data_ptr(), etype=et)
        torch.cuda.synchronize()
        out[mode] = D.cpu().numpy()
    assert (out["valu"].view(np.uint8) == out["default"].view(np.uint8)).all()
    assert out["default"].any()
