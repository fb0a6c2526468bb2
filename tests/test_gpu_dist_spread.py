"""GPU parity of k_snp_mfma3 with the ring's DMA pieces spread over the chunk:
the default dist path against the VALU tile kernel (CCG_DIST_MFMA=0), bit for
bit on the output bytes, as test_gpu_dist_ring.py compares them.

Iteration c of the kernel's steady loop issues the 8 pieces of chunk c + 3, two
in each of its four steps, into the stage chunk c - 1 has just left; the
prologue issues chunks 0 .. 2 only.  What can go wrong is a piece that
overwrites a stage still being read, a counted wait that no longer counts whole
chunks, or the second copy of the loop (the last three opens of a tile)
entered with other pieces outstanding than it counts.  The cases are the
chunks per launch item where those differ:

    4              exactly the ring: the steady loop runs once, its pieces
                   (chunk 3) go into the one stage no chunk has used yet
    5, 6, 7, 8     the first ring cycle: every stage overwritten once
    9, 12, 13      the second and third cycles; with 5 .. 8 the second copy
                   is entered at every residue of the chunk count mod 4

The planes hold Wp words per taxon, the included words rounded up to 16, so a
whole row is an even number of 8-word chunks: an item of an even count C is
the whole row (L = 256 C - 177 is 8 C - 5 words, CCG_DIST_SLICES=1, one slice),
and an item of an odd count C is one of the two equal slices of a row of 2 C
chunks (L = 512 C - 177, CCG_DIST_SLICES=2).  last_dist_plan() reads the plan
back, so that every case asserts the slices the kernel really got.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNKS = [4, 5, 6, 7, 8, 9, 12, 13]


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    d = cg.Device(0)
    yield d
    d.close()


def _alignment(n, L):
    rng = np.random.default_rng(n + L)
    W = L // 32 + 1
    seqs = rng.integers(-2**62, 2**62, (n, W), dtype=np.int64)
    seqs[:, : W // 3] = seqs[0, : W // 3]
    inc = np.full(W, -1, dtype=np.int32)
    inc[(L + 31) // 32:] = 0
    if L % 32:
        inc[(L + 31) // 32 - 1] = ((0xFFFFFFFF << (32 - L % 32)) & 0xFFFFFFFF) - (1 << 32)
    inc[W // 2] &= 0x0F0F0F0F   # one masked word in the middle (it stays: no word is excluded whole)
    return seqs, inc, W


def _run(dev, monkeypatch, n, C, et):
    import torch
    S = 1 if C % 2 == 0 else 2
    L = 256 * C * S - 177
    seqs, inc, W = _alignment(n, L)
    s_d = torch.from_numpy(seqs).cuda()
    i_d = torch.from_numpy(inc).cuda()
    monkeypatch.setenv("CCG_DIST_SLICES", str(S))
    for k in ("CCG_DIST_GLDS", "CCG_DIST_KC", "CCG_DIST_ORDER", "CCG_DIST_NOCOMPACT"):
        monkeypatch.delenv(k, raising=False)
    out = {}
    for mode in ("valu", "default"):
        if mode == "valu":
            monkeypatch.setenv("CCG_DIST_MFMA", "0")
        else:
            monkeypatch.delenv("CCG_DIST_MFMA", raising=False)
        D = torch.zeros(n * (n - 1) // 2, dtype={8: torch.float64, 4: torch.float32}[et], device="cuda")
        dev.snp_ltd_dev(s_d.data_ptr(), i_d.data_ptr(), n, L, W, D.data_ptr(), etype=et)
        torch.cuda.synchronize()
        if mode == "default":   # every item is C chunks: S slices of 8 C words cover the 8 C S words exactly
            assert dev.last_dist_plan() == (S, 8 * C)
        out[mode] = D.cpu().numpy()
    assert (out["valu"].view(np.uint8) == out["default"].view(np.uint8)).all()
    assert out["default"].any()


@pytest.mark.parametrize("et", [8, 4])
@pytest.mark.parametrize("C", CHUNKS)
def test_dist_spread_equals_valu(dev, monkeypatch, C, et):
    """n = 300 (three tiles: one partial, one on the diagonal), items of C chunks."""
    _run(dev, monkeypatch, 300, C, et)


def test_dist_spread_six_tiles(dev, monkeypatch):
    """n = 600: six tiles of two 9-chunk items each, so the items outnumber a small context's blocks."""
    _run(dev, monkeypatch, 600, 9, 8)
