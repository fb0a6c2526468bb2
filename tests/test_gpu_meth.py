"""GPU: `dist -y` methylation motif masking on the gfx950 engine (ccg_meth_mask /
ccg_meth_mask_dev, the CLI option and the fused --tree / --dbscan paths).
Masks, counts and the match count are integers: every comparison is bit for
bit, against tests/meth_oracle.py (pinned to the reference's bytes by
tests/test_meth_oracle.py) or the reference's own stdout / stderr
(tests/golden/meth).

The kernel gives one lane a 32-position word and folds SLICE taxa per atomic in
non-pair mode, BATCH strands per launch (METH_SLICE / METH_BATCH in
ccphylo_amd/csrc/meth.hip)."""
import json
import os
import subprocess

import numpy as np
import pytest

import meth_oracle as mo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
METH = os.path.join(GOLDEN, "meth")
with open(os.path.join(METH, "meth.json")) as _f:
    CASES = json.load(_f)["cases"]
SLICE, BATCH = 64, 64
LENGTHS = (2, 31, 32, 33, 63, 64, 65, 96, 97)
TAXA = (1, 2, 63, 64, SLICE + 1)
NMAX = max(TAXA)
ACGT8 = "acgt" * 8


def tables():
    many = ["%s%s%s" % (a, b.upper(), c) for a in "acgt" for b in "acgt" for c in "acgt"] + ["aNn", "cNn", "gNn", "tNn"]
    t = {
        "short": mo.strands_of("aA", "gAtc", "Tag", "gaNtc", "RRg"),           # m = 2, 3, 4, 5
        "long": mo.strands_of(ACGT8[:30] + "G", ACGT8[:31] + "T", "nN"),        # m = 31, 32 (and > L for the short rows)
        "many": mo.strands_of(*many),                                           # 136 strands: three launches
    }
    assert len(t["many"]) > 2 * BATCH and {int(x) for x in t["long"]["len"]} == {2, 31, 32}
    return t


def rows_of(L):
    """NMAX rows of 2-bit codes: random; ACGT repeats (the 31 / 32-mers match at
    every fourth start, also from position 1 to 32 and 32 to 63); all A (what
    an N column is stored as: `aA` matches at every start but the last, where
    only the padding would complete it); GATC planted across the word boundary
    (30 .. 33), up to bit 0 of word 1 (60 .. 63), from bit 31 of word 2
    (64 .. 67) and up to L - 1; a row ending in `A` after a non-A."""
    rng = np.random.default_rng(1000 + L)
    out = np.zeros((NMAX, L), dtype=np.uint8)
    gatc = [2, 0, 3, 1]
    for t in range(NMAX):
        kind = t % 5
        c = rng.integers(0, 4, L).astype(np.uint8)
        if kind == 1:
            c = ((np.arange(L) + t // 5) % 4).astype(np.uint8)
        elif kind == 2:
            c[:] = 0
        elif kind == 3:
            for at in (30, 60, 64, L - 4):
                if 0 <= at and at + 4 <= L:
                    c[at:at + 4] = gatc
        elif kind == 4 and L >= 2:
            c[-2:] = [1, 0]
        out[t] = c
    return out


_ref = {}


def reference(L):
    """Per length, once: packed rows, and per table each row's clear words and matches."""
    if L not in _ref:
        codes = rows_of(L)
        W = L // 32 + 1
        seqs = np.array([mo.pack(c, W) for c in codes], dtype=np.uint64)
        per = {}
        for name, tab in tables().items():
            got = [mo.sites(c, tab) for c in codes]
            per[name] = (np.array([mo.to_words(cl, W) for cl, _ in got], dtype=np.uint32),
                         np.array([f for _, f in got], dtype=np.int64))
        _ref[L] = (seqs, per)
    return _ref[L]


def npos(m, L):
    return int(sum(bin(int(x)).count("1") for x in np.asarray(m)[:(L + 31) // 32]))


def expect(L, n, name, incs, pair, stride):
    _, per = reference(L)
    clr, found = per[name]
    c = np.zeros((n, stride), dtype=np.uint32)
    c[:, :clr.shape[1]] = clr[:n]
    if pair:
        out = incs & ~c
        cnt = [npos(r, L) for r in out]
    else:
        out = incs & ~np.bitwise_or.reduce(c, axis=0)
        cnt = [npos(out, L)] * n
    return out, np.array(cnt, dtype=np.int32), int(found[:n].sum())


def inputs(L, n, pair, slack, rng):
    """stride = L / 32 + 1 exactly, or two words more with garbage in every word past the data."""
    seqs0, _ = reference(L)
    W, Wd = L // 32 + 1, (L + 31) // 32
    stride = W + slack
    seqs = np.zeros((n, stride), dtype=np.uint64)
    seqs[:, :W] = seqs0[:n]
    full = np.zeros(stride, dtype=np.uint32)
    full[:Wd] = 0xFFFFFFFF
    if L % 32:
        full[Wd - 1] = (0xFFFFFFFF << (32 - L % 32)) & 0xFFFFFFFF
    incs = rng.integers(0, 2 ** 32, (n, stride) if pair else stride, dtype=np.uint64).astype(np.uint32) | 0x11111111
    incs &= full
    if slack:
        seqs[:, Wd:] = rng.integers(1, 2 ** 63, (n, stride - Wd), dtype=np.uint64)
        incs[..., Wd:] = rng.integers(1, 2 ** 32, incs[..., Wd:].shape, dtype=np.uint64).astype(np.uint32)
    return seqs, incs, stride


@pytest.fixture(scope="module")
def dev():
    import ccphylo_amd as cg
    with cg.Device(0) as d:
        yield d


@pytest.mark.parametrize("L", LENGTHS)
def test_meth_mask_equals_restatement(dev, L):
    rng = np.random.default_rng(L)
    tabs = tables()
    planted = 0
    for name in ("short", "long"):
        for n in TAXA:
            for pair in (False, True):
                for slack in (0, 2):
                    seqs, incs, stride = inputs(L, n, pair, slack, rng)
                    want, wcnt, wfound = expect(L, n, name, incs, pair, stride)
                    got, cnt, found = dev.meth_mask(seqs, incs, n, L, tabs[name], pair=pair)
                    key = (name, n, pair, slack)
                    assert found == wfound, key
                    assert (got == want).all(), key
                    assert (cnt == wcnt).all(), key
                    planted += found
    # rows 1 (ACGT repeats), 2 (all A) and 3 (GATC) hold planted sites wherever a motif fits
    assert planted > 0
    _, per = reference(L)
    if L >= 4:
        assert per["short"][1][2] == L - 1 and per["short"][1][3] > 0
    if L >= 31:
        assert per["long"][1][1] > 2 * (L - 1)     # the 31-mer on the ACGT repeats, beside nN at every start
    else:
        assert per["long"][1][1] == 2 * (L - 1)    # m > L matches nowhere: only nN and its other strand


def test_edges_padding_overlap_and_boundaries(dev):
    aA = mo.strands_of("aA")
    for codes, L, found, word0 in (([1, 1, 0], 3, 0, 0),                   # CCA + zero padding: no match
                                   ([0, 0, 0, 0], 4, 3, 0x70000000),       # AAAA: overlapping matches at 0, 1, 2
                                   ([0, 0], 2, 1, 0x40000000)):
        seqs = mo.pack(codes).reshape(1, -1)
        ones = np.full(L // 32 + 1, 0xFFFFFFFF, dtype=np.uint32)
        for pair in (False, True):
            got, cnt, f = dev.meth_mask(seqs, ones.reshape(1, -1) if pair else ones, 1, L, aA, pair=pair)
            assert f == found and int(got.ravel()[0]) == 0xFFFFFFFF & ~word0
            assert cnt[0] == npos(got.ravel(), 32)
    # a 32-mer from position 32 to 63 (row 1: ACGT from 0) and one from 1 to 32 (row 16: ACGT from 1);
    # GATC over the word boundary
    seqs0, per = reference(64)
    tab = mo.strands_of(ACGT8[:31] + "T")
    for t, must in ((1, (31, 63, 0, 32)), (16, (32, 1))):
        got, _, f = dev.meth_mask(seqs0[t:t + 1], np.full(3, 0xFFFFFFFF, np.uint32), 1, 64, tab)
        cl, wf = mo.sites(mo.unpack(seqs0[t], 64), tab)
        assert f == wf > 0 and (got == ~mo.to_words(cl, 3)).all() and all(cl[q] for q in must)
    g = mo.strands_of("gAtc")
    got, _, f = dev.meth_mask(seqs0[3:4], np.full(3, 0xFFFFFFFF, np.uint32), 1, 64, g)
    cl, wf = mo.sites(mo.unpack(seqs0[3], 64), g)
    assert f == wf >= 4 and (got == ~mo.to_words(cl, 3)).all() and cl[31] and cl[32] and cl[61] and cl[62]


@pytest.mark.parametrize("pair", [False, True], ids=["nonpair", "pair"])
def test_more_strands_than_a_batch_and_dev_form(dev, pair):
    L, n = 97, SLICE + 1
    rng = np.random.default_rng(9)
    tab = tables()["many"]
    seqs, incs, stride = inputs(L, n, pair, 2, rng)
    want, wcnt, wfound = expect(L, n, "many", incs, pair, stride)
    got, cnt, found = dev.meth_mask(seqs, incs, n, L, tab, pair=pair)
    assert found == wfound > 0 and (got == want).all() and (cnt == wcnt).all()
    ds, di = dev.malloc(seqs.nbytes), dev.malloc(incs.nbytes)
    try:
        dev.h2d(ds, seqs)
        dev.h2d(di, incs)
        cnt2, found2 = dev.meth_mask_dev(ds, di, n, L, stride, tab, pair=pair)
        back = np.zeros_like(incs)
        dev.d2h(back, di)
        assert found2 == wfound and (back == want).all() and (cnt2 == wcnt).all()
        # idempotent, and without outputs
        assert dev.meth_mask_dev(ds, di, n, L, stride, tab, pair=pair, want_counts=False) is None
        dev.sync()
        dev.d2h(back, di)
        assert (back == want).all()
    finally:
        dev.free(ds)
        dev.free(di)


def test_arguments(dev):
    import ctypes as C
    from ccphylo_amd import native
    seqs = np.zeros((2, 2), dtype=np.uint64)
    incs = np.full(2, 0xFFFFFFFF, dtype=np.uint32)
    ok = mo.strands_of("gAtc")
    # no strands, no taxa: nothing happens
    got, cnt, f = dev.meth_mask(seqs, incs, 2, 40, ok[:0])
    assert (got == incs).all() and f == 0
    got, cnt, f = dev.meth_mask(seqs[:0], incs, 0, 40, ok)
    assert (got == incs).all() and f == 0 and len(cnt) == 0
    bad = []
    for edit in ("len1", "len33", "empty", "wide", "meth"):
        t = ok.copy()
        if edit == "len1":
            t["len"][0] = 1
        elif edit == "len33":
            t["len"][1] = 33
        elif edit == "empty":
            t["allow"][0][2] = 0
        elif edit == "wide":
            t["allow"][1][0] = 16
        else:
            t["meth"][0] |= 0x80000000 >> 4
        bad.append(t)
    for t in bad:
        with pytest.raises(native.CcgError, match="invalid argument"):
            dev.meth_mask(seqs, incs, 2, 40, t)
    with pytest.raises(native.CcgError, match="invalid argument"):
        dev.meth_mask(seqs[:, :1], incs[:1], 2, 40, ok)      # stride below the data words


# ------------------------------------------------------------------ the CLI
def cli(args, cwd=METH):
    import ccphylo_amd as cg
    p = subprocess.run([cg.CLI_PATH] + args, cwd=cwd, capture_output=True, timeout=120)
    assert p.returncode == 0, (args, p.stderr.decode()[-2000:])
    return p


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_equals_reference_bytes(case):
    p = cli(case["args"])
    with open(os.path.join(METH, case["err"]), "rb") as f:
        assert p.stderr == f.read()
    with open(os.path.join(METH, case["out"]), "rb") as f:
        assert p.stdout == f.read()


def test_cli_long_option_and_plain_dist_unchanged():
    a = cli(["dist", "-i", "a8.fsa", "--methylation_motifs", "multi.fa"])
    b = cli(["dist", "-i", "a8.fsa", "-y", "multi.fa"])
    plain = cli(["dist", "-i", "a8.fsa"])
    assert a.stdout == b.stdout and a.stderr == b.stderr and plain.stdout != a.stdout


FUSED = [("a8.fsa", "multi.fa", []), ("b5.fsa", "dam.fa", ["-f", "3", "-L", "40"])]


@pytest.mark.parametrize("msa,motifs,opts", FUSED, ids=[f[0][:-4] + f[1][:-3] + "".join(f[2]) for f in FUSED])
def test_fused_tree_and_dbscan(tmp_path, msa, motifs, opts):
    phy, nwk, db = tmp_path / "d.phy", tmp_path / "fused.nwk", tmp_path / "fused.txt"
    d = cli(["dist", "-i", msa, "-y", motifs] + opts)
    phy.write_bytes(d.stdout)
    two_tree = cli(["tree", "-i", str(phy)]).stdout
    two_db = cli(["dbscan", "-i", str(phy), "-e", "8", "-N", "1"]).stdout
    f = cli(["dist", "-i", msa, "-y", motifs] + opts + ["--tree", str(nwk), "--dbscan", str(db), "--max_distance", "8",
                                                         "--min_neighbors", "1"])
    assert f.stdout == b"" and two_tree and two_db
    assert nwk.read_bytes() == two_tree
    assert db.read_bytes() == two_db
    # the same Included / Excluded lines as the unfused run
    assert f.stderr.startswith(d.stderr[:d.stderr.rfind(b"# Included")])
