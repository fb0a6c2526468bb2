"""`dist -y` on the CPU: tests/meth_oracle.py pinned to the reference's bytes
(tests/golden/meth), and the host layer (ccq_load_motifs, ccq_meth_clear_row,
the motif loaders and ccq_msa_meth_finish) equal to that restatement."""
import json
import os
import subprocess

import numpy as np
import pytest

import meth_oracle as mo
from conftest import GOLDEN

METH = os.path.join(GOLDEN, "meth")
with open(os.path.join(METH, "meth.json")) as _f:
    CASES = json.load(_f)["cases"]
MOTIF_FILES = ("dam.fa", "multi.fa", "multi.fa.gz")


def read(name):
    with open(os.path.join(METH, name), "rb") as f:
        return f.read()


# ------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_reference_bytes(case):
    out, err = mo.expected_cli(METH, case)
    assert err == read(case["err"])
    assert out == read(case["out"])


def test_golden_coverage():
    names = {c["name"] for c in CASES}
    assert len(CASES) >= 12 and any(c["motifs"].endswith(".gz") for c in CASES)
    # the first record goes by masking alone; a pair-mode record goes by masking alone
    assert b"# Excluded:\tdense0\t( 30 / 60 )\n# Included:\tr1" in read("b5_dam_L40.err")
    assert b"# Excluded:\tdense3\t( 32 / 60 )" in read("b5_dam_f3L40.err")
    assert {"a8_multi_f3n", "a8_multi_P5", "a8_multi_W1000p", "a8_multi_f11"} <= names


def test_strrc_is_the_reference_quirk():
    def rc(text):
        (_, q), = mo.motif_records(b">x\n" + text.encode())
        return mo.motif_text(mo.strrc(q))
    assert rc("gAtc") == "gaTc"          # even: the true reverse complement
    assert rc("Tag") == "gaA"            # odd: the middle stays, its left neighbour is the mirror uncomplemented
    assert rc("ccwgg") == "cgwgg"
    assert rc("gaNtc") == "gtNtc"
    assert rc("RRg") == "gRY"


# ------------------------------------------------------------------ ccq_load_motifs
def test_load_motifs_equals_restatement(tmp_path):
    from ccphylo_amd import native
    texts = {name: read(name) for name in MOTIF_FILES}
    texts["noise.fa"] = b">a b c\r\ng-A.t\nc 12\n>second\n\nacrykmRYKMSW\n>u\nuUaA"
    texts["nohdr.fa"] = b"gAtc\n>x\nccWgg"
    texts["len32.fa"] = b">long\n" + b"acgt" * 8 + b"\n"
    texts["widest.fa"] = b">w\nNNaNcgt\n>v\nacgtBDHV\n"
    for name, data in texts.items():
        p = tmp_path / name
        p.write_bytes(data)
        got = native.load_motifs(str(p))
        want = mo.strands(data)
        assert got.dtype == mo.MOTIF_DTYPE == native.MOTIF_DTYPE
        assert len(got) == len(want) == 2 * len(mo.motif_records(data)) and len(got) > 0, name
        assert got.tobytes() == want.tobytes(), name
    assert len(native.load_motifs(str(tmp_path / "multi.fa"))) == 8
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    assert len(native.load_motifs(str(empty))) == 0


REFUSED = [
    (b">dam\ngAtc\n>cc\ncCwgg\n", 'record 2 ("cc")', "narrower than its widest"),
    (b">deg\ngAnTc\n", 'record 1 ("deg")', "narrower than its widest"),
    (b">one\nA\n", 'record 1 ("one")', "has one base"),
    (b">ok\nag\n>none\n\n>x\nacg\n", 'record 2 ("none")', "has no bases"),
    (b">tail\n", 'record 1 ("tail")', "has no bases"),
    (b">long\n" + b"acgt" * 8 + b"a\n", 'record 1 ("long")', "longer than 32"),
]


@pytest.mark.parametrize("data,where,why", REFUSED, ids=[r[1].split('"')[1] for r in REFUSED])
def test_refusals_name_the_record(tmp_path, data, where, why):
    from ccphylo_amd import native
    with pytest.raises(mo.MotifRefused) as e:
        mo.strands(data)
    assert where in str(e.value) and why in str(e.value)
    p = tmp_path / "m.fa"
    p.write_bytes(data)
    with pytest.raises(native.CcgError) as e:
        native.load_motifs(str(p))
    assert where in str(e.value) and why in str(e.value)
    # the CLI ends before it opens a GPU, with the message
    r = subprocess.run([native.CLI_PATH, "dist", "-i", os.path.join(METH, "a8.fsa"), "-y", str(p)],
                       capture_output=True, timeout=60)
    assert r.returncode != 0 and r.stdout == b""
    assert where.encode() in r.stderr and why.encode() in r.stderr


def test_cli_refuses_missing_file_and_multi_file_input(tmp_path):
    from ccphylo_amd import native
    a8 = os.path.join(METH, "a8.fsa")
    r = subprocess.run([native.CLI_PATH, "dist", "-i", a8, "-y", str(tmp_path / "absent.fa")], capture_output=True,
                       timeout=60)
    assert r.returncode != 0 and b"cannot open" in r.stderr
    r = subprocess.run([native.CLI_PATH, "dist", "-y", os.path.join(METH, "dam.fa"), "-r", "t0", "-i", a8, a8],
                       capture_output=True, timeout=60)
    assert r.returncode != 0 and b"-y with several FASTA files" in r.stderr
    h = subprocess.run([native.CLI_PATH, "dist", "-h"], capture_output=True, timeout=60)
    assert b"methylation_motifs" in h.stdout and b"Mask methylation motifs from <file>" in h.stdout


# ------------------------------------------------------------------ ccq_meth_clear_row
def test_clear_row_equals_restatement():
    from ccphylo_amd import native
    rng = np.random.default_rng(5)
    tabs = [mo.strands(read("multi.fa")), mo.strands_of("aA"), mo.strands_of("acgtacgtacgtacgtacgtacgtacgtacgT", "Nn"),
            mo.strands_of("gAtc", "Tag", "ccWgg", "a" * 30 + "A")]
    total = 0
    for L in (2, 31, 32, 33, 63, 64, 65, 96, 97, 130, 257):
        for tab in tabs:
            codes = rng.integers(0, 4, L).astype(np.uint8) if L % 2 else rng.integers(0, 2, L).astype(np.uint8) * 3
            if L > 40:
                codes[L - 4:] = [2, 0, 3, 1]          # GATC ends exactly at L - 1
                codes[29:33] = [2, 0, 3, 1]           # ... and straddles words 0 / 1
            row = mo.pack(codes)
            clr, found = native.meth_clear_row(row, L, tab)
            cl, f = mo.sites(codes, tab)
            assert found == f
            assert (clr == mo.to_words(cl, L // 32 + 1)).all()
            total += f
    assert total > 100
    # the zero padding is `A` but completes no match; N columns (stored 00) match `a`; matches overlap
    aA = mo.strands_of("aA")
    clr, found = native.meth_clear_row(mo.pack([1, 1, 0]), 3, aA)      # C C A + padding
    assert found == 0 and not clr.any()
    clr, found = native.meth_clear_row(mo.pack([0, 0, 0, 0]), 4, aA)   # AAAA: aA at 0, 1, 2; tT nowhere
    assert found == 3 and clr[0] == 0x70000000


# ------------------------------------------------------------------ the loaders and ccq_msa_meth_finish
@pytest.mark.parametrize("threads", [0, 3])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_motif_loaders_equal_restatement(case, threads, tmp_path, monkeypatch):
    """The host side of `dist -y` end to end, the restatement standing in for
    the GPU step: rows, masks and the Included / Excluded lines in record order."""
    import conftest
    from ccphylo_amd import native
    o = conftest.parse_dist_args(case["args"])
    tab = mo.strands(read(case["motifs"]))
    want = mo.load_dist(read(case["input"]), tab, o["flag"], o["minLength"], o["minCov"], o["proxi"])
    steps = []

    def gpu_step(seqs, incs, n, length, pair):
        out, cnt, found = mo.mask_rows(seqs, incs, n, length, tab, pair)
        incs[...] = out
        steps.append(found)
        return cnt
    monkeypatch.setenv("CCQ_FASTA_WINDOW", "700")   # the parallel loader: several windows
    log = tmp_path / "log"
    heads, seqs, incs, L, ml = native.load_msa(os.path.join(METH, case["input"]), o["flag"], o["minLength"],
                                               o["minCov"], o["proxi"], threads=threads, log_path=str(log),
                                               motifs=native.load_motifs(os.path.join(METH, case["motifs"])),
                                               mask_fn=gpu_step)
    assert steps and steps[0] > 0
    assert heads == want["headers"] and L == want["len"] and ml == want["minLength"]
    assert (seqs == want["seqs"]).all() and (incs == want["incs"]).all()
    assert log.read_text() == want["log"]
    assert log.read_bytes() == read(case["err"])[:len(want["log"])]


def test_loaders_without_motifs_are_unchanged(tmp_path):
    from ccphylo_amd import native
    path = os.path.join(METH, "b5.fsa")
    for flag in (1, 3):
        for threads in (0, 3):
            a = native.load_msa(path, flag, 40, threads=threads, log_path=str(tmp_path / "a"))
            b = native.load_msa(path, flag, 40, threads=threads, log_path=str(tmp_path / "b"),
                                motifs=np.zeros(0, native.MOTIF_DTYPE), mask_fn=lambda *x: 1 / 0)
            assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[3:] == b[3:]
            assert (tmp_path / "a").read_bytes() == (tmp_path / "b").read_bytes()
