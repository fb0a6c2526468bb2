"""CPU: the table reader and writer of `ccphylo tsv2phy` (ccq_load_tsv /
ccq_print_tsvphy, ccphylo_amd/host/tsv.c) against tests/tsv_oracle.py and the
reference's rules (tsv.c:30 loadTsv), and the CLI's exits that need no GPU:
every refusal of the loader ends with status 1 before a device is opened, an
input without rows prints the reference's message and ends with 0, and a
one-row table has no cell to compute."""
import os
import subprocess

import numpy as np
import pytest

import tsv_oracle as tso
from tsv_oracle import CASES, TSV

INPUTS = sorted({(c["input"], "," if c["input"].endswith(".csv") else "\t") for c in CASES})


def run(args, cwd=TSV, data=None):
    import ccphylo_amd as cg
    return subprocess.run([cg.CLI_PATH, "tsv2phy"] + args, cwd=cwd, input=data, capture_output=True, timeout=60)


@pytest.mark.parametrize("inp,sep", INPUTS, ids=[i for i, _ in INPUTS])
@pytest.mark.parametrize("vtype", [8, 4])
def test_load_tsv_matches_restatement(inp, sep, vtype):
    import ccphylo_amd as cg
    X = cg.load_tsv(os.path.join(TSV, inp), sep, vtype)
    R = tso.read_tsv(os.path.join(TSV, inp), sep, vtype)
    assert X.dtype == R.dtype and X.shape == R.shape
    assert np.array_equal(X, R)


def test_shapes_of_the_inputs():
    import ccphylo_amd as cg
    shapes = {i: cg.load_tsv(os.path.join(TSV, i), s).shape for i, s in INPUTS}
    assert shapes["mix12.tsv"] == shapes["mix12.tsv.gz"] == (12, 37)
    assert shapes["hash9.tsv"] == (9, 4) and shapes["col1.tsv"] == (9, 1)
    assert shapes["one.tsv"] == (1, 6) and shapes["two.tsv"] == (2, 6) and shapes["comma12.csv"] == (12, 5)


def test_strtod_forms_and_empty_entries(tmp_path):
    """hex floats, exponents, leading blanks and an empty entry (strtod("") = 0) are read as the reference reads them;
    the column count ignores a separator in the header's first byte."""
    import ccphylo_amd as cg
    p = tmp_path / "t.tsv"
    p.write_text("\ta\tb\tc\n0x1p-3\t 2.5e1\t\n-.5\t+7\t1e-320\n")
    X = cg.load_tsv(str(p))
    assert X.tolist() == [[0.125, 25.0, 0.0], [-0.5, 7.0, 1e-320]]
    p.write_text("h\n1\n\n3\n")   # n = 1: an empty line is a row of 0
    assert cg.load_tsv(str(p)).tolist() == [[1.0], [0.0], [3.0]]


BAD = [
    ("long", "a\tb\n1\t" + "1" * 32 + "\n", "Malformatted entry at pos:\t(0,2)"),
    ("garbage", "a\tb\n1\t2\n3x\t4\n", "Malformatted entry at pos:\t(1,1) 3x"),
    ("no_newline", "a\tb\n1\t2\n3\t4", "Unexpected end of file"),
    ("short_row", "a\tb\n1\t2\n3\n", "Unexpected end of file"),
    ("nan", "a\tb\n1\tnan\n", "Non-finite entry at pos:\t(0,2) nan"),
    ("inf", "a\tb\n-inf\t1\n", "Non-finite entry at pos:\t(0,1) -inf"),
    ("overflow", "a\tb\n1e999\t1\n", "Non-finite entry"),
]


@pytest.mark.parametrize("name,text,msg", BAD, ids=[b[0] for b in BAD])
def test_refusals_exit_1(tmp_path, name, text, msg):
    import ccphylo_amd as cg
    p = tmp_path / "bad.tsv"
    p.write_text(text)
    r = run(["-i", str(p)])
    assert r.returncode == 1 and r.stdout == b"" and msg.encode() in r.stderr, r.stderr
    with pytest.raises(ValueError, match=msg.split("\t")[0]):
        cg.load_tsv(str(p))


def test_31_byte_entry_is_read(tmp_path):
    import ccphylo_amd as cg
    p = tmp_path / "t.tsv"
    p.write_text("a\n" + "1" + "0" * 30 + "\n")
    assert cg.load_tsv(str(p)).tolist() == [[1e30]]


def test_float_overflow_is_refused_only_with_p(tmp_path):
    import ccphylo_amd as cg
    p = tmp_path / "t.tsv"
    p.write_text("a\n1e39\n")
    assert cg.load_tsv(str(p), vtype=8).tolist() == [[1e39]]
    with pytest.raises(ValueError, match="Non-finite"):
        cg.load_tsv(str(p), vtype=4)


@pytest.mark.parametrize("text", ["", "header only\n", "h\n#c\n"], ids=["empty", "header", "hash"])
def test_zero_rows_message(tmp_path, text):
    import ccphylo_amd as cg
    p = tmp_path / "e.tsv"
    p.write_text(text)
    r = run(["-i", str(p)])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b"Input matrix contained zero rows.\n"
    assert cg.load_tsv(str(p)).shape[0] == 0
    r = run([], data=text.encode())   # stdin is the default input
    assert r.returncode == 0 and r.stderr == b"Input matrix contained zero rows.\n"


def test_one_row_table_needs_no_gpu():
    case = next(c for c in CASES if c["name"] == "cos_one")
    r = run(case["args"][1:])
    with open(os.path.join(TSV, case["out"]), "rb") as f:
        assert r.returncode == 0 and r.stdout == f.read() == b"         1\n0\n"


def test_writer_matches_restatement(tmp_path):
    import ccphylo_amd as cg
    rng = np.random.default_rng(3)
    for m in (1, 2, 7):
        D = rng.normal(size=m * (m - 1) // 2) * 10.0 ** rng.integers(-8, 8, m * (m - 1) // 2)
        for flag, prec in ((1, 9), (0, 9), (1, 17), (0, 3)):
            path = str(tmp_path / "o.phy")
            cg.write_tsvphy(path, D, m, flag, prec)
            with open(path, "rb") as f:
                assert f.read() == tso.format_phy(D, m, flag, prec)
    cg.write_tsvphy(path, D.astype(np.float32), m, 1, 9, etype=4)
    with open(path, "rb") as f:
        assert f.read() == tso.format_phy(D.astype(np.float32).astype(np.float64), m, 1, 9)


def test_help_texts_match_the_reference():
    """-h, -D and -F print the reference's bytes (tsv2phy.c:117-135, :296-315); tsv2phy is in the top-level help."""
    import ccphylo_amd as cg
    h = run(["-h"])
    assert h.returncode == 0 and h.stdout.startswith(b"#CCPhylo tsv2phy converts tsv files to phylip distance files.\n")
    assert h.stdout.count(b"\n") == 16 and b"#    -d, --distance        \tDistance method" in h.stdout
    assert run(["--help"]).stdout == h.stdout
    d = run(["-D"])
    assert d.returncode == 0 and d.stdout.startswith(b"# Distance calculation methods:\n#\n# cos:\tCalculate cosine")
    assert d.stdout.endswith(b"# p:\tCalculate Pearsons correlation between vectors.\n#\n") and d.stdout.count(b"\n") == 9
    assert run(["--distance_help"]).stdout == d.stdout
    f = run(["-F"])
    assert f.stdout == b"Format flags output format, add them to combine them.\n#\n# 1:\tRelaxed Phylip\n#\n"
    assert run(["--flag_help"]).stdout == f.stdout
    top = subprocess.run([cg.CLI_PATH, "--help"], capture_output=True, timeout=60)
    assert b"tsv2phy" in top.stdout


REFUSED = [
    (["-s"], b"not supported"), (["-b"], b"not supported"), (["-s", "100"], b"not supported"),
    (["--byte_precision"], b"not supported"),
    (["-d", "euclid"], b"Invalid value parsed at \"--distance\".\n"),
    (["-d", "lx"], b"Invalid value parsed at \"--distance ln\".\n"),
    (["-d", "l0"], b"must be finite and > 0"), (["-d", "l-2"], b"must be finite and > 0"),
    (["-q"], b"Unknown argument or option: \"-q\"\n"),
]


@pytest.mark.parametrize("opts,msg", REFUSED, ids=["_".join(o) for o, _ in REFUSED])
def test_cli_refusals(opts, msg):
    r = run(["-i", "mix12.tsv"] + opts)
    assert r.returncode != 0 and r.stdout == b"" and msg in r.stderr, r.stderr
