"""GPU: a parsed value reaches the engine whichever way it is spelled.

The recorded corpus (test_cli_args.py) ends every case before a GPU is opened,
so it cannot see where a value lands.  Here one small run of each command is
spelled in its equivalent forms -- short options with separate and with
attached values, long options with separate values and with `=`, flags
clustered in front of a value option -- and every form must write the same
stdout bytes and the same bytes into every output file.  One process per form,
run serially; after a form that did not end with status 0 no further process
is started."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_broken = []   # the first form that failed: nothing more is started on the GPU after it

NAMES = ["tA", "tB", "tC", "tD", "tE"]


def phylip(names, D):
    rows = ["%10d" % len(names)]
    for i, nm in enumerate(names):
        rows.append(nm + "".join("\t%.6f" % D[i, j] for j in range(i)))
    return "\n".join(rows) + "\n"


def inputs():
    rng = np.random.default_rng(5)
    pts = rng.random((5, 3)) * 4
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    perm = [3, 0, 4, 1, 2]
    D2 = D + np.triu(rng.random((5, 5)) * 0.1, 1) + np.triu(rng.random((5, 5)) * 0.1, 1).T
    W = rng.integers(1, 50, (5, 5)).astype(float)
    W = np.triu(W, 1) + np.triu(W, 1).T
    msa = "".join(">s%d\n%s\n" % (i, "".join(rng.choice(list("ACGT"), 40))) for i in range(5))
    sub = [0, 1, 2, 3], [4, 2, 0]
    return {
        "m.phy": phylip(NAMES, D),
        "m2.phy": phylip([NAMES[k] for k in perm], D2[np.ix_(perm, perm)]),
        "msa.fsa": msa,
        "t.tsv": "".join("\t".join("%.3f" % v for v in row) + "\n" for row in rng.uniform(-2, 2, (5, 3))),
        "t.nwk": "(((tA:1.5,tB:2.5):0.5,tC:1.5):0.25,tD:1.25,tE:3.5);\n",
        "two.phy": "".join(phylip([NAMES[k] for k in s], D[np.ix_(s, s)]) for s in sub),
        "two_w.phy": "".join(phylip([NAMES[k] for k in s], W[np.ix_(s, s)]) for s in sub),
    }


def spell(opts, form):
    """opts: (letter or None, long name, value or None) in order; form 0..4"""
    words, flags = [], ""
    for letter, name, value in opts:
        short = letter is not None and form in (0, 1, 4)
        if value is None:
            if short and form == 4:
                flags += letter          # waits for the next short value option
            else:
                words.append("-" + letter if short else "--" + name)
        elif short:
            lead, flags = "-" + flags + letter, ""
            words += [lead + value] if form == 1 else [lead, value]
        else:
            words += ["--" + name + "=" + value] if form in (1, 3) else ["--" + name, value]
    return words + (["-" + flags] if flags else [])


H = ("H", "mmap", None)   # no effect on the result: something to cluster where the run has no flag of its own
RUNS = {
    "tree": ([("i", "input", "m.phy"), H, ("m", "method", "nj"), ("f", "flag", "1"), ("x", "print_precision", "5"),
              ("p", "float_precision", None), ("o", "output", "out.nwk")], ["out.nwk"], 5),
    "dbscan": ([("i", "input", "m.phy"), H, ("e", "max_distance", "2.5"), ("N", "min_neighbors", "2")], [], 5),
    "dist": ([("i", "input", "msa.fsa"), H, ("f", "flag", "1"), ("x", "print_precision", "5"),
              ("W", "normalization_weight", "1"), (None, "tree", "-"), (None, "tree_method", "nj"),
              (None, "tree_flag", "1")], [], 5),
    "tsv2phy": ([("i", "input", "t.tsv"), H, ("d", "distance", "l2"), ("x", "print_precision", "5"),
                 (None, "tree", "out.nwk"), ("o", "output", "out.phy")], ["out.nwk", "out.phy"], 5),
    "nwck2phy": ([("i", "input", "t.nwk"), H, ("x", "print_precision", "5")], [], 5),
    "phycmp": ([(None, "by_name", None), H, ("o", "output", "out.txt"), ("i", "input", "m.phy")], ["out.txt"], 5),
    # merge -H ends its short-option word, so nothing is clustered behind it there
    "merge": ([("i", "input", "two.phy"), ("w", "nucleotides_weights", "two_w.phy"), ("x", "print_precision", "5")],
              [], 4),
}


@pytest.mark.parametrize("cmd", list(RUNS))
def test_forms_write_the_same_bytes(cmd, tmp_path):
    import ccphylo_amd as cg
    assert not _broken, "not started: %r failed before" % (_broken[0],)
    opts, outfiles, nforms = RUNS[cmd]
    got = []
    for form in range(nforms):
        words = spell(opts, form) + (["m2.phy"] if cmd == "phycmp" else [])
        cwd = tmp_path / str(form)
        cwd.mkdir()
        for name, text in inputs().items():
            (cwd / name).write_text(text)
        try:
            p = subprocess.run([cg.CLI_PATH, cmd] + words, capture_output=True, timeout=60, cwd=cwd,
                               stdin=subprocess.DEVNULL)
            rc, err = p.returncode, p.stderr.decode()[-2000:]
        except subprocess.TimeoutExpired:
            rc, err = "timeout", ""
        if rc != 0:
            _broken.append((cmd, words, rc))
            pytest.fail("%s %s: status %s\n%s" % (cmd, words, rc, err))
        got.append((words, p.stdout, {f: (cwd / f).read_bytes() for f in outfiles}))
    assert len({tuple(g[0]) for g in got}) == nforms                  # the forms are different command lines
    assert got[0][1] or all(got[0][2].values()), "the run wrote nothing"
    assert all(v for v in got[0][2].values())
    for words, out, files in got[1:]:
        assert (out, files) == (got[0][1], got[0][2]), (got[0][0], words)


def test_the_forms_are_the_ones_named():
    opts = RUNS["tree"][0]
    assert spell(opts, 0) == ["-i", "m.phy", "-H", "-m", "nj", "-f", "1", "-x", "5", "-p", "-o", "out.nwk"]
    assert spell(opts, 1) == ["-im.phy", "-H", "-mnj", "-f1", "-x5", "-p", "-oout.nwk"]
    assert spell(opts, 2)[:5] == ["--input", "m.phy", "--mmap", "--method", "nj"]
    assert spell(opts, 3)[:3] == ["--input=m.phy", "--mmap", "--method=nj"]
    assert spell(opts, 4) == ["-i", "m.phy", "-Hm", "nj", "-f", "1", "-x", "5", "-po", "out.nwk"]
    assert spell(RUNS["dist"][0], 1)[-3:] == ["--tree=-", "--tree_method=nj", "--tree_flag=1"]
