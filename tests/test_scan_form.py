"""The DNJ scan-form resolver (dnj_scan_form, ccphylo_amd/csrc/ccg_dnj_form.h)
against tests/golden/scan_forms.txt: which rescan kernel, grid, pruning,
helper blocks, k_dnj_sphase and k_dnj_fold a join gets for a given matrix
size, element type and CCG_* setting.

The header is host-only, so this needs no GPU: tests/scan_form_rows.cpp is
compiled against it with the host compiler on first use, into a temporary
directory.  The table holds the defaults at every (n, et, gen, have_lbm) of
interest, every setting the GPU tests run the tree engines with, and the
retired CCG_SCAN_WAVE values, which must resolve as their base values
(5-8 and 10-19 as 4; 22 and 23 as 20).
"""
import atexit
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ccphylo_amd", "csrc")
_exe = None


def resolver():
    global _exe
    if _exe is None:
        tmp = tempfile.mkdtemp(prefix="scan_form_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        exe = os.path.join(tmp, "scan_form_rows")
        subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                        "-o", exe, os.path.join(HERE, "scan_form_rows.cpp")], check=True)
        _exe = exe
    return _exe


def resolve(keys):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CCG_")}
    out = subprocess.run([resolver()], input="\n".join(keys) + "\n", capture_output=True, text=True, check=True, env=env)
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "scan_forms.txt")) as f:
        rows = [ln.rstrip("\n").split(" | ") for ln in f if ln.strip() and not ln.startswith("#")]
    keys = [k for k, _ in rows]
    assert len(set(keys)) == len(keys)
    return keys, [w for _, w in rows], resolve(keys)


def test_scan_form_table(table):
    """Every row of the table resolves to the recorded form."""
    keys, want, got = table
    assert len(got) == len(keys) > 300
    wrong = [(k, w, g) for k, w, g in zip(keys, want, got) if w != g]
    assert not wrong, "%d rows differ, the first: %s\n  want %s\n  got  %s" % ((len(wrong),) + wrong[0])


def test_scan_form_defaults(table):
    """The defaults the comments promise: the block scan up to 16384 taxa;
    past it double rows stream through the 16-byte wave scan and narrower
    rows go in (4, 8) row groups, both compacted and pruned through
    k_dnj_sphase with the plan's 256 helper blocks -- or, under the block
    lower bounds, the bounded 16-byte wave scan for every element type."""
    keys, _, got = table
    form = dict(zip(keys, (dict(kv.split("=") for kv in g.split()) for g in got)))
    for et in (8, 4, 2, 1):
        for n in (3000, 16384):
            f = form[f"0 {n} {et} 0 0 1 0"]
            assert (f["kernel"], f["prune"], f["sphase"], f["fold"], f["launches"]) == ("block", "0", "none", "1", "2")
        for n in (16385, 40000, 140000):
            f = form[f"0 {n} {et} 0 0 1 0"]
            assert (f["prune"], f["cmp"], f["helpers"], f["sphase"], f["sfold"], f["launches"]) == \
                ("2", "1", "256", "compact", "1", "3")
            assert (f["kernel"], f["stream"], f["G"], f["UC"]) == \
                (("wave16", "1", "0", "0") if et == 8 else ("group_cmp", "0", "4", "8"))
            assert f["grid"] == "1024"
            b = form[f"0 {n} {et} 0 1 1 0"]
            assert (b["kernel"], b["stream"], b["lb"], b["cmp"], b["prune"]) == ("wave16", "0", "1", "1", "2")
            g = form[f"0 {n} {et} 1 1 1 0"]   # missing entries: the wave scan, nothing else
            assert (g["kernel"], g["prune"], g["cmp"], g["lb"]) == ("wave", "0", "0", "0")


def test_scan_form_retired_values():
    """Every retired CCG_SCAN_WAVE value gives its base value's form, in both
    engines, at a small and a large n, with and without the bounds."""
    base = {**{w: 4 for w in (5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19)}, 22: 20, 23: 20}
    tail = "CCG_PREFOLD_N=0 CCG_SEG_MUL=1 CCG_S_SPLIT_N=100 CCG_PRUNE_CELLS=0"
    heads = [f"{sh} {n} {et} 0 {lbm} 1 0" for sh in (0, 1) for n in (2500, 40000) for et in (8, 4) for lbm in (0, 1)]
    ws = sorted(base)
    got = resolve([f"{h} CCG_SCAN_WAVE={w} {tail}" for w in ws for h in heads])
    ref = dict(zip(((b, h) for b in (4, 20) for h in heads),
                   resolve([f"{h} CCG_SCAN_WAVE={b} {tail}" for b in (4, 20) for h in heads])))
    k = 0
    for w in ws:
        for h in heads:
            assert got[k] == ref[(base[w], h)], (w, h)
            k += 1
