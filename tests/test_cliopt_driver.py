"""host/cliopt.c under AddressSanitizer and UBSan, on the host.

tests/cliopt_driver.c is a stand-alone program with one option row of every
kind.  It is built here with -fsanitize=address,undefined and run over the argv
lists of the recorded corpus (command names stripped, so most words are unknown
to it: the walk still has to be clean) and over the degenerate lists; then a
few equivalent spellings must print the same struct."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ccphylo_amd", "host")
CASES = os.path.join(ROOT, "tests", "golden", "cli", "cases.json")
ENV = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cliopt") / "cliopt_driver")
    subprocess.run(["gcc", "-std=gnu11", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "cliopt_driver.c"),
                    os.path.join(HOST, "cliopt.c")], check=True)
    return exe


def run(exe, mode, words):
    p = subprocess.run([exe, mode] + words, capture_output=True, stdin=subprocess.DEVNULL, env=ENV, timeout=60)
    return p.returncode, p.stdout, p.stderr


def test_walk_is_clean_over_the_corpus_and_the_degenerate_lists(driver):
    with open(CASES) as f:
        lists = {tuple(c["argv"][1:]) for c in json.load(f)["cases"]}
    lists |= {(), ("-",), ("-", "a", "b"), ("-x" + "9" * 4096,), ("--" + "n" * 4096 + "=1",), ("--=x",), ("--",),
              ("-" + "p" * 4096,), ("--int=" + "7" * 4096,), ("-i",), ("-I",), ("-i", "-"), ("--list=",), ("--need=",),
              ("", ""), ("-s", ""), ("-x", ""), ("-S", "")}
    jobs = [(m, list(w)) for w in sorted(lists) for m in "sl"]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:
        got = list(pool.map(lambda j: run(driver, *j), jobs))
    bad = [(j, g) for j, g in zip(jobs, got)
           if g[0] not in (0, 1) or b"Sanitizer" in g[2] or b"runtime error" in g[2]]
    assert not bad, bad[:3]


def test_equivalent_spellings_store_the_same(driver):
    def same(*forms):
        outs = [run(driver, "s", list(f)) for f in forms]
        assert outs[0][0] == 0 and all(o == outs[0] for o in outs), (forms, outs)
        return outs[0][1].decode()

    assert "num=5 " in same(("-x", "5"), ("-x5",), ("--int", "5"), ("--int=5",), ("--int=", "5"), ("-gx5",))
    assert "flag=4 " in same(("-p",), ("--flag",), ("-gp",), ("-pg",), ("--flag=1",))
    assert "flag=0 " in same(("-Gp",), ("--ignore_end",), ("-G",))             # the word ends at -G
    assert "prec=2/0.01" in same(("-s", "1e-2"), ("-s1e-2",), ("--prec=1e-2",), ("--prec", "1e-2"), ("-gs", "1e-2"))
    assert "prec=2/1\n" in same(("-s",), ("--prec",), ("-s", "-g"), ("--prec=", "-g"))
    assert "unset=[(null)]" in same(("-U",), ("--unset",), ("-gU",))
    assert "unsup=[a]" in same(("-a", "v"), ("-av",), ("-ga", "v"))
    assert "unsup=[unsup]" in same(("--unsup", "v"), ("--unsup=v",))
    assert "pick=2 " in same(("--pick", "two"), ("--pick=two",))
    assert "list=2 [a] [b]" in same(("-i", "a", "b"), ("-ia", "b"), ("--list=a", "b"), ("--list", "a", "b", "-g"))
    assert "need=2 [a] [-]" in same(("-I", "a", "-"), ("-Ia", "-"), ("--need=", "a", "-"), ("-gI", "a", "-", "-g"))
    assert "rest=[in]" in same(("in",), ("-g", "in"), ("--", "in"), ("--=x", "in"))
    assert "ch=44 " in same(("-S", ","), ("-S,",), ("--char=,x",))
    assert "pct=0.25 " in same(("-C", "25"), ("--pct=25",)) and "udbl=3 " in same(("-E", "3.9"), ("--udbl=3.9",))
    for words, msg in ((("-x",), b'Missing argument:\t"x"\n'), (("--int",), b'Missing argument:\t"int"\n'),
                       (("--int=zz",), b'Invalid argument:\t"int"\n'), (("-gxzz",), b'Invalid argument:\t"x"\n'),
                       (("-t", "1x"), b'Invalid argument:\t"t"\n'), (("-e", "1x"), b'Invalid argument:\t"e"\n'),
                       (("-sx",), b'Invalid argument:\t"s"\n'), (("--pick", "three"), b'Invalid argument:\t""--pick""\n'),
                       (("-I",), b'Missing argument:\t"need"\n'), (("-gZ",), b'Unknown argument:\t"-Z"\n'),
                       (("--nope=1",), b'Unknown argument:\t"--nope"\n'),
                       (("a", "b"), b"Unexpected non-option argument(s).\n")):
        assert run(driver, "s", list(words)) == (1, b"", msg), words
    assert run(driver, "l", ["--"]) == (1, b"", b'Unknown argument or option: "--"\n')
    assert b"list=3 [a] [-b] [c]" in run(driver, "l", ["a", "-b", "c"])[1]
    rc, out, err = run(driver, "s", ["-gh"])
    assert rc == 0 and err == b"" and out.count(b"\n") == 2 + 17 and b"unsup" not in out
