"""The argument surface of the command line, replayed from a recorded corpus.

tests/golden/cli/cases.json (tests/golden/gen_cli_golden.py) holds, for every
case, the argv, stdin and working-directory files, and the exit status, stdout
and stderr of the binary it was recorded from.  Every case ends before a GPU is
opened, so this runs anywhere; all three outputs are compared byte for byte."""
import base64
import json
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ccphylo_amd", "bin", "ccphylo")
CASES = os.path.join(ROOT, "tests", "golden", "cli", "cases.json")
COMMANDS = ("tree", "dbscan", "dist", "tsv2phy", "nwck2phy", "phycmp", "merge")


def dec(v):
    return v.encode("utf-8") if isinstance(v, str) else base64.b64decode(v["b64"])


def replay(case):
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in case["files"].items():
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        p = subprocess.run([BIN] + case["argv"], input=case["stdin"].encode(), capture_output=True, cwd=tmp,
                           timeout=60)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def corpus():
    with open(CASES) as f:
        doc = json.load(f)
    texts = [dec(t) for t in doc["texts"]]   # each distinct output is stored once
    return [dict(c, stdin=c.get("stdin", ""), files=c.get("files", {}), stdout=texts[c["stdout"]],
                 stderr=texts[c["stderr"]]) for c in doc["cases"]]


def test_corpus_covers_every_command(corpus):
    assert len(corpus) >= 250
    for cmd in COMMANDS:
        assert sum(1 for c in corpus if c["argv"][:1] == [cmd]) >= 25, cmd
        h = [c["stdout"] for c in corpus if c["argv"] in ([cmd, "-h"], [cmd, "--help"])]
        assert len(h) == 2 and h[0] == h[1] and h[0], cmd
    assert not any(b"cannot open GPU" in c["stderr"] for c in corpus)


def test_every_case_replays_byte_for_byte(corpus):
    assert os.path.exists(BIN), "bin/ccphylo is not built"
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:   # the cases are independent processes in their own directories
        got = list(pool.map(replay, corpus))
    bad = []
    for c, (rc, out, err) in zip(corpus, got):
        want = (c["rc"], c["stdout"], c["stderr"])
        if (rc, out, err) != want:
            bad.append((c["argv"], want, (rc, out, err)))
    assert not bad, "%d of %d cases differ; the first:\n%r" % (len(bad), len(corpus), bad[:3])
