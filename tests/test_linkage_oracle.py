"""CPU: the serial restatement of upgma / cf / ff / mn (tests/linkage_oracle.c)
reproduces the reference binary: its committed golden vectors
(tests/golden/golden_linkage.json) and, where the binary is built
(oracle/_ref/ccphylo), live runs on larger generated matrices.  The
restatement is then the arbiter of the GPU tests (tests/test_gpu_linkage.py),
which need whole join records where Newick at -x 9 pins nine decimals, and
tie-heavy inputs on which the binary's own Newick assembly aborts."""
import os
import subprocess

import numpy as np
import pytest

import linkage_oracle as lo
from conftest import ROOT
from test_gpu import _clade_ltd, _euclid, _missing_ltd   # the GPU suite's matrix recipes (plain numpy)

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ccphylo")


def restated_newick(path, method, et=8, bs=1.0, flags=0, prec=9):
    import ccphylo_amd as cg
    trees = cg.newick_from_phylip(path, lambda D, n: lo.tree(D, n, etype=et, byte_scale=bs, method=method, flags=flags),
                                  etype=et, byte_scale=bs, flags=flags, precision=prec)
    return ("\n".join(trees) + "\n").encode()


@pytest.mark.parametrize("case", lo.linkage_cases(), ids=lambda c: c["name"])
def test_restatement_matches_golden(case):
    path, method, et, bs, flags, prec = lo.parse_tree_args(case["args"])
    assert restated_newick(path, method, et, bs, flags, prec) == lo.golden_out(case)


def _all200(n):
    return np.full(n * (n - 1) // 2, 200.0)


LIVE = ([("mn", "euc", 1500)] + [(m, "euc", 2500) for m in ("upgma", "cf", "ff")] +
        [(m, "miss", n) for m in ("upgma", "ff", "mn") for n in (400, 1100)] +
        [(m, "all200", 300) for m in ("upgma", "cf", "ff", "mn")])


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="the reference binary is not built (oracle/_ref/ccphylo)")
@pytest.mark.parametrize("method,kind,n", LIVE)
def test_restatement_matches_live_binary(tmp_path, method, kind, n):
    D = _euclid(n, n) if kind == "euc" else _missing_ltd(n, n) if kind == "miss" else _all200(n)
    path = str(tmp_path / "in.phy")
    lo.write_phylip(path, D, n)
    p = subprocess.run([REF_BIN, "tree", "-i", path, "-m", method], capture_output=True, timeout=600)
    assert p.returncode == 0 and p.stdout, p.stderr.decode()[-2000:]
    assert restated_newick(path, lo.METHODS[method]) == p.stdout


def test_restatement_prefix_and_stats():
    """max_joins gives a prefix of the full run; UPGMApair rescans bounded rows on a tie-heavy matrix."""
    n = 400
    D = _clade_ltd(n, 3)
    for m in (lo.UPGMA, lo.FF):
        full = lo.tree(D, n, method=m, stats=True)
        pre = lo.tree(D, n, method=m, max_joins=50)
        assert len(pre[0]) == 50 and (pre[0] == full[0][:50]).all()
        assert full[3][0] > 0 and full[3][1] > 0
