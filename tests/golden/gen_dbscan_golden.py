#!/usr/bin/env python3
"""Generates the golden vectors of `ccphylo dbscan` by running the REFERENCE
binary built by oracle/Makefile (oracle/_ref/ccphylo) on Phylip inputs that
gen_golden.py committed (no new inputs):

    python __graft_entry__.py && python tests/golden/gen_dbscan_golden.py

Outputs (data, committed): dbscan/dbscan.json lists the cases with their
command lines, md5 and what they cover; dbscan/*.out are the reference's
stdout.  Per input, -e is the first of the matrix's own distance quantiles
(QUANTILES, in that order) at which the case's -N leaves more than one cluster
and fewer than n; the two deliberate extremes (one cluster, n singletons) are
marked "extreme".  The generator checks the coverage the tests rely on (border
rows attached to a cluster and left alone, missing cells as neighbours) with
tests/dbscan_oracle.py, whose result it also compares with every output."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
OUT = os.path.join(HERE, "dbscan")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
QUANTILES = (0.01, 0.03, 0.1, 0.3, 0.6)

# (name, input, precision options, -N)
PLAN = [
    ("test", "test.phy.gz", [], 1), ("test_N2", "test.phy.gz", [], 2), ("test_p_N4", "test.phy.gz", ["-p"], 4),
    ("test_s100", "test.phy.gz", ["-s", "100"], 2),
    ("snp300", "snp300.phy", [], 1), ("snp300_N4", "snp300.phy", [], 4), ("snp300_b_N2", "snp300.phy", ["-b"], 2),
    ("snp300_s100_N4", "snp300.phy", ["-s", "100"], 4),
    ("miss80", "miss80.phy", [], 1), ("miss80_N4", "miss80.phy", [], 4), ("miss80_p_N2", "miss80.phy", ["-p"], 2),
    ("multi", "multi.phy", [], 1), ("multi_N2", "multi.phy", [], 2),
    ("euc400", "euc400.phy.gz", [], 1), ("euc400_p_N4", "euc400.phy.gz", ["-p"], 4),
    ("adv_line_N2", "adv_line.phy.gz", [], 2), ("adv_line_N4", "adv_line.phy.gz", [], 4),
    ("adv_dupes", "adv_dupes.phy.gz", [], 1), ("adv_dupes_N4", "adv_dupes.phy.gz", [], 4),
    ("adv_grid_N2", "adv_grid.phy.gz", [], 2), ("adv_grid_b_N4", "adv_grid.phy.gz", ["-b"], 4),
]
# the extremes: everything within reach (one cluster), nothing within reach (n singletons)
EXTREMES = [("snp300_all", "snp300.phy", [], 1, "1e9"), ("snp300_none", "snp300.phy", [], 1, "-2")]


def etype_of(opts):
    if "-p" in opts:
        return 4, 1.0
    for o, et in (("-s", 2), ("-b", 1)):
        if o in opts:
            k = opts.index(o)
            return et, float(opts[k + 1]) if k + 1 < len(opts) else 1.0
    return 8, 1.0


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle all")
    from ccphylo_amd import native
    import dbscan_oracle
    os.makedirs(OUT, exist_ok=True)
    os.chdir(HERE)
    cases = []
    for name, inp, opts, minn, *fixed in PLAN + EXTREMES:
        et, bs = etype_of(opts)
        mats = native.load_phylip(os.path.join(HERE, inp), etype=et, byte_scale=bs)
        d0 = dbscan_oracle.cells_as_double(mats[0][1], et, bs)
        if fixed:
            cands = [fixed[0]]
        else:
            cands = ["%.6g" % q for q in np.quantile(d0[d0 >= 0], QUANTILES)]
        for e in cands:
            res = [dbscan_oracle.dbscan(D, len(nm), float(e), minn, et, bs) for nm, D in mats]
            if fixed or all(1 < r[2] < len(nm) for r, (nm, _) in zip(res, mats)):
                break
        else:
            sys.exit(f"{name}: no quantile of {QUANTILES} gives 1 < nClust < n")
        args = ["dbscan", "-i", inp, "-e", e, "-N", str(minn)] + opts
        p = subprocess.run([REF] + args, capture_output=True, check=True)
        blocks = dbscan_oracle.parse_table(p.stdout)
        assert len(blocks) == len(mats), name
        attached = alone = 0
        miss_nb = False
        for (hdr, n, nclust, names, N, C), r, (nm, D) in zip(blocks, res, mats):
            assert n == len(nm) and names == nm, name
            assert (N == r[0]).all() and (C == r[1]).all() and nclust == r[2], f"{name}: restatement differs"
            assert fixed or 1 < nclust < n, name
            N, C = np.array(N), np.array(C)
            b = (N > 0) & (N < minn)
            attached += int((b & (C != np.arange(n))).sum())
            alone += int((b & (C == np.arange(n))).sum())
            d = dbscan_oracle.cells_as_double(D, et, bs)
            miss_nb |= bool(((d == -1) & (d <= float(e))).any())
        with open(os.path.join(OUT, name + ".out"), "wb") as f:
            f.write(p.stdout)
        cases.append({"name": name, "input": inp, "args": args, "out": name + ".out",
                      "md5": hashlib.md5(p.stdout).hexdigest(), "n": [b[1] for b in blocks],
                      "nclust": [b[2] for b in blocks], "border_attached": attached, "border_alone": alone,
                      "missing_neighbours": miss_nb, "extreme": bool(fixed)})
    ext = {c["name"]: c for c in cases if c["extreme"]}
    assert ext["snp300_all"]["nclust"] == [1] and ext["snp300_none"]["nclust"] == ext["snp300_none"]["n"]
    withb = [c for c in cases if c["border_attached"] + c["border_alone"]]
    assert len(withb) >= 4 and any(c["border_attached"] for c in withb) and any(c["border_alone"] for c in withb)
    assert any(c["missing_neighbours"] for c in cases)
    with open(os.path.join(OUT, "dbscan.json"), "w") as f:   # one case per line
        f.write('{"reference": "ccphylo 0.8.5 (oracle/_ref/ccphylo, built by oracle/Makefile)", "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print(f"{len(cases)} golden cases, {len(withb)} with border rows")
    for c in cases:
        print(c["name"], c["args"][3:], c["n"], c["nclust"], c["border_attached"], c["border_alone"],
              c["missing_neighbours"], os.path.getsize(os.path.join(OUT, c["out"])))


if __name__ == "__main__":
    main()
