#!/usr/bin/env python3
"""Generates the golden vectors of `ccphylo tsv2phy` by running the REFERENCE
binary built by oracle/Makefile (oracle/_ref/ccphylo), on the CPU:

    python __graft_entry__.py && python tests/golden/gen_tsv_golden.py

Outputs (data, committed) under tsv/: the input tables, the reference's
stdout per case, and tsv.json listing {name, input, args, out} (tree cases:
the Newick of `tsv2phy -x 17 ... | tree -m M`, with the method in "tree").

Tables (three decimals per entry, so the float rows of -p differ from the
double ones):
  mix12   12 x 37, signed; row 11 repeats row 0, row 1 is all zero (cos -> -1,
          p -> 0), row 2 is constant (p -> 0)
  pos12   the same shape, non-negative (chi2, bc)
  tree30  30 x 12, strictly positive and without special rows: every cos and
          l2 cell is >= 0 (the fused --tree cases)
  comma12 12 x 5 with ',' separators; hash9 9 x 4 with '#' lines after the
  header; one / two: one and two rows; col1: 9 x 1 (n = 1)
The generator checks every -x 17 output of a bit-exact metric against
tests/tsv_oracle.py before it writes anything."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
OUT = os.path.join(HERE, "tsv")
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALL = ("cos", "chi2", "bc", "l1", "l2", "linf", "l3", "l2.5", "p")


def table(rng, m, n, lo, hi, special=True):
    X = np.round(rng.uniform(lo, hi, size=(m, n)), 3)
    if special:
        X[m - 1] = X[0]
        X[1] = 0
        X[2] = 1.25
    return X


def write_table(name, X, sep="\t", hashes=0, gz=False):
    lines = [sep.join("c%d" % k for k in range(X.shape[1]))]
    lines += ["#comment line %d%s with%sseparators" % (k, sep, sep) for k in range(hashes)]
    if hashes:   # the column count comes from the LAST dropped line
        lines[-1] = "#" + sep.join("h%d" % k for k in range(X.shape[1]))
    lines += [sep.join("%.3f" % v for v in row) for row in X]
    data = ("\n".join(lines) + "\n").encode()
    path = os.path.join(OUT, name)
    if gz:
        with open(path, "wb") as f:
            f.write(gzip.compress(data, mtime=0))
    else:
        with open(path, "wb") as f:
            f.write(data)


def plan():
    cases = []
    for d in ALL:
        inp = "pos12.tsv" if d in ("chi2", "bc") else "mix12.tsv"
        tag = d.replace(".", "_")
        cases.append((f"{tag}_x17", inp, ["-d", d, "-x", "17"]))
        cases.append((f"{tag}_p_x17", inp, ["-d", d, "-p", "-x", "17"]))
    cases += [
        ("cos_default", "mix12.tsv", []),
        ("l2_p_default", "mix12.tsv", ["-d", "l2", "-p"]),
        ("bc_f0", "pos12.tsv", ["-d", "bc", "-f", "0"]),
        ("cos_f0_x17", "mix12.tsv", ["-f", "0", "-x", "17"]),
        ("l1_comma_x17", "comma12.csv", ["-S", ",", "-d", "l1", "-x", "17"]),
        ("cos_gz_x17", "mix12.tsv.gz", ["-x", "17"]),
        ("l2_hash_x17", "hash9.tsv", ["-d", "l2", "-x", "17"]),
        ("cos_one", "one.tsv", []),
        ("cos_two_x17", "two.tsv", ["-x", "17"]),
        ("p_two_x17", "two.tsv", ["-d", "p", "-x", "17"]),
        ("l1_col1_x17", "col1.tsv", ["-d", "l1", "-x", "17"]),
        ("cos_col1_x17", "col1.tsv", ["-x", "17"]),
        ("p_col1_x17", "col1.tsv", ["-d", "p", "-x", "17"]),
    ]
    trees = [("tree_cos_dnj", "cos", "dnj"), ("tree_cos_nj", "cos", "nj"), ("tree_l2_dnj", "l2", "dnj"),
             ("tree_l2_nj", "l2", "nj"), ("tree_l2_p_dnj", "l2", "dnj")]
    return cases, trees


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle all")
    import tsv_oracle
    os.makedirs(OUT, exist_ok=True)
    os.chdir(OUT)
    rng = np.random.default_rng(20211)
    mix = table(rng, 12, 37, -5, 5)
    write_table("mix12.tsv", mix)
    write_table("mix12.tsv.gz", mix, gz=True)
    write_table("pos12.tsv", table(rng, 12, 37, 0, 10))
    write_table("tree30.tsv", table(rng, 30, 12, 0.5, 10, special=False))
    write_table("comma12.csv", table(rng, 12, 5, -5, 5), sep=",")
    write_table("hash9.tsv", table(rng, 9, 4, -5, 5), hashes=3)
    write_table("one.tsv", table(rng, 1, 6, -5, 5, special=False))
    write_table("two.tsv", table(rng, 2, 6, -5, 5, special=False))
    write_table("col1.tsv", table(rng, 9, 1, -5, 5))
    cases, trees = plan()
    listed = []
    for name, inp, opts in cases:
        args = ["tsv2phy", "-i", inp] + opts
        p = subprocess.run([REF] + args, capture_output=True, check=True)
        if "17" in opts:
            d = opts[opts.index("-d") + 1] if "-d" in opts else "cos"
            kind, ex = tsv_oracle.parse_metric(d)
            sep = opts[opts.index("-S") + 1] if "-S" in opts else "\t"
            X = tsv_oracle.read_tsv(inp, sep, 4 if "-p" in opts else 8)
            m, cells = tsv_oracle.parse_phy(p.stdout)
            mine = tsv_oracle.vec_ltd(X, kind, ex)
            assert m == X.shape[0] and np.isfinite(cells).all(), name
            if kind == "ln":
                assert np.allclose(mine, cells, rtol=1e-12, atol=0), name
            else:
                bad = int((mine.view(np.uint64) != cells.view(np.uint64)).sum())
                assert bad == 0, f"{name}: {bad} of {len(cells)} cells differ from the restatement"
        with open(name + ".out", "wb") as f:
            f.write(p.stdout)
        listed.append({"name": name, "input": inp, "args": args, "out": name + ".out",
                       "md5": hashlib.md5(p.stdout).hexdigest()})
    for name, d, method in trees:
        opts = ["-d", d] + (["-p"] if "_p_" in name else [])
        args = ["tsv2phy", "-i", "tree30.tsv", "-x", "17"] + opts
        phy = subprocess.run([REF] + args, capture_output=True, check=True).stdout
        m, cells = tsv_oracle.parse_phy(phy)
        assert (cells >= 0).all(), name
        nwk = subprocess.run([REF, "tree", "-m", method], input=phy, capture_output=True, check=True).stdout
        with open(name + ".nwk", "wb") as f:
            f.write(nwk)
        listed.append({"name": name, "input": "tree30.tsv", "args": args, "tree": method, "out": name + ".nwk",
                       "md5": hashlib.md5(nwk).hexdigest()})
    with open("tsv.json", "w") as f:   # one case per line
        f.write('{"reference": "ccphylo 0.8.5 (oracle/_ref/ccphylo, built by oracle/Makefile)", "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in listed) + "\n]}\n")
    print(f"{len(listed)} golden cases")
    for c in listed:
        print(c["name"], c["args"][3:], os.path.getsize(c["out"]))


if __name__ == "__main__":
    main()
