#!/usr/bin/env python3
"""Generates the golden vectors of `ccphylo dist -y` (methylation motif masking)
by running the REFERENCE binary built by oracle/Makefile (oracle/_ref/ccphylo):

    python __graft_entry__.py && python tests/golden/gen_meth_golden.py

Outputs (data, committed) under meth/: the inputs (small alignments, motif
files, one of them gzip), meth.json listing the cases with their command lines,
and the reference's stdout (*.out) and stderr (*.err) bytes.  The generator
checks with tests/meth_oracle.py that the cases cover what they are meant to:
sites found, the first record excluded by masking alone, a pair-mode record
excluded by masking alone."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
OUT = os.path.join(HERE, "meth")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fasta(names, seqs, width=60):
    return "".join(">%s\n%s\n" % (n, "\n".join(s[k:k + width] for k in range(0, len(s), width)))
                   for n, s in zip(names, seqs)).encode()


def inputs():
    rng = np.random.default_rng(20240611)
    # a8: 8 taxa x 200 columns around one ancestor: SNPs, N / gap columns, a lowercase stretch, planted motifs
    L = 200
    anc = rng.choice(list("ACGT"), L)
    for at, text in ((5, "GATC"), (30, "GATC"), (62, "GAATC"), (90, "TAG"), (127, "GAGTC"), (150, "GATC"),
                     (180, "AAG"), (196, "GATC")):
        anc[at:at + len(text)] = list(text)
    a8 = []
    for t in range(8):
        s = anc.copy()
        snp = rng.choice(L, 12, replace=False)
        s[snp] = rng.choice(list("ACGT"), 12)
        s[rng.choice(L, 3, replace=False)] = "N"
        if t % 3 == 1:
            s[40:44] = "-"
        if t == 5:
            s[100:120] = [c.lower() for c in s[100:120]]
        a8.append("".join(s))
    files = {"a8.fsa": fasta(["t%d" % t for t in range(8)], a8)}
    # b6: 6 taxa x 60; records 0 and 3 are nearly all GATC: gAtc clears half of their columns;
    # record 5 is mostly N (below -L 40 before masking) with sites in the rest
    dense = "GATC" * 15
    d3 = list(dense)
    d3[7] = "G"
    b5 = [dense, "".join(rng.choice(list("ACGT"), 60)), "".join(rng.choice(list("ACGT"), 60)), "".join(d3),
          "".join(rng.choice(list("ACGT"), 60)), "N" * 17 + "GATCCGATC" + "N" * 18 + "GATTGATCAGGATCTA"]
    files["b5.fsa"] = fasta(["dense0", "r1", "r2", "dense3", "r4", "nrich5"], b5)
    files["dam.fa"] = b">dam\ngAtc\n"
    multi = b">dam even palindrome\ngAtc\n>odd\nTag\n>degenerate, its widest base the site\ngaNtc\n>two sites\nRRg\n"
    files["multi.fa"] = multi
    files["multi.fa.gz"] = gzip.compress(multi, mtime=0)
    return files


# (name, input, motif file, options)
PLAN = [
    ("a8_dam", "a8.fsa", "dam.fa", []),
    ("a8_multi", "a8.fsa", "multi.fa", []),
    ("a8_multi_gz", "a8.fsa", "multi.fa.gz", []),
    ("a8_multi_f3n", "a8.fsa", "multi.fa", ["-f", "3", "-n", "/dev/null"]),
    ("a8_multi_P5", "a8.fsa", "multi.fa", ["-P", "5"]),
    ("a8_multi_f3P5", "a8.fsa", "multi.fa", ["-f", "3", "-P", "5"]),
    ("a8_multi_W1000p", "a8.fsa", "multi.fa", ["-W", "1000", "-p"]),
    ("a8_multi_f11", "a8.fsa", "multi.fa", ["-f", "11"]),
    ("a8_dam_f33s", "a8.fsa", "dam.fa", ["-f", "33", "-s", "10"]),
    ("b5_dam_L40", "b5.fsa", "dam.fa", ["-L", "40"]),
    ("b5_dam_f3L40", "b5.fsa", "dam.fa", ["-f", "3", "-L", "40", "-n", "/dev/null"]),
    ("b5_multi_f3L20C60", "b5.fsa", "multi.fa", ["-f", "3", "-L", "20", "-C", "60"]),
]


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle all")
    import meth_oracle
    os.makedirs(OUT, exist_ok=True)
    files = inputs()
    for name, data in files.items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
    os.chdir(OUT)
    cases = []
    for name, inp, mot, opts in PLAN:
        args = ["dist", "-i", inp, "-y", mot] + opts
        p = subprocess.run([REF] + args, capture_output=True, check=True)
        plain = subprocess.run([REF, "dist", "-i", inp] + opts, capture_output=True, check=True)
        assert p.stdout and p.stdout != plain.stdout, f"{name}: -y changes nothing"
        with open(name + ".out", "wb") as f:
            f.write(p.stdout)
        with open(name + ".err", "wb") as f:
            f.write(p.stderr)
        cases.append({"name": name, "input": inp, "motifs": mot, "args": args, "out": name + ".out", "err": name + ".err",
                      "plain_err": plain.stderr.decode()})
    by = {c["name"]: c for c in cases}
    # the first record goes by masking alone, so the second is the reference
    e, q = open("b5_dam_L40.err").read(), by["b5_dam_L40"]["plain_err"]
    assert "# Excluded:\tdense0" in e and "# Included:\tdense0" in q and "# Included:\tdense3" in e
    # pair mode: a later record goes by masking alone
    e, q = open("b5_dam_f3L40.err").read(), by["b5_dam_f3L40"]["plain_err"]
    assert "# Excluded:\tdense3" in e and "# Included:\tdense3" in q and "# Excluded:\tdense0" in e
    # ... and one that fails before masking is printed with its count after masking (25 less the A and T of 4 GATC)
    assert "# Excluded:\tnrich5\t( 25 / 60 )" in q and "# Excluded:\tnrich5\t( 17 / 60 )" in e, (q, e)
    for c in cases:
        del c["plain_err"]
        out, err = meth_oracle.expected_cli(OUT, c)
        assert out == open(c["out"], "rb").read(), f"{c['name']}: the restatement's stdout differs"
        assert err == open(c["err"], "rb").read(), f"{c['name']}: the restatement's stderr differs"
    with open("meth.json", "w") as f:
        f.write('{"reference": "ccphylo 0.8.5 (oracle/_ref/ccphylo, built by oracle/Makefile)", "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print(f"{len(cases)} golden cases")


if __name__ == "__main__":
    main()
