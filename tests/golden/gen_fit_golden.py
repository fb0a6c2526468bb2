#!/usr/bin/env python3
"""Generates the golden vectors of `ccphylo nwck2phy` and `ccphylo phycmp` by
running the REFERENCE binary built by oracle/Makefile (oracle/_ref/ccphylo):

    python __graft_entry__.py && python tests/golden/gen_fit_golden.py

Outputs (data, committed) under fit/:
  *.nwk            hand-written Newick inputs (the trees of gen_golden.py are
                   read where they lie)
  *.phy.gz         the reference's `nwck2phy` stdout (gzip, mtime 0), which
                   also serve as `phycmp` inputs
  in_*.phy.gz      further `phycmp` inputs derived from committed matrices:
                   perturbed, shuffled and all-zero copies
  fit.json         the cases: command line, exit status, stderr, and for
                   `phycmp` the stdout itself
The generator checks every case against tests/fit_oracle.py (names, cells as
printed, metric lines), and that no `phycmp` value lies within 1e-9 of a tie
in the sixth decimal, so that %f cannot hide a summation difference."""
import gzip
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
OUT = os.path.join(HERE, "fit")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HAND = {
    "star": b"(A:1,B:2,C:3,D:4);\n",
    "trifurc": b"(Alpha:1.5,Beta:2.25,(Gamma:1.125,Delta:2.0625):3.5);\n",
    "lj_neg": b"((A:1.5,B:2.5):1.5,C:-3.5);\n((P:-1.5,Q:2.5):1.5,R:0.25,S:-2.75);\n",
    "two_lines": b"first (A:1.25,B:2.5,C:3.75);\nsecond tree\t((X:1.5,Y:2.25):0.5,Z:4.125,W:1.0625);\n",
}
# (name, input relative to tests/golden, extra options)
NWCK = [(t, t + ".out", []) for t in ("miss80_dnj", "test_hnj_f2", "adv_line_nj", "adv_dupes_dnj")]
NWCK += [("star", "fit/star.nwk", []), ("trifurc", "fit/trifurc.nwk", []), ("lj_neg", "fit/lj_neg.nwk", []),
         ("two_lines", "fit/two_lines.nwk", ["-f", "5"]), ("miss80_nj", "miss80_nj.out", [])]


def gz_write(path, data):
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(data)


def phy_text(names, D, n, fmt="%.6f"):
    out = ["%10d\n" % n]
    k = 0
    for i in range(n):
        out.append(names[i] + "".join("\t" + fmt % D[k + j] for j in range(i)) + "\n")
        k += i
    return "".join(out).encode()


def parse_phy(data):
    """[(header, names, cells as text)] of a relaxed Phylip text"""
    mats = []
    lines = data.split(b"\n")
    k = 0
    while k < len(lines) and lines[k].strip():
        hdr = None
        if lines[k].startswith(b"#"):
            hdr = lines[k][1:]
            k += 1
        n = int(lines[k])
        names, cells = [], []
        for i in range(n):
            f = lines[k + 1 + i].split(b"\t")
            names.append(f[0])
            cells += f[1:]
            assert len(f) == i + 1
        mats.append((hdr, names, cells))
        k += n + 1
    return mats


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle all")
    import fit_oracle as fo
    from ccphylo_amd import native
    os.makedirs(OUT, exist_ok=True)
    os.chdir(HERE)
    biggest = max(os.path.getsize(f) for f in os.listdir(HERE) if os.path.isfile(f))
    for name, text in HAND.items():
        with open(os.path.join(OUT, name + ".nwk"), "wb") as f:
            f.write(text)
    cases = []
    # ---- nwck2phy, double and float
    for name, inp, opts in NWCK:
        with open(inp, "rb") as f:
            parsed = fo.parse_file(f.read())
        for et, popt in ((8, []), (4, ["-p"])):
            cname = name + ("_p" if et == 4 else "")
            args = ["nwck2phy", "-i", inp] + opts + popt
            p = subprocess.run([REF] + args, capture_output=True)
            mats = parse_phy(p.stdout)
            good = [r for r in parsed if not isinstance(r, Exception)]
            assert len(mats) == len(good), cname
            assert (p.returncode != 0) == (len(good) != len(parsed)), cname
            if p.returncode:
                assert isinstance(parsed[-1], fo.InvalidLimb), cname
                assert p.stderr == b"Invalid limb length at node:\t" + parsed[-1].args[0].encode("latin-1") + b"\n"
            for (hdr, names, cells), (h, nm, sp) in zip(mats, good):
                assert names == nm and (hdr is None or hdr == h), cname
                D = fo.replay(sp, et) if len(sp) < 200 else fo.replay_np(sp, et)
                assert len(cells) == len(D), cname
                # the text has 9 decimals (trailing zeros cut): every cell as printed
                assert all(float("%.9f" % v) == float(c) for v, c in zip(D, cells)), cname
            case = {"cmd": "nwck2phy", "name": cname, "args": args, "etype": et, "rc": p.returncode,
                    "stderr": p.stderr.decode("latin-1"), "md5": hashlib.md5(p.stdout).hexdigest(), "out": None,
                    "matrices": len(mats)}
            if p.stdout:
                case["out"] = cname + ".phy.gz"
                gz_write(os.path.join(OUT, case["out"]), p.stdout)
            cases.append(case)
    # ---- phycmp inputs
    rng = np.random.default_rng(20261021)

    def derived(name, src, fn):
        (names, D), = native.load_phylip(os.path.join(HERE, src))
        n = len(names)
        names2, D2 = fn(list(names), np.array(D, dtype=np.float64), n)
        gz_write(os.path.join(OUT, name), phy_text(names2, D2, n))

    def perturb(names, D, n):
        D2 = np.where(D < 0, D, np.round(D * (1 + 0.2 * rng.random(D.size)), 6))
        return names, D2

    def perturb_missing(names, D, n):
        D2 = np.where(D < 0, D, np.round(D * (1 + 0.2 * rng.random(D.size)) + 0.5, 6))
        D2[rng.random(D.size) < 0.02] = -1.0   # cells missing in one matrix only
        return names, D2

    def shuffle_of(src_perturbed):
        def fn(names, D, n):
            (nm, Dp), = native.load_phylip(os.path.join(OUT, src_perturbed))
            perm = rng.permutation(n)
            return [nm[k] for k in perm], fo.permute_lt(np.array(Dp, dtype=np.float64), n, perm)
        return fn

    derived("in_test_pert.phy.gz", "test.phy.gz", perturb)
    derived("in_miss80_pert.phy.gz", "miss80.phy", perturb_missing)
    derived("in_miss80_pert_shuf.phy.gz", "miss80.phy", shuffle_of("in_miss80_pert.phy.gz"))
    zero = phy_text(["z%d" % i for i in range(5)], np.zeros(10), 5)
    gz_write(os.path.join(OUT, "in_zero5x2.phy.gz"), zero + zero)   # one file that holds both matrices
    gz_write(os.path.join(OUT, "in_zero5.phy.gz"), zero)
    PHYCMP = [
        ("self_p", ["fit/adv_line_nj.phy.gz", "fit/adv_line_nj_p.phy.gz"]),
        ("perturbed", ["test.phy.gz", "fit/in_test_pert.phy.gz"]),
        ("itself", ["test.phy.gz", "test.phy.gz"]),
        ("zero", ["fit/in_zero5x2.phy.gz"]),
        ("missing", ["miss80.phy", "fit/in_miss80_pert.phy.gz"]),
        ("err_missing", ["fit/in_zero5.phy.gz"]),
        ("err_size", ["fit/in_zero5.phy.gz", "miss80.phy"]),
        ("err_entries", ["miss80.phy", "fit/in_miss80_pert_shuf.phy.gz"]),
    ]
    for name, files in PHYCMP:
        for et, popt in ((8, []), (4, ["-p"])):
            cname = name + ("_p" if et == 4 else "")
            args = ["phycmp", "-f", "127"] + popt + ["-i"] + files
            p = subprocess.run([REF] + args, capture_output=True)
            case = {"cmd": "phycmp", "name": cname, "args": args, "etype": et, "rc": p.returncode,
                    "stderr": p.stderr.decode(), "stdout": p.stdout.decode(), "files": files}
            if p.returncode == 0:
                mats = []
                for f in files:
                    mats += native.load_phylip(os.path.join(HERE, f), etype=et)
                (n1, A), (n2, B) = mats
                n = len(n1)
                s, _ = fo.cmp_sums(A, B, et)
                cells = n * (n - 1) // 2
                assert fo.phycmp_lines(s, cells, 127) == case["stdout"], (cname, fo.phycmp_lines(s, cells, 127), case["stdout"])
                for m in fo.METRIC_NAMES:
                    v = fo.metric(s, cells, m)
                    if math.isfinite(v):
                        frac = abs(v) * 1e6 % 1.0
                        assert abs(frac - 0.5) > 1e-9 * 1e6, (cname, m, v)
                case["n"] = n
            else:
                assert p.stdout == b""
            cases.append(case)
    msgs = {c["stderr"] for c in cases if c["cmd"] == "phycmp" and c["rc"]}
    assert msgs == {"Missing matrix\n", "Matrices differ in size.\n", "Matrices has different entries.\n"}, msgs
    with open(os.path.join(OUT, "fit.json"), "w") as f:   # one case per line
        f.write('{"reference": "ccphylo 0.8.5 (oracle/_ref/ccphylo, built by oracle/Makefile)", "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    for fn in sorted(os.listdir(OUT)):
        size = os.path.getsize(os.path.join(OUT, fn))
        assert size <= biggest, (fn, size)
        print(fn, size)
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
