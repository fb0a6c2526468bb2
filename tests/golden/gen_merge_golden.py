#!/usr/bin/env python3
"""Generates the golden vectors of `ccphylo merge` by running the REFERENCE
binary built by oracle/Makefile (oracle/_ref/ccphylo):

    python __graft_entry__.py && python tests/golden/gen_merge_golden.py

Outputs (data, committed) under merge/:
  <case>.phy.gz      the multi-Phylip input (gzip, mtime 0)
  <case>.w.phy.gz    the weights file of a -w case
  <case>.stdout.gz / .o.gz / .n.gz   the reference's stdout and its -o / -n files
  merge.json         the cases: options, exit status, stderr
Every case stays inside the envelope in which the reference is reliable (first
matrix <= 63 entries, <= 126 distinct names: asserted), and the generator
checks tests/merge_oracle.py against every byte it stores.

The reference has a third limit, found here: getOrderedNames (merge.c:109)
walks the buckets `i < size` with size already turned into the mask 127, so a
name whose hash falls into the last bucket never reaches the output's name
list, and printphy then reads an unset pointer (SIGSEGV, or bytes of another
string).  Which names those are is asked of the reference itself (usable()),
and the large case takes its names from the ones it keeps."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")
OUT = os.path.join(HERE, "merge")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def gz_write(path, data):
    with open(path, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(data)


def phy_text(names, cells, sep="\t", header=None):
    out = [] if header is None else ["#" + header + "\n"]
    out.append("%10d\n" % len(names))
    k = 0
    for i, nm in enumerate(names):
        out.append(nm + "".join(sep + c for c in cells[k:k + i]) + "\n")
        k += i
    return "".join(out)


def num(v):
    return "%d" % v if v == int(v) else ("%.9f" % v).rstrip("0")


def matrix(rng, names, lo=0.0, hi=100.0, digits=4, sep="\t", header=None, values=None):
    m = len(names)
    cells = m * (m - 1) // 2
    v = np.round(rng.uniform(lo, hi, cells), digits) if values is None else values
    return phy_text(names, [num(x) for x in v], sep, header)


def usable(name):
    """the reference keeps `name`: a two-matrix merge of (name, zz) prints it"""
    text = phy_text([name, "zz"], ["1"])
    with tempfile.NamedTemporaryFile(suffix=".phy") as t:
        t.write((text + text).encode())
        t.flush()
        p = subprocess.run([REF, "merge", "-i", t.name], capture_output=True)
    return p.returncode == 0 and p.stdout == phy_text([name, "zz"], ["1"]).encode()


def build_cases():
    rng = np.random.default_rng(20261021)
    S = ["s%02d" % i for i in range(12)]
    cases = []

    def add(name, mats, wmats=None, opts=(), files=(), sep="\t"):
        cases.append(dict(name=name, data="".join(mats).encode(), wdata="".join(wmats).encode() if wmats else None,
                          opts=list(opts), files=list(files), sep=sep))

    def weights_for(sets, zero_at=None, **kw):
        out = []
        for k, nm in enumerate(sets):
            m = len(nm)
            w = rng.integers(1, 5000, m * (m - 1) // 2).astype(float)
            if zero_at is not None and k == zero_at[0]:
                w[zero_at[1]] = 0
            out.append(matrix(rng, nm, values=w, **kw))
        return out

    # three matrices with partly overlapping, reordered names
    sets3 = [S[0:6], [S[7], S[3], S[1], S[8], S[5]], [S[8], S[0], S[9], S[2], S[7], S[4], S[10]]]
    d3 = [matrix(rng, nm) for nm in sets3]
    w3 = weights_for(sets3)
    add("plain3", d3)
    add("w3", d3, w3, files=("o", "n"))
    add("w3_stdout", d3, w3)                      # -w without -n: both matrices on stdout, D first
    add("plain3_p", d3, opts=["-p"])
    add("w3_p", d3, w3, opts=["-p"], files=("o", "n"))
    add("plain3_f4", d3, opts=["-f", "4"])
    add("plain3_f5", d3, opts=["-f", "5"])
    add("plain3_f0", d3, opts=["-f", "0"])
    add("w3_x3", d3, w3, opts=["-x", "3"], files=("n",))
    # a pair that never co-occurs: s00 / s11 -> -1
    never = [[S[0], S[1], S[2]], [S[11], S[2], S[1]]]
    add("never", [matrix(rng, nm) for nm in never])
    add("never_w", [matrix(rng, nm) for nm in never], weights_for(never), files=("n",))
    # a zero weight, in the first matrix and in a later one (cells seen once -> N = 0 -> -1)
    zsets = [S[0:4], [S[3], S[4], S[0]]]
    add("w_zero_first", [matrix(rng, nm) for nm in zsets], weights_for(zsets, zero_at=(0, 1)), files=("n",))
    add("w_zero_later", [matrix(rng, nm) for nm in zsets], weights_for(zsets, zero_at=(1, 0)), files=("n",))
    # the weights file carries different names: they are the ones merged and printed
    dn = [["a", "b", "c", "d"], ["c", "e", "a"]]
    wn = [["P", "Q", "R", "T"], ["T", "Q", "U"]]
    add("w_names", [matrix(rng, nm) for nm in dn], weights_for(wn), files=("n",))
    # -S ,: the separator stays inside the name
    add("sep_comma", [matrix(rng, nm, sep=",") for nm in sets3], opts=["-S", ","], sep=",")
    # a one-entry first matrix, and one in the middle
    one = [[S[5]], S[3:7], [S[9]], [S[9], S[5], S[0]]]
    add("one_first", [matrix(rng, nm) for nm in one])
    add("one_first_w", [matrix(rng, nm) for nm in one], weights_for(one), files=("n",))
    # -1 distances are summed like any other value; zeros, tiny and large values beside them
    msets = [S[0:5], [S[4], S[2], S[0], S[6]], [S[6], S[0], S[4]]]
    pool = np.array([0.0, -1.0, 2.0 / 3.0, 1e-7, 12345.678, -1.0, 0.5, 3.0])
    mm = [matrix(rng, nm, values=rng.choice(pool, len(nm) * (len(nm) - 1) // 2)) for nm in msets]
    add("minus_one", mm)
    add("minus_one_w", mm, weights_for(msets), files=("n",))
    add("minus_one_p", mm, opts=["-p"])
    # comment lines in the input, and a size line of 0 that ends it
    add("headers", [matrix(rng, nm, header="tmpl%d" % k) for k, nm in enumerate(sets3)] + ["%10d\n" % 0, d3[0]],
        opts=["-f", "5"])
    # the edge of the reference's envelope: 63 entries growing to 126 names
    assert usable("n000") and not all(usable("n%03d" % i) for i in range(200))   # the last bucket does lose names
    big = [nm for nm in ("n%03d" % i for i in range(200)) if usable(nm)][:126]
    perm = [big[i] for i in rng.permutation(126)]
    add("edge126", [matrix(rng, big[:63], digits=2), matrix(rng, perm, digits=2)])
    add("edge126_w", [matrix(rng, big[:63], digits=2), matrix(rng, perm, digits=2)], weights_for([big[:63], perm]),
        opts=["-p"], files=("n",))
    # the weights file is short: exit 1
    add("w_short", d3, w3[:2], files=("o", "n"))
    add("w_size", d3, [w3[0], w3[2], w3[1]])
    return cases


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle all")
    import merge_oracle as mo
    os.makedirs(OUT, exist_ok=True)
    listed = []
    for c in build_cases():
        name = c["name"]
        et = 4 if "-p" in c["opts"] else 8
        mats = mo.parse_multi(c["data"], et, c["sep"].encode())
        distinct = {nm for names, _ in mats for nm in names}
        if c["wdata"] is not None:
            distinct |= {nm for names, _ in mo.parse_multi(c["wdata"], et, c["sep"].encode()) for nm in names}
        assert len(mats[0][0]) <= 63 and len(distinct) <= 126, name   # the reference's envelope
        gz_write(os.path.join(OUT, name + ".phy.gz"), c["data"])
        if c["wdata"] is not None:
            gz_write(os.path.join(OUT, name + ".w.phy.gz"), c["wdata"])
        with tempfile.TemporaryDirectory() as tmp:
            args = ["merge", "-i", os.path.join(OUT, name + ".phy.gz")] + c["opts"]
            if c["wdata"] is not None:
                args += ["-w", os.path.join(OUT, name + ".w.phy.gz")]
            for f in c["files"]:
                args += ["-" + f, os.path.join(tmp, f)]
            p = subprocess.run([REF] + args, capture_output=True)
            got = {"stdout": p.stdout}
            for f in c["files"]:
                path = os.path.join(tmp, f)
                got[f] = open(path, "rb").read() if os.path.exists(path) else None
        # the restatement, byte for byte
        flag = int(c["opts"][c["opts"].index("-f") + 1]) if "-f" in c["opts"] else 1
        prec = int(c["opts"][c["opts"].index("-x") + 1]) if "-x" in c["opts"] else 9
        rc, err, dtext, ntext = mo.run(c["data"], c["wdata"], et, flag, prec, c["sep"].encode())
        assert (rc, err) == (p.returncode, p.stderr), (name, rc, err, p.returncode, p.stderr)
        if rc == 0:
            want = {"stdout": b"", "o": None, "n": None}
            want["o" if "o" in c["files"] else "stdout"] = dtext
            if ntext is not None:
                key = "n" if "n" in c["files"] else "stdout"
                want[key] = (want[key] or b"") + ntext
            for k, v in got.items():
                assert v == want[k], (name, k, v[:300] if v else v, want[k][:300] if want[k] else want[k])
        entry = {"name": name, "opts": c["opts"], "weights": c["wdata"] is not None, "files": c["files"],
                 "etype": et, "rc": p.returncode, "stderr": p.stderr.decode(), "outputs": {}}
        for k, v in got.items():
            if v is not None and (v or k == "stdout"):
                gz_write(os.path.join(OUT, "%s.%s.gz" % (name, k)), v)
                entry["outputs"][k] = "%s.%s.gz" % (name, k)
            elif v is not None:
                entry["outputs"][k] = ""      # the file exists and is empty
        listed.append(entry)
    with open(os.path.join(OUT, "merge.json"), "w") as f:   # one case per line
        f.write('{"reference": "ccphylo 0.8.5 (oracle/_ref/ccphylo, built by oracle/Makefile)", "cases": [\n')
        f.write(",\n".join(json.dumps(e) for e in listed) + "\n]}\n")
    total = 0
    for fn in sorted(os.listdir(OUT)):
        size = os.path.getsize(os.path.join(OUT, fn))
        assert size < 256 * 1024, (fn, size)
        total += size
    print(len(listed), "cases,", total, "bytes")


if __name__ == "__main__":
    main()
