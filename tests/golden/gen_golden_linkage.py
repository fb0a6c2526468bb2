#!/usr/bin/env python3
"""Generates the golden vectors of the tree methods upgma, cf, ff and mn by
running the REFERENCE ccphylo binary built by oracle/Makefile
(oracle/_ref/ccphylo) on the inputs gen_golden.py committed (no new inputs;
run gen_golden.py first):

    make -C oracle && python tests/golden/gen_golden_linkage.py

Outputs (data, committed): golden_linkage.json lists the cases with their
command lines and md5; golden_linkage_out.tar.gz holds the outputs lk_*.out
(453 KB of Newick text; the tests read the members), and
golden_linkage_adv_out.tar.gz those of the adversarial matrices adv_*.phy.gz
(an archive of their own: the first one stays as it is).  cf has no cases on
matrices with missing cells (its update in the reference miscounts there; the
engine refuses them)."""
import gzip
import hashlib
import io
import json
import os
import subprocess
import sys
import tarfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "ccphylo")


def run(args, out, tar):
    p = subprocess.run([REF] + args, capture_output=True, check=True)
    assert p.stdout, args
    info = tarfile.TarInfo(out)   # mtime 0, no owner: the archive depends on the outputs alone
    info.size = len(p.stdout)
    tar.addfile(info, io.BytesIO(p.stdout))
    return hashlib.md5(p.stdout).hexdigest()


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle")
    os.chdir(HERE)
    cases = []
    variants = [("test", "test.phy.gz", []), ("test_p", "test.phy.gz", ["-p"]), ("test_f1", "test.phy.gz", ["-f", "1"]),
                ("test_f2", "test.phy.gz", ["-f", "2"]), ("test_s", "test.phy.gz", ["-s", "1000"]),
                ("test_x4", "test.phy.gz", ["-x", "4"]), ("snp300", "snp300.phy", []), ("snp300_s", "snp300.phy", ["-s"]),
                ("snp300_b", "snp300.phy", ["-b"]), ("euc400", "euc400.phy.gz", []), ("euc400_p", "euc400.phy.gz", ["-p"])]
    missing = [("miss80", "miss80.phy", []), ("miss80_p", "miss80.phy", ["-p"]), ("multi", "multi.phy", [])]
    with open("golden_linkage_out.tar.gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as gz, \
            tarfile.open(fileobj=gz, mode="w") as tar:
        for m in ("upgma", "cf", "ff", "mn"):
            for name, inp, extra in variants + ([] if m == "cf" else missing):
                args = ["tree", "-i", inp, "-m", m] + extra
                out = f"lk_{name}_{m}.out"
                cases.append({"name": f"{name}_{m}", "kind": "tree", "method": m, "args": args, "out": out,
                              "md5": run(args, out, tar)})
    # the adversarial matrices, at the -x of their golden.json cases (gen_golden.py (viii)); none has missing cells
    with open("golden.json") as f:
        xs = {c["args"][2]: c["args"][-1] for c in json.load(f)["cases"] if c["name"].startswith("adv_")
              and c["name"].endswith("_dnj")}
    with open("golden_linkage_adv_out.tar.gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as gz, \
            tarfile.open(fileobj=gz, mode="w") as tar:
        for m in ("upgma", "cf", "ff", "mn"):
            for inp in sorted(xs):
                name = inp[:-len(".phy.gz")]
                args = ["tree", "-i", inp, "-m", m, "-x", xs[inp]]
                out = f"lk_{name}_{m}.out"
                cases.append({"name": f"{name}_{m}", "kind": "tree", "method": m, "args": args, "out": out,
                              "md5": run(args, out, tar)})
    with open("golden_linkage.json", "w") as f:   # one case per line
        f.write('{"reference": "ccphylo 0.8.5 (oracle/_ref/ccphylo, built by oracle/Makefile)", "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print(f"{len(cases)} golden cases")


if __name__ == "__main__":
    main()
