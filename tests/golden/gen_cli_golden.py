#!/usr/bin/env python3
"""Records the argument surface of the `ccphylo` command line:

    python tests/golden/gen_cli_golden.py PATH/TO/bin/ccphylo

writes cli/cases.json (data, committed): for every case the argv, the stdin
bytes, the files of its working directory, and the exit status, stdout and
stderr that binary answered with (each distinct output once, in "texts").
tests/test_cli_args.py replays them on the binary of the tree and compares all three byte for byte, so the binary given
here is the one to be compared AGAINST: one built from the parent commit in a
worktree outside the repository, when the argument handling is being changed.

Every case ends before a GPU is opened (help, sub-help, parse failures,
post-parse refusals, unreadable paths, the zero-row and one-row inputs that the
commands answer without a launch), so the corpus replays on a machine without
one; a case whose stderr says `cannot open GPU` fails the generator.  The OPTS
table below restates each command's options only to enumerate the cases: every
value option as the last word, with a non-numeric value where it is checked
and in the `--name=value` form; every flag clustered in front of `-h`.
Where a line only has to show that a value was taken, it ends in `-Z`, which is
unknown to every command and answers in one short line."""
import base64
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cli", "cases.json")

# kind: flag (no value), str / int / dbl (value; int and dbl are checked), prec (optional number),
# list (file list), sub (a sub-help flag), help
COMMON_TAIL = [("H", "mmap", "flag"), ("T", "tmp", "str"), ("h", "help", "help")]
PREC = [("p", "float_precision", "flag"), ("s", "short_precision", "prec"), ("b", "byte_precision", "prec")]
OPTS = {
    "tree": [("i", "input", "str"), ("o", "output", "str"), ("S", "separator", "str"), ("q", "quotes", "str"),
             ("x", "print_precision", "int"), ("m", "method", "str"), ("M", "method_help", "sub"),
             ("f", "flag", "int"), ("F", "flag_help", "sub")] + PREC +
            [("g", "free", "flag"), ("H", "mmap", "flag"), ("T", "tmp", "str"), ("t", "threads", "int"),
             ("h", "help", "help"), (None, "gpus", "int"), (None, "transport", "str"), (None, "fast_sums", "flag"),
             (None, "phycmp", "str"), (None, "phycmp_flag", "int"), (None, "device", "int"), (None, "stats", "flag")],
    "dbscan": [("i", "input", "str"), ("o", "output", "str"), ("S", "separator", "str"), ("q", "quotes", "str"),
               ("N", "min_neighbors", "int"), ("e", "max_distance", "dbl")] + PREC + COMMON_TAIL +
              [(None, "device", "int")],
    "dist": [("i", "input", "list"), ("o", "output", "str"), ("n", "nucleotide_numbers", "str"),
             ("x", "print_precision", "int"), ("y", "methylation_motifs", "str"), ("L", "min_len", "int"),
             ("C", "min_cov", "str"), ("W", "normalization_weight", "int"), ("P", "proximity", "int"),
             ("f", "flag", "int"), ("F", "flag_help", "sub")] + PREC +
            [("t", "threads", "int"), ("h", "help", "help"), (None, "tree", "str"), (None, "dbscan", "str"),
             (None, "max_distance", "dbl"), (None, "min_neighbors", "int"), (None, "tree_method", "str"),
             (None, "tree_flag", "int"), (None, "gpus", "int"), (None, "transport", "str"),
             ("d", "distance", "str"), ("D", "distance_help", "sub"), ("r", "reference", "str"),
             ("E", "min_depth", "str"), ("l", "significance_lvl", "str"), ("S", "separator", "str"),
             ("T", "tmp", "str"), ("H", "mmap", "flag"), ("a", "add", "str"), ("V", "nucleotide_variations", "str"),
             (None, "device", "int"), (None, "fast_sums", "flag")],
    "tsv2phy": [("i", "input", "str"), ("o", "output", "str"), ("S", "separator", "str"),
                ("x", "print_precision", "int"), ("d", "distance", "str"), ("D", "distance_help", "sub"),
                ("f", "flag", "int"), ("F", "flag_help", "sub")] + PREC + COMMON_TAIL +
               [(None, "tree", "str"), (None, "tree_method", "str"), (None, "device", "int")],
    "nwck2phy": [("i", "input", "str"), ("o", "output", "str"), ("x", "print_precision", "int"), ("f", "flag", "int"),
                 ("F", "flag_help", "sub")] + PREC + COMMON_TAIL + [(None, "device", "int")],
    "phycmp": [("i", "input", "list"), ("o", "output", "str"), ("S", "separator", "str"), ("f", "flag", "int"),
               ("F", "flag_help", "sub")] + PREC + COMMON_TAIL + [(None, "by_name", "flag"), (None, "device", "int")],
    "merge": [("i", "input", "str"), ("o", "output", "str"), ("w", "nucleotides_weights", "str"),
              ("n", "nucleotide_numbers", "str"), ("S", "separator", "str"), ("x", "print_precision", "int"),
              ("f", "flag", "int"), ("F", "flag_help", "sub")] + PREC + COMMON_TAIL +
             [(None, "tree", "str"), (None, "tree_method", "str"), (None, "device", "int")],
}

PHY1 = "1\nonly\n"
PHY2 = "2\nA\nB\t3.5\n"
PHY3 = "3\nA\nB\t1\nC\t2\t3\n"
PHY3B = "3\nA\nB\t1\nD\t2\t3\n"
PHY3R = "3\nC\nA\t2\nB\t3\t1\n"
MSA3 = ">a\nACGTACGTAC\n>b\nACGTACGTAA\n>c\nACGAACGTAC\n"
MSA1 = ">a\nACGTACGTAC\n"
MSA_N = ">a\nNNNNNNNNNN\n>b\nNNNNNNNNNN\n"
TSV1 = "1\t2\t3\n"
TSV2 = "1\t2\t3\n4\t5\t6\n"


def enc(b):
    try:
        t = b.decode("utf-8")
        if t.encode("utf-8") == b:
            return t
    except UnicodeDecodeError:
        pass
    return {"b64": base64.b64encode(b).decode("ascii")}


def build_cases():
    cases = []

    def add(cmd, args, stdin="", files=None):
        argv = ([cmd] if cmd else []) + list(args)
        cases.append({"argv": argv, "stdin": stdin, "files": files or {}})

    add(None, [])
    add(None, ["--help"])
    add(None, ["-h"])
    add(None, ["upgma"])
    for cmd, opts in OPTS.items():
        add(cmd, ["-h"])
        add(cmd, ["--help"])
        walked = set()
        for letter, name, kind in opts:
            short, long_ = ("-" + letter if letter else None), "--" + name
            if kind == "sub":
                add(cmd, [short])
                add(cmd, [long_])
                add(cmd, ["-p" + letter + "h"])
            elif kind == "flag":
                if (cmd, letter) == ("merge", "H"):   # -H ends its word there: -Hh would go on to the run
                    add(cmd, ["-Hh", "-F"])
                else:
                    add(cmd, ["-" + letter + "ph" if letter != "p" else "-pHh" if cmd != "merge" else "-ph"] if short
                        else [long_, "-h"])
            elif kind == "help":
                add(cmd, [long_ + "=x"])
            elif kind == "prec":
                add(cmd, [short, "-h"])
                add(cmd, [short + "x"])
                add(cmd, [long_ + "=0"])
                add(cmd, ["-p" + letter + "2", "-Z"])
            else:
                # -Z, unknown everywhere, ends a line whose value was taken: its message shows the walk went on
                add(cmd, [short or long_])                # the last word: Missing (a list of none for dist -i)
                add(cmd, [long_ + "=zz", "-Z"])           # Invalid where it is checked
                if kind not in walked:                    # the forms that are the walker's, once per kind and command
                    walked.add(kind)
                    add(cmd, [long_])
                    add(cmd, [long_, "zz", "-Z"])
                    add(cmd, [long_ + "=", "zz", "-Z"])   # an empty attached value: the next word is the value
                    add(cmd, [long_ + "=1", "-Z"])
                    add(cmd, ["--mmap=1", "-Z"])          # a value given to a flag is dropped
                    if short:
                        add(cmd, [short, "zz", "-Z"])
                        add(cmd, [short + "1", "-Z"])
                        add(cmd, ["-p" + letter + "1", "-Z"])   # flags clustered in front of a value option
                        add(cmd, ["-p" + letter])
        add(cmd, ["-Z"])
        add(cmd, ["-pZ"])
        add(cmd, ["--no_such_option"])
        add(cmd, ["--no_such_option=5"])
        add(cmd, ["--", "-h"])
        add(cmd, ["--=x", "-h"])
        add(cmd, ["one", "two"])
        add(cmd, ["-p", "one", "two"])
        add(cmd, ["-", "-h"])

    # the precision options of the issue, spelled out
    for cmd in OPTS:
        add(cmd, ["-b", "1e-2", "-h"])
        add(cmd, ["--byte_precision=0"])
        add(cmd, ["-s", "-h"])
        add(cmd, ["-s0"])
        add(cmd, ["-sx"])

    # oddities
    add("merge", ["-Hp", "-F"])
    add("tree", ["-Hp", "-F"])
    add("merge", ["-Hh", "-F"])
    add("tree", ["-Hh", "-F"])
    add("merge", ["-Hx", "zz", "-F"])
    add("tree", ["-Hx", "zz", "-F"])
    add("merge", ["-HZ", "-F"])
    add("tree", ["-HZ", "-F"])
    add("merge", ["--mmap", "-pF"])
    add("dist", ["--"])
    add("dist", ["--", "x.fsa"])
    add("dist", ["-C", "101"])
    add("dist", ["-C", "-1"])
    add("dist", ["-C", "x", "-h"])
    add("dist", ["-C", "x"], stdin="")
    add("dist", ["-C", "100", "-F"])
    add("dist", ["-E", "x", "-F"])
    add("dist", ["-a", "x"], stdin=MSA3)
    add("dist", ["-V", "x"], stdin=MSA3)
    add("dist", ["--add", "x"], stdin=MSA3)
    add("dist", ["--nucleotide_variations=x"], stdin=MSA3)
    add("dist", ["-a", "x", "-V", "y"], stdin=MSA3)
    add("dist", ["-a"])
    add("dist", ["-d", "nope"])
    add("dist", ["-d", "l2x"])
    add("dist", ["-d", "nl3x"])
    add("dist", ["-d", "l3", "-F"])
    add("dist", ["-d", "z", "-F"])
    add("dist", ["-D"])
    add("dist", ["-FD"])
    add("dist", ["-d", "nope", "-D"])
    add("dist", ["-D", "-d", "nope"])
    add("phycmp", ["a.phy", "b.phy", "c.phy"], files={"a.phy": PHY3, "b.phy": PHY3, "c.phy": PHY3})
    add("phycmp", ["-i", "a.phy", "b.phy", "c.phy"], files={"a.phy": PHY3, "b.phy": PHY3, "c.phy": PHY3})
    add("phycmp", ["-i", "a.phy", "b.phy", "-o", "out", "c.phy"], files={"a.phy": PHY3, "b.phy": PHY1})
    add("phycmp", ["-i"])
    add("phycmp", ["-pi"])
    add("phycmp", ["--input"])
    add("phycmp", ["--input="])
    add("phycmp", ["-ia.phy", "b.phy", "c.phy"])

    # post-parse refusals before the first open_gpu, once each
    add("tree", ["-m", "upgma"])
    add("tree", ["-m", "frank"])
    add("tree", ["-m", "nope"])
    add("tree", ["-m", "mh"])
    add("tree", ["-M", "-m", "nj", "no.phy"])
    add("tree", ["-m", "nj", "-M"])
    add("tree", ["-s", "0"])
    add("tree", ["-b0"])
    add("tree", ["--gpus", "-1"])
    add("tree", ["--gpus", "2", "-m", "cf"])
    add("tree", ["--gpus", "2", "-m", "ff"])
    add("tree", ["--gpus", "2", "-m", "mn"])
    add("tree", ["--phycmp", "cmp.out", "--gpus", "2"])
    add("tree", ["--phycmp", "cmp.out", "-s"])
    add("tree", ["--phycmp", "cmp.out", "-b"])
    add("tree", ["--transport", "tcp"])
    add("tree", ["--transport=host", "-h"])
    add("tree", ["--phycmp", "cmp.out"], stdin=PHY1)
    add("dbscan", ["-s", "0"])
    add("dbscan", ["-b", "0"])
    add("dist", ["-s", "0"])
    add("dist", ["-b", "0"])
    add("dist", ["-p", "-s0"])
    add("dist", ["--transport", "tcp"])
    add("dist", ["-y", "m.txt", "-r", "a", "a.fsa", "b.fsa"], files={"a.fsa": MSA1, "b.fsa": MSA1, "m.txt": "GATC\n"})
    add("dist", ["a.fsa", "b.fsa"], files={"a.fsa": MSA1, "b.fsa": MSA1})
    add("dist", ["-i", "a.fsa", "b.fsa", "-x", "5"], files={"a.fsa": MSA1, "b.fsa": MSA1})
    add("dist", ["-r", "t", "-d", "z", "a.mat", "b.mat"], files={"a.mat": "#t\n", "b.mat": "#t\n"})
    add("dist", ["-r", "t", "-d", "p", "-i", "a.mat", "b.mat"], files={"a.mat": "#t\n", "b.mat": "#t\n"})
    add("dist", ["--tree", "-", "--tree_method", "upgma"], stdin=MSA3)
    add("dist", ["--tree", "-", "--tree_method", "cf", "--gpus", "2"], stdin=MSA3)
    add("dist", ["--tree", "-", "-W", "1", "-s"], stdin=MSA3)
    add("dist", ["--dbscan", "-", "--gpus", "2"], stdin=MSA3)
    add("dist", ["--dbscan", "-", "-b", "2"], stdin=MSA3)
    add("dist", ["--dbscan", "-", "-s", "-W", "1"], stdin=MSA3)
    add("dist", ["--tree", "-"], stdin=PHY3)
    add("dist", ["--tree", "-"], stdin=MSA1)
    add("dist", ["--dbscan", "-"], stdin=MSA1)
    add("dist", ["--dbscan", "db.out", "in.fsa"], files={"in.fsa": MSA1})
    add("dist", ["--tree", "nodir/t.nwk"], stdin=MSA3)
    add("dist", ["--dbscan", "nodir/d.tsv"], stdin=MSA3)
    add("dist", ["--tree", "-", "absent.fsa"])
    add("dist", [], stdin=PHY3)
    add("dist", [], stdin="")
    add("dist", ["-y", "absent.txt"], stdin=MSA3)
    add("dist", ["--tree", "-", "-y", "absent.txt"], stdin=MSA3)
    add("dist", [], stdin=MSA_N)
    add("dist", ["-n", "n.out"], stdin=MSA_N)
    add("dist", ["-o", "nodir/out"], stdin=MSA3)
    add("dist", ["absent.fsa"])
    add("dist", ["-i", "absent.fsa", "-x", "3"])
    add("dist", ["-r", "a", "-o", "nodir/out", "a.fsa", "b.fsa"], files={"a.fsa": MSA1, "b.fsa": MSA1})
    add("dist", ["-r", "t", "-o", "nodir/out", "a.mat", "b.mat"], files={"a.mat": "#t\n", "b.mat": "#t\n"})
    add("dist", ["-r", "t", "-n", "nodir/n", "a.mat", "b.mat"], files={"a.mat": "#t\n", "b.mat": "#t\n"})
    add("tsv2phy", ["-s"], stdin=TSV2)
    add("tsv2phy", ["-b", "2"], stdin=TSV2)
    add("tsv2phy", ["-d", "nope"])
    add("tsv2phy", ["-d", "l2x"])
    add("tsv2phy", ["-d", "l0"])
    add("tsv2phy", ["-d", "l-1"])
    add("tsv2phy", ["-d", "l"])
    add("tsv2phy", ["-D"])
    add("tsv2phy", ["-d", "nope", "-D"])
    add("tsv2phy", ["--tree", "-", "--tree_method", "upgma"], stdin=TSV2)
    add("tsv2phy", ["--tree_method", "upgma"], stdin="")
    add("tsv2phy", ["--tree", "-"], stdin=TSV2)
    add("tsv2phy", ["--tree", "-"], stdin=TSV1)
    add("tsv2phy", ["--tree", "-"], stdin="")
    add("tsv2phy", [], stdin="")
    add("tsv2phy", [], stdin=TSV1)
    add("tsv2phy", ["-f", "0", "-x", "3"], stdin=TSV1)
    add("tsv2phy", ["-p", "-d", "l2"], stdin=TSV1)
    add("tsv2phy", ["-i", "t.tsv", "-o", "out.phy"], files={"t.tsv": TSV1})
    add("tsv2phy", ["-S", ",", "t.csv"], files={"t.csv": "1,2,3\n"})
    add("tsv2phy", [], stdin="1\t2\n3\n")
    add("tsv2phy", [], stdin="1\tx\n")
    add("tsv2phy", ["absent.tsv"])
    add("tsv2phy", ["-o", "nodir/out"], stdin=TSV1)
    add("tsv2phy", ["--tree", "nodir/t.nwk"], stdin=TSV2)
    add("nwck2phy", ["-s"])
    add("nwck2phy", ["-b", "2"])
    add("nwck2phy", ["absent.nwk"])
    add("nwck2phy", ["-o", "nodir/out"])
    add("nwck2phy", [], stdin="")
    add("nwck2phy", [], stdin="A;\n")
    add("nwck2phy", [], stdin="(A:1;\n")
    add("nwck2phy", ["-x", "3", "-f", "0"], stdin="A;\n")
    add("phycmp", ["-s"])
    add("phycmp", ["-b", "2"])
    add("phycmp", ["absent.phy"])
    add("phycmp", ["a.phy", "absent.phy"], files={"a.phy": PHY3})
    add("phycmp", ["-o", "nodir/out", "a.phy"], files={"a.phy": PHY3})
    add("phycmp", [], stdin="")
    add("phycmp", [], stdin=PHY3)
    add("phycmp", [], stdin=PHY3 + PHY2)
    add("phycmp", ["a.phy", "b.phy"], files={"a.phy": PHY3, "b.phy": PHY2})
    add("phycmp", ["a.phy", "b.phy"], files={"a.phy": PHY3, "b.phy": PHY3B})
    add("phycmp", ["a.phy", "b.phy"], files={"a.phy": PHY3, "b.phy": PHY3R})
    add("phycmp", ["--by_name", "a.phy", "b.phy"], files={"a.phy": PHY3, "b.phy": PHY3B})
    add("phycmp", ["--by_name", "-i", "a.phy", "b.phy"], files={"a.phy": PHY3, "b.phy": "3\nA\nA\t1\nC\t2\t3\n"})
    add("phycmp", [], stdin=PHY1 + PHY1)
    add("phycmp", ["--by_name"], stdin=PHY1 + PHY1)
    add("phycmp", ["-S", ","], stdin=PHY1 + "1\nother\n")
    add("merge", ["-s"])
    add("merge", ["-b", "2"])
    add("merge", ["--tree", "-", "--tree_method", "upgma"])
    add("merge", ["--tree_method", "upgma", "absent.phy"])
    add("merge", ["absent.phy"])
    add("merge", ["-w", "absent.phy"], stdin=PHY3)
    add("merge", ["-i", "a.phy", "-w", "absent.phy"], files={"a.phy": PHY3})
    add("tree", ["absent.phy"])
    add("tree", ["-o", "nodir/out"])
    add("tree", ["--phycmp", "nodir/cmp"], stdin=PHY3)
    add("tree", [], stdin="")
    add("tree", [], stdin=PHY1)
    add("tree", [], stdin=PHY2)
    add("tree", ["-x", "3", "-f", "1"], stdin=PHY2)
    add("tree", ["-i", "a.phy", "-o", "out.nwk"], files={"a.phy": PHY2})
    add("tree", ["-S", ",", "-q", "'"], stdin="2\n'A,1'\n'B',3.5\n")
    add("tree", ["-p"], stdin=PHY2)
    add("tree", ["-s", "0.01"], stdin=PHY2)
    add("tree", ["-b1"], stdin=PHY2 + PHY1)
    add("dbscan", ["absent.phy"])
    add("dbscan", ["-o", "nodir/out"])
    add("dbscan", [], stdin="")
    add("dbscan", ["-e", "2.5", "-N", "2", "-p"], stdin="")
    add("dbscan", ["-e", "1x"])
    add("dbscan", ["-N", "1.5"])

    # two faults on one line, in both orders: the first in argv order is the one reported
    add("tree", ["-x", "zz", "-Z"])
    add("tree", ["-Z", "-x", "zz"])
    add("tree", ["-x", "zz", "-o"])
    add("tree", ["--transport", "tcp", "-x", "zz"])
    add("tree", ["-x", "zz", "--transport", "tcp"])
    add("tree", ["-m", "nope", "--gpus", "-1"])       # post-parse order: -m before --gpus
    add("tree", ["--gpus", "-1", "-m", "nope"])
    add("tree", ["-F", "-m", "nope"])
    add("tree", ["-m", "nope", "-F"])
    add("tree", ["-s0", "-m", "upgma"])
    add("tree", ["a", "b", "-Z"])
    add("dist", ["-x", "zz", "-Z"])
    add("dist", ["-Z", "-x", "zz"])
    add("dist", ["-C", "101", "-s", "0"])             # post-parse order: --min_cov before the precision
    add("dist", ["-s", "0", "-C", "101"])
    add("dist", ["-d", "nope", "-a", "x"])
    add("dist", ["-a", "x", "-d", "nope"])
    add("dist", ["-F", "-C", "101"])
    add("dist", ["-L", "zz", "--transport", "tcp"])
    add("dist", ["--transport", "tcp", "-L", "zz"])
    add("merge", ["-x", "zz", "-Z"])
    add("merge", ["-Z", "-x", "zz"])
    add("merge", ["-s", "--tree_method", "upgma", "--tree", "-"])
    add("merge", ["--tree", "-", "--tree_method", "upgma", "-s"])
    add("merge", ["-F", "-s"])
    add("merge", ["-f", "zz", "one", "two"])
    add("merge", ["one", "two", "-f", "zz"])
    add("tsv2phy", ["-x", "zz", "-Z"])
    add("tsv2phy", ["-Z", "-x", "zz"])
    add("tsv2phy", ["-F", "-D"])
    add("tsv2phy", ["-D", "-s"])
    add("dbscan", ["-N", "zz", "-e", "zz"])
    add("dbscan", ["-e", "zz", "-N", "zz"])
    add("nwck2phy", ["-x", "zz", "--nope"])
    add("nwck2phy", ["--nope", "-x", "zz"])
    add("phycmp", ["-f", "zz", "-Z"])
    add("phycmp", ["-Z", "-f", "zz"])
    add("phycmp", ["-F", "-s"])
    return cases


def run(binary, case):
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in case["files"].items():
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        return subprocess.run([binary] + case["argv"], input=case["stdin"].encode(), capture_output=True, cwd=tmp,
                              timeout=60)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    binary = os.path.abspath(sys.argv[1])
    seen, cases = set(), []
    for c in build_cases():
        key = json.dumps(c, sort_keys=True)
        if key in seen:
            continue
        seen.add(key)
        p = run(binary, c)
        assert b"cannot open GPU" not in p.stderr, (c["argv"], p.stderr)
        assert p.returncode >= 0, (c["argv"], p.returncode, p.stderr)
        c.update(rc=p.returncode, stdout=p.stdout, stderr=p.stderr)
        cases.append(c)
    per = {cmd: sum(1 for c in cases if c["argv"][:1] == [cmd]) for cmd in OPTS}
    assert all(k >= 25 for k in per.values()) and len(cases) >= 250, (per, len(cases))
    for cmd in OPTS:   # -h and --help print the same bytes
        h = [c["stdout"] for c in cases if c["argv"] in ([cmd, "-h"], [cmd, "--help"])]
        assert len(h) == 2 and h[0] == h[1] and h[0], cmd
    # many cases answer with the same bytes (a help text, a message): each distinct output is stored
    # once in "texts", and a case holds the indices of its stdout and stderr
    texts = sorted({c[k] for c in cases for k in ("stdout", "stderr")})
    at = {t: i for i, t in enumerate(texts)}
    rows = []
    for c in cases:
        row = {"argv": c["argv"], "rc": c["rc"], "stdout": at[c["stdout"]], "stderr": at[c["stderr"]]}
        row.update({k: c[k] for k in ("stdin", "files") if c[k]})
        rows.append(json.dumps(row))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:   # one text and one case per line
        f.write('{"texts": [\n' + ",\n".join(json.dumps(enc(t)) for t in texts) + '\n],\n"cases": [\n' +
                ",\n".join(rows) + "\n]}\n")
    assert os.path.getsize(OUT) < 1024 * 1024
    print(len(cases), "cases", per, len(texts), "texts", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
