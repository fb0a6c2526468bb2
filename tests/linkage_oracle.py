"""ctypes view of tests/linkage_oracle.c, the serial CPU restatement of the
reference's tree methods upgma, cf, ff and mn.  The C file is compiled on
first use into a temporary directory (gcc, -ffp-contract=off).

TEST INFRASTRUCTURE ONLY: the checker of tests/test_linkage_oracle.py and
tests/test_gpu_linkage.py -- never imported by ccphylo_amd/.
"""
import atexit
import ctypes as C
import json
import os
import shutil
import subprocess
import tarfile
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ETYPES = {8: np.float64, 4: np.float32, 2: np.uint16, 1: np.uint8}
JOIN_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("Li", np.float64), ("Lj", np.float64)])
UPGMA, CF, FF, MN = 3, 4, 5, 6
METHODS = {"upgma": UPGMA, "cf": CF, "ff": FF, "mn": MN}

_lib = None


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="linkage_oracle_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "liblinkage_oracle.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-Wall",
                        "-Wno-unused-function", "-shared", "-o", so, os.path.join(HERE, "linkage_oracle.c"),
                        "-lpthread", "-lm", "-lz"], check=True)
        L = C.CDLL(so)
        L.lk_tree.argtypes = [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                              C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p, C.c_int]
        L.lk_tree.restype = C.c_int
        _lib = L
    return _lib


def tree(D, n, etype=8, byte_scale=1.0, method=UPGMA, flags=0, stats=False, max_joins=0):
    """Serial upgma (3) / cf (4) / ff (5) / mn (6) exactly as the reference at
    -t 1.  Returns (joins, final_n, final_d[, stats]) as oracle.pyoracle.tree
    does; stats = (rows, cells) that UPGMApair rescanned."""
    D = np.array(D, dtype=ETYPES[etype], copy=True)
    cap = min(n, max_joins) if max_joins > 0 else n
    joins = np.zeros(max(cap, 1), dtype=JOIN_DTYPE)
    fn = C.c_int(0)
    fd = C.c_double(0)
    st = np.zeros(2, dtype=np.int64)
    nj = lib().lk_tree(n, etype, byte_scale, D.ctypes.data, method, flags, joins.ctypes.data, C.byref(fn),
                       C.byref(fd), st.ctypes.data, max_joins)
    if nj < 0:
        raise ValueError(f"method {method}")
    res = (joins[:nj], fn.value, fd.value)
    return res + (st,) if stats else res


def parse_tree_args(args):
    """tree CLI args of a golden_linkage.json case -> (input, method id, etype, bs, flags, precision)."""
    golden = os.path.join(HERE, "golden")
    inp, method, et, bs, flags, prec = None, None, 8, 1.0, 0, 9
    k = 1
    while k < len(args):
        a = args[k]
        if a == "-i":
            inp = args[k + 1]; k += 1
        elif a == "-m":
            method = METHODS[args[k + 1]]; k += 1
        elif a == "-p":
            et = 4
        elif a in ("-s", "-b"):
            et = 2 if a == "-s" else 1
            if k + 1 < len(args) and not args[k + 1].startswith("-"):
                bs = float(args[k + 1]); k += 1
        elif a == "-f":
            flags = int(args[k + 1]); k += 1
        elif a == "-x":
            prec = int(args[k + 1]); k += 1
        k += 1
    return os.path.join(golden, inp), method, et, bs, flags, prec


# ---------------------------------------------------------------- inputs
def golden_out(case):
    """The reference's bytes of a golden_linkage.json case (a member of golden_linkage_out.tar.gz or, for the
    adversarial matrices, of golden_linkage_adv_out.tar.gz)."""
    if not _OUT:
        for arc in ("golden_linkage_out.tar.gz", "golden_linkage_adv_out.tar.gz"):
            with tarfile.open(os.path.join(HERE, "golden", arc)) as t:
                for m in t.getmembers():
                    _OUT[m.name] = t.extractfile(m).read()
    return _OUT[case["out"]]


_OUT = {}


def linkage_cases(methods=None):
    with open(os.path.join(HERE, "golden", "golden_linkage.json")) as f:
        cases = json.load(f)["cases"]
    return [c for c in cases if methods is None or c["method"] in methods]


def write_phylip(path, D, n, fmt="%.9f"):
    """A packed LT as the Phylip text `ccphylo tree` reads (phy.c:275)."""
    with open(path, "w") as f:
        f.write("%10d\n" % n)
        k = 0
        for i in range(n):
            f.write("\t".join([f"t{i}"] + [fmt % v for v in D[k:k + i]]) + "\n")
            k += i
