"""Serial CPU restatement of the reference's dbscan (dbscan.c:31-163) on a
packed lower-triangular matrix, and the parallel form the GPU engine runs
(DESIGN.md "dbscan"), both in numpy.

TEST INFRASTRUCTURE ONLY: the checker of tests/test_dbscan_oracle.py and
tests/test_gpu_dbscan.py -- never imported by ccphylo_amd/.
"""
import numpy as np

ETYPES = {8: np.float64, 4: np.float32, 2: np.uint16, 1: np.uint8}


def cells_as_double(D, etype=8, byte_scale=1.0):
    """The cells as dbscan.c:65 reads them: etype 8 / 4 converted to double,
    etype 2 / 1 divided by ByteScale (uctod, bytescale.h:23)."""
    d = np.asarray(D, dtype=ETYPES[etype]).astype(np.float64)
    return d / np.float64(byte_scale) if etype <= 2 else d


def dbscan(D, n, max_dist=10.0, min_neighbors=1, etype=8, byte_scale=1.0, want_border=False):
    """The reference's two walks over the rows, in its order.  Returns
    (N, C, nclust), plus the number of border rows (0 < N[i] < minN) with
    want_border."""
    d = cells_as_double(D, etype, byte_scale)
    assert d.size == n * (n - 1) // 2
    N = np.zeros(n, dtype=np.int64)
    C = np.arange(n, dtype=np.int64)
    # first walk: a cell at or below the threshold counts for its row and its column
    nbs = []
    for i in range(n):
        nb = d[i * (i - 1) // 2:i * (i - 1) // 2 + i] <= max_dist
        nbs.append(np.flatnonzero(nb))
        N[i] += len(nbs[i])
        N[nbs[i]] += 1
    # second walk: every row takes the cluster of an earlier row, or stays its own
    nclust = 0
    border = 0
    for i in range(n):
        c = i
        if min_neighbors <= N[i]:
            # a core row: the scan runs while j < c, so the first neighbour ends it
            if len(nbs[i]):
                c = C[nbs[i][0]]
        elif N[i]:
            # a border row: the first core neighbour; the countdown of the
            # neighbours seen only ends the scan early
            border += 1
            left = N[i]
            for j in nbs[i]:
                if min_neighbors <= N[j]:
                    c = C[j]
                    break
                left -= 1
                if not left:
                    break
        if c != i:
            C[i] = c
        else:
            nclust += 1
    res = (N.astype(np.int32), C.astype(np.int32), nclust)
    return res + (border,) if want_border else res


def dbscan_parallel(D, n, max_dist=10.0, min_neighbors=1, etype=8, byte_scale=1.0):
    """The order-free form: N from one pass, f(i) per row, C by pointer
    jumping.  Returns (N, C, nclust, rounds)."""
    d = cells_as_double(D, etype, byte_scale)
    nb = np.zeros((n, n), dtype=bool)
    nb[np.tril_indices(n, -1)] = d <= max_dist      # row-major order of the packed LT
    N = nb.sum(1) + nb.sum(0)
    core = min_neighbors <= N
    f = np.arange(n)
    any_nb = nb.any(1)
    first_any = nb.argmax(1)
    nbc = nb & core[None, :]
    any_core = nbc.any(1)
    first_core = nbc.argmax(1)
    take_any = core & any_nb
    f[take_any] = first_any[take_any]
    take_core = ~core & (N > 0) & any_core
    f[take_core] = first_core[take_core]
    rounds = 0
    while True:
        rounds += 1
        g = f[f]
        if (g == f).all():
            break
        f = g
    return N.astype(np.int32), f.astype(np.int32), int((f == np.arange(n)).sum()), rounds


def format_table(names, N, C, nclust, max_dist, min_neighbors, header=None):
    """print_dbscan (dbscan.c:165) and the header line of dbscan.c:220, as bytes."""
    out = []
    if header:
        out.append("#%s\n" % header)
    out.append("## %d\t%d\t%f\t%d\n" % (len(names), nclust, max_dist, min_neighbors))
    out.append("#Sample\tNeighbors\tCluster\n")
    out += ["%s\t%d\t%d\n" % (s, a, b) for s, a, b in zip(names, N, C)]
    return "".join(out).encode()


def parse_table(text):
    """The bytes `ccphylo dbscan` prints -> [(header or None, n, nclust, names, N, C)]."""
    blocks, lines, k = [], text.decode().split("\n"), 0
    while k < len(lines) and lines[k]:
        header = None
        if not lines[k].startswith("## "):
            header = lines[k][1:]
            k += 1
        n, nclust = (int(x) for x in lines[k][3:].split("\t")[:2])
        rows = [ln.split("\t") for ln in lines[k + 2:k + 2 + n]]
        blocks.append((header, n, nclust, [r[0] for r in rows], [int(r[1]) for r in rows], [int(r[2]) for r in rows]))
        k += 2 + n
    return blocks


def golden_cases():
    """The cases of tests/golden/dbscan/dbscan.json (gen_dbscan_golden.py), each with its expected bytes."""
    import json
    import os
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan")
    with open(os.path.join(gdir, "dbscan.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        with open(os.path.join(gdir, c["out"]), "rb") as f:
            c["bytes"] = f.read()
    return cases


def case_options(args):
    """The command line of a golden case -> (max_dist, min_neighbors, etype, byte_scale)."""
    e, minn, et, bs = 10.0, 1, 8, 1.0
    k = 1
    while k < len(args):
        a = args[k]
        if a == "-e":
            e = float(args[k + 1]); k += 1
        elif a == "-N":
            minn = int(args[k + 1]); k += 1
        elif a == "-i":
            k += 1
        elif a == "-p":
            et = 4
        elif a in ("-s", "-b"):
            et = 2 if a == "-s" else 1
            if k + 1 < len(args) and not args[k + 1].startswith("-"):
                bs = float(args[k + 1]); k += 1
        k += 1
    return e, minn, et, bs
