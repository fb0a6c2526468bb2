"""A numpy restatement of the reference's `ccphylo merge` (merge.c:122 merge,
:309 jl_merge, :47 normalize_ltdMatrix), pinned to the reference's bytes by
tests/golden/merge (test_merge_oracle.py) and used as the expected value of the
GPU engine (test_gpu_merge.py).

A name gets the next union index at its first appearance.  A cell of the first
matrix starts as D = d * w, N = w (d and 1 without weights); every later matrix,
in file order, does D[hi][lo] += d * w, N[hi][lo] += w with hi / lo the larger /
smaller union index, every step rounded in the element type; rows added later
start at +0.  The close is D = N != 0 ? D / N : -1.  A matrix touches a union
cell at most once, so a fancy-indexed += is the reference's loop.

The reference itself is only reliable while the first matrix has at most 63
entries and the union at most 126 names (merge.c:138 sizes its work matrices
before the first load; hashmapstrindex.c:30 can register a name twice from the
127th on).  Outside that envelope this file is the definition: a correct name
map, in insertion order."""
import numpy as np

DTYPES = {8: np.float64, 4: np.float32}
CONCUR = b"Distance and included nucleotides does not concur!\n"


class Refused(Exception):
    """an input the engine's CLI refuses (a name twice in one matrix)"""


def tri(i):
    return i * (i - 1) // 2


def union_cells(idx):
    """flat union cell of every cell of a source with union rows idx, in packed order"""
    idx = np.asarray(idx, dtype=np.int64)
    i, j = np.tril_indices(len(idx), -1)
    a, b = idx[i], idx[j]
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    return hi * (hi - 1) // 2 + lo


def apply(D, N, d, w, idx, first=False):
    """one source into accumulators of the element type, in place"""
    dt = D.dtype.type
    d = np.asarray(d, dtype=dt)
    f = union_cells(idx)
    assert len(np.unique(np.asarray(idx))) == len(idx) and len(d) == len(f)
    if w is None:
        p, one = d, np.ones(len(f), dtype=dt)
    else:
        one = np.asarray(w, dtype=dt)
        p = d * one            # rounded in the element type before the sum
    if first:
        D[f] = p
        N[f] = one
    else:
        D[f] = D[f] + p
        N[f] = N[f] + one


def close(D, N):
    """normalize_ltdMatrix: a new D; N stays"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(N != 0, D / N, D.dtype.type(-1)).astype(D.dtype)


def grow(A, n):
    """the accumulator with rows up to n, new cells +0"""
    return np.concatenate([A, np.zeros(tri(n) - len(A), dtype=A.dtype)]) if tri(n) > len(A) else A


# ---------------------------------------------------------------- text
def parse_multi(data, etype=8, sep=b"\t"):
    """loadPhy (phy.c:251) over a whole file: [(names, packed cells)] up to the
    end of the input or a size of 0.  A name runs to the first separator or
    newline; trailing white space is cut, so a non-blank separator stays."""
    dt = DTYPES[etype]
    mats = []
    pos = 0
    while pos < len(data):
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
        if pos >= len(data):
            break
        end = data.index(b"\n", pos)
        digits = bytes(c for c in data[pos:end] if 48 <= c <= 57)
        n = int(digits) if digits else 0
        pos = end + 1
        if n == 0 or pos >= len(data):
            break
        names, cells = [], []
        for i in range(n):
            end = data.find(b"\n", pos)
            line = data[pos:end if end >= 0 else len(data)]
            pos = end + 1 if end >= 0 else len(data)
            k = line.find(sep)
            name = line if k < 0 else line[:k + 1]
            names.append(name.rstrip())
            toks = [t for t in line[k + 1:].split(sep) if t] if k >= 0 else []
            assert len(toks) >= i, (i, line)
            cells += [float(t) for t in toks[:i]]
        mats.append((names, np.array(cells, dtype=np.float64).astype(dt)))
    return mats


def print_phy(names, D, flag=1, precision=9, comment=b"Merged"):
    """printphy (phy.c:59): integral cells as integers, the others %.*f; flag
    bit 1 relaxed names (else %-10.10s), bit 4 the comment line"""
    n = len(names)
    out = []
    if flag & 4:
        out.append(b"#" + comment + b"\n")
    out.append(b"%10d\n" % n)
    k = 0
    for i in range(n):
        row = [names[i] if flag & 1 else b"%-10.10s" % names[i]]
        for j in range(i):
            d = float(D[k + j])
            if -2147483649.0 < d < 2147483648.0 and d == int(d):
                row.append(b"%d" % int(d))
            else:
                row.append(("%.*f" % (precision, d)).encode())
        k += i
        out.append(b"\t".join(row) + b"\n")
    return b"".join(out)


# ---------------------------------------------------------------- whole runs
def merge(mats, wmats=None, etype=8):
    """(names, D, N) of the reference's merge over parsed matrices; with wmats
    the names are the weights file's.  Raises ValueError(CONCUR) where the
    reference exits 1, Refused for a name twice in one matrix."""
    dt = DTYPES[etype]
    index, names = {}, []
    D, N = np.zeros(0, dtype=dt), np.zeros(0, dtype=dt)
    for k, (nm, d) in enumerate(mats):
        w = None
        if wmats is not None:
            if k >= len(wmats) or len(wmats[k][0]) != len(nm):
                raise ValueError(CONCUR)
            nm, w = wmats[k]
        idx = []
        for r, name in enumerate(nm):
            if name not in index:
                index[name] = len(names)
                names.append(name)
            if index[name] in idx:
                raise Refused("matrix %d holds the name %r twice, on rows %d and %d" % (k + 1, name, idx.index(index[name]) + 1, r + 1))
            idx.append(index[name])
        D, N = grow(D, len(names)), grow(N, len(names))
        apply(D, N, d, w, idx, first=k == 0)
    return names, D, N


def run(data, wdata=None, etype=8, flag=1, precision=9, sep=b"\t"):
    """`ccphylo merge` on file contents: (exit status, stderr, D text, N text or None)"""
    mats = parse_multi(data, etype, sep)
    wmats = parse_multi(wdata, etype, sep) if wdata is not None else None
    try:
        names, D, N = merge(mats, wmats, etype)
    except ValueError as e:
        return 1, e.args[0], b"", None
    D = close(D, N)
    return (0, b"", print_phy(names, D, flag, precision),
            print_phy(names, N, flag, precision) if wdata is not None else None)
