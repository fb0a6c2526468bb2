"""Python restatement of the reference's `nwck2phy` and `phycmp` arithmetic.

Newick side (nwck.c:157-359, nwck2phy.c:96-161): a literal parser that edits a
byte buffer exactly as getNwck / splitNwck / stripNwck / getLimbNwck do, node
by node as (start, len) pairs -- including the length of a peeled node, which
is one short until getLimbNwck finds a ':' -- and the driver loop that keeps
splitting names[org] until it no longer splits.  `replay` applies the split
list to a packed lower triangle cell by cell.

Comparison side (distcmp.c, phycmp.c:111-138): the per-cell terms with the C
types of the double and float functions, summed exactly (math.fsum), and the
closing expression of every metric.

Where the reference steps outside a node's own bytes (undefined behaviour) the
parser raises Refused; where it prints "Invalid limb length at node" and exits
it raises InvalidLimb.
"""
import math
import re

import numpy as np

SUM_NAMES = ("ab", "aa", "bb", "a", "b", "apb", "mn", "l1", "l2", "chi2", "linf")
METRIC_NAMES = ("cos", "chi2", "bc", "l1", "l2", "linf", "p")


class Refused(ValueError):
    """the literal bookkeeping would leave the node's bytes"""


class InvalidLimb(ValueError):
    """getLimbNwck's exit(1); args[0] is the node text the reference prints"""


def _cstr(buf, start):
    end = buf.index(0, start)
    return bytes(buf[start:end])


def _strtod(buf, start):
    """strtod on the NUL-terminated text at start: (value, index of the first unparsed byte)."""
    text = _cstr(buf, start)
    m = re.match(rb"[ \t\n\v\f\r]*[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf(?:inity)?|nan)", text, re.I)
    if not m:
        return 0.0, start
    return float(m.group(0).decode()), start + m.end()


class _Node:
    __slots__ = ("seq", "len")

    def __init__(self, seq=0, length=0):
        self.seq = seq
        self.len = length


def _scan_back(buf, base, length):
    """the backward walk of splitNwck from base + length: (stop, len) at its end"""
    if length > 512:
        return _scan_back_np(buf, base, length)
    return _scan_back_loop(buf, base, length)


def _scan_back_np(buf, base, length):
    """_scan_back_loop in array form (long nodes): the walk ends at the first
    byte, going backwards, that is '(' or ',' while stop == 0 -- stop being the
    '(' minus ')' count of the bytes behind it, which never exceeds 0 before."""
    w = np.frombuffer(buf, dtype=np.uint8, count=length, offset=base)[::-1]
    delta = (w == 0x28).astype(np.int64) - (w == 0x29)
    before = np.cumsum(delta) - delta
    hit = np.flatnonzero((before == 0) & ((w == 0x28) | (w == 0x2C)))
    if hit.size:
        return 1, length - 1 - int(hit[0])
    return int(delta.sum()), -1


def _scan_back_loop(buf, base, length):
    stop = 0
    seq = base + length
    while stop <= 0:
        length -= 1
        if length < 0:
            break
        seq -= 1
        c = buf[seq]
        if c == 0x29:
            stop -= 1
        elif c == 0x28:
            stop += 1
        elif c == 0x2C and stop == 0:
            stop += 1
    return stop, length


def _limb(buf, node):
    length = node.len
    seq = node.seq + length
    if length == 0:
        return -1.0
    length -= 1
    seq -= 1
    if buf[seq] == 0x29:
        return -1.0
    while True:
        length -= 1
        if length == 0:
            break
        if length < 0:
            raise Refused("limb search leaves node: " + _cstr(buf, node.seq).decode("latin-1"))
        seq -= 1
        if buf[seq] == 0x3A:
            break
    if length:
        buf[seq] = 0
        node.len = length
        L, end = _strtod(buf, seq + 1)
        if buf[end] != 0:
            raise InvalidLimb(_cstr(buf, node.seq).decode("latin-1"))
        return L
    return -1.0


def _split(buf, ni, nj):
    """splitNwck: None, or (Li, Lj) with ni / nj updated"""
    while True:
        length = ni.len
        if not length:
            return None
        stop, length = _scan_back(buf, ni.seq, length)
        if stop == 0:
            # stripNwck
            if buf[ni.seq] == 0x28 and buf[ni.seq + ni.len - 1] == 0x29:
                ni.len -= 2
                ni.seq += 1
                buf[ni.seq + ni.len] = 0
                if ni.len:
                    continue
            return None
        if length < 0:
            raise Refused("unbalanced node: " + _cstr(buf, ni.seq).decode("latin-1"))
        buf[ni.seq + length] = 0
        nj.len = ni.len - length - 2
        nj.seq = ni.seq + length + 1
        ni.len = length
        if nj.len < 0:
            raise Refused("empty node after: " + _cstr(buf, ni.seq).decode("latin-1"))
        stop, _ = _scan_back(buf, ni.seq, length)
        if stop != 0:
            Li = 0.0
            Lj = _limb(buf, nj)
        else:
            Li = _limb(buf, ni)
            Lj = _limb(buf, nj)
            if Lj < 0 and 0 <= Li:
                Lj = 0.0
        return Li, Lj


def parse_line(line):
    """One input line (bytes without the newline; the header is what precedes
    the first '(').  Returns (header, names, splits): names in row order as
    the reference prints them, splits a list of (org, Li, Lj)."""
    line = bytes(line)
    p = line.find(b"(")
    if p < 0:
        raise Refused("no '(' in line")
    header = line[:p]
    body = line[p + 1:]
    q = body.rfind(b")")
    if q < 1:
        raise Refused("no node between '(' and ')'")
    buf = bytearray(body) + b"\0"
    buf[q] = 0
    n = 1 + body[:q].count(b",")
    nodes = [_Node(0, q)]
    splits = []
    org = 0
    while len(nodes) != n:
        if org >= len(nodes):
            raise Refused("more commas than nodes")
        nj = _Node()
        r = _split(buf, nodes[org], nj)
        if r is None:
            org += 1
        else:
            nodes.append(nj)
            splits.append((org, r[0], r[1]))
    names = [_cstr(buf, nd.seq) for nd in nodes]
    return header, names, splits


def parse_file(data):
    """getNwck over a whole file: a list of (header, names, splits) or of the
    exception that ends the run there (nothing follows it)."""
    out = []
    pos = 0
    while True:
        p = data.find(b"(", pos)
        if p < 0:
            break
        e = data.find(b"\n", p)
        if e < 0:
            break
        try:
            out.append(parse_line(data[pos:e]))
        except (Refused, InvalidLimb) as ex:
            out.append(ex)
            break
        pos = e + 1
    return out


def tri(i):
    return i * (i - 1) // 2


def replay(splits, etype=8):
    """The packed LT of n = len(splits) + 1 rows (nwck2phy.c:99-225)."""
    dt = np.float64 if etype == 8 else np.float32
    n = len(splits) + 1
    D = np.zeros(tri(n), dtype=dt)

    def at(i, j):
        return tri(i) + j if j < i else tri(j) + i

    for s, (org, Li, Lj) in enumerate(splits):
        m = s + 1
        old = [float(D[at(org, k)]) if k != org else 0.0 for k in range(m)]
        for k in range(m):
            c = old[k]
            if Lj < 0:
                D[tri(m) + k] = dt(Lj)
            elif k == org:
                D[tri(m) + k] = dt(Lj + Li)
            else:
                D[tri(m) + k] = dt(-1.0) if c < 0 else dt(Lj + c)
            if k != org:
                if Li < 0:
                    D[at(org, k)] = dt(Li)
                elif c >= 0:
                    D[at(org, k)] = dt(c + Li)
    return D


def replay_np(splits, etype=8):
    """replay with numpy row operations (the same roundings), for large trees"""
    dt = np.float64 if etype == 8 else np.float32
    n = len(splits) + 1
    M = np.zeros((n, n), dtype=dt)   # symmetric working copy
    for s, (org, Li, Lj) in enumerate(splits):
        m = s + 1
        c = M[org, :m].astype(np.float64)
        if Lj < 0:
            new = np.full(m, dt(Lj), dtype=dt)
        else:
            new = np.where(c < 0, -1.0, Lj + c).astype(dt)
            new[org] = dt(Lj + Li)
        if Li < 0:
            upd = np.full(m, dt(Li), dtype=dt)
        else:
            upd = np.where(c >= 0, c + Li, c).astype(dt)
        upd[org] = 0
        M[org, :m] = upd
        M[:m, org] = upd
        M[m, :m] = new
        M[:m, m] = new
    iu = np.tril_indices(n, -1)
    return np.ascontiguousarray(M[iu])


# ---------------------------------------------------------------- comparison
def cmp_terms(A, B, etype=8):
    """The per-cell terms of distcmp.c as double arrays, in SUM_NAMES order
    (linf's are |a - b|).  Float rows multiply, add, subtract and take the
    minimum in float before widening."""
    dt = np.float64 if etype == 8 else np.float32
    a = np.ascontiguousarray(A, dtype=dt)
    b = np.ascontiguousarray(B, dtype=dt)
    w = np.float64
    diff = (a - b).astype(w)
    apb = (a + b).astype(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        chi = np.where(diff != 0, diff * diff / apb, 0.0)
    return {
        "ab": (a * b).astype(w), "aa": (a * a).astype(w), "bb": (b * b).astype(w),
        "a": a.astype(w), "b": b.astype(w), "apb": apb,
        "mn": np.where(a < b, a, b).astype(w),
        "l1": np.abs(diff), "l2": diff * diff, "chi2": chi, "linf": np.abs(diff),
    }


def cmp_sums(A, B, etype=8):
    """(sums, abs_sums): each sum exactly rounded (math.fsum), and the sum of
    |term| that scales the engine's error bound; linf is the maximum."""
    t = cmp_terms(A, B, etype)
    sums, mags = {}, {}
    for k in SUM_NAMES:
        if k == "linf":
            sums[k] = float(t[k].max())
            mags[k] = 0.0
        else:
            sums[k] = math.fsum(t[k])
            mags[k] = math.fsum(np.abs(t[k]))
    return sums, mags


def _sqrt(x):
    """C's sqrt: NaN for a negative sum (missing cells can make one), no exception"""
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(x)))


def metric(s, cells, which):
    """Closes metric `which` (METRIC_NAMES) from the sums as phycmp does."""
    if which == "cos":
        if not s["aa"] or not s["bb"]:
            return -1.0
        d = 1 - s["ab"] / _sqrt(s["aa"] * s["bb"])
        return 0.0 if d < 0 else d
    if which == "chi2":
        return _sqrt(s["chi2"])
    if which == "bc":
        with np.errstate(all="ignore"):
            d = float(1 - 2 * np.float64(s["mn"]) / np.float64(s["apb"]))
        return 0.0 if d < 0 else d
    if which == "l1":
        return s["l1"]
    if which == "l2":
        return _sqrt(s["l2"])
    if which == "linf":
        return s["linf"]
    if which == "p":
        v11 = s["aa"] - s["a"] * s["a"] / cells
        v12 = s["ab"] - s["a"] * s["b"] / cells
        v22 = s["bb"] - s["b"] * s["b"] / cells
        if not v11 or not v22:
            return 0.0
        with np.errstate(all="ignore"):
            return float(np.float64(v12) / np.float64(_sqrt(v11 * v22)))
    raise KeyError(which)


def phycmp_lines(s, cells, flag):
    out = []
    for bit, name in enumerate(METRIC_NAMES):
        if flag & (1 << bit):
            d = metric(s, cells, name)
            if math.isnan(d):   # glibc prints the sign of a NaN (0 / 0 on x86 sets it)
                out.append("%s:\t%s\n" % (name, "-nan" if math.copysign(1.0, d) < 0 else "nan"))
            else:
                out.append("%s:\t%f\n" % (name, d))
    return "".join(out)


def permute_lt(B, n, perm):
    """B'[i, j] = B[perm[i], perm[j]] as a packed LT"""
    i, j = np.tril_indices(n, -1)
    pi, pj = np.asarray(perm)[i], np.asarray(perm)[j]
    hi, lo = np.maximum(pi, pj), np.minimum(pi, pj)
    return np.ascontiguousarray(np.asarray(B)[hi * (hi - 1) // 2 + lo])


# ---------------------------------------------------------------- text
def print_phy(header, names, D, flag=1, precision=9):
    """printphy (phy.c:59) of a packed LT with relaxed names (flag bit 1; bit 4
    adds the comment line): integral cells as integers, the others %.*f."""
    n = len(names)
    out = []
    if flag & 4:
        out.append(b"#" + header + b"\n")
    out.append(b"%10d\n" % n)
    k = 0
    for i in range(n):
        row = [names[i]]
        for j in range(i):
            d = float(D[k + j])
            if -2147483649.0 < d < 2147483648.0 and d == int(d):
                row.append(b"%d" % int(d))
            else:
                row.append(("%.*f" % (precision, d)).encode())
        k += i
        out.append(b"\t".join(row) + b"\n")
    return b"".join(out)


def nwck2phy(data, etype=8, flag=1):
    """The reference's `nwck2phy` on a whole file: (stdout, exit status, stderr)."""
    out = []
    for r in parse_file(data):
        if isinstance(r, InvalidLimb):
            return b"".join(out), 1, b"Invalid limb length at node:\t" + r.args[0].encode("latin-1") + b"\n"
        if isinstance(r, Refused):
            return b"".join(out), None, str(r).encode()
        header, names, splits = r
        D = replay(splits, etype) if len(splits) < 64 else replay_np(splits, etype)
        out.append(print_phy(header, names, D, flag))
    return b"".join(out), 0, b""
