"""A numpy restatement of `ccphylo tsv2phy` (ref tsv2phy.c:35, tsv.c:30 and the
*_d / *_f functions of distcmp.c): the table reader, the cells and the Phylip
text.

The cells are computed serially over the columns and vectorised over the
pairs, so that every operation is ONE IEEE elementwise operation in the
reference's order: every accumulator starts from column 0's term, products,
differences and sums of two floats are rounded to float32 before they are
widened (`-p`, float32 input), and the closing expressions are written as the
reference writes them.  numpy's +, -, *, / and sqrt are correctly rounded and
never fused, so finite results equal the reference's bit for bit -- except
l<n>, whose pow() differs from libm's in the last places."""
import gzip
import json
import os

import numpy as np

METRICS = ("cos", "chi2", "bc", "l1", "l2", "linf", "p")   # the bit-exact ones


def parse_metric(name):
    """-d name -> (kind, exponent): "l3" / "l2.5" are ("ln", 3.0 / 2.5)."""
    if name in METRICS:
        return name, 0.0
    if name.startswith("l") and len(name) > 1:
        return "ln", float(name[1:])
    raise ValueError(name)


def read_tsv(path, sep="\t", vtype=8):
    """loadTsv: header dropped, then lines while the next starts with '#'; the
    column count is 1 + the separators after the first byte of the last
    dropped line; every further line is one row."""
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    with op(path, "rb") as f:
        data = f.read().decode()
    assert data.endswith("\n") or not data
    lines = data.split("\n")[:-1]
    k = 0
    while True:
        if k >= len(lines):
            return np.zeros((0, 1))
        n = 1 + lines[k][1:].count(sep)
        k += 1
        if k >= len(lines):
            return np.zeros((0, n))
        if not lines[k].startswith("#"):
            break
    rows = [[float(t) if t else 0.0 for t in ln.split(sep)] for ln in lines[k:]]
    X = np.array(rows, dtype=np.float64).reshape(len(rows), n)
    return X.astype(np.float32) if vtype == 4 else X


def vec_ltd(X, metric, exponent=0.0):
    """The packed LT (float64, row i holds (i,0) .. (i,i-1)) of distcmp_d
    (float64 X) or distcmp_f (float32 X) over the rows of X."""
    X = np.asarray(X)
    assert X.dtype in (np.float64, np.float32) and X.ndim == 2
    m, n = X.shape
    i, j = np.tril_indices(m, -1)   # row-major: the reference's cell order
    f64 = np.float64
    A, B = X[i], X[j]               # v1 = row i, v2 = row j
    P = len(i)
    d = np.zeros(P)
    s = np.zeros(P)
    c1 = np.zeros(P)
    c2 = np.zeros(P)
    e1 = np.zeros(P)
    e2 = np.zeros(P)
    with np.errstate(all="ignore"):
        for k in range(n):
            x, y = A[:, k], B[:, k]
            first = k == 0
            if metric in ("cos", "p"):
                t, t1, t2 = (x * y).astype(f64), (x * x).astype(f64), (y * y).astype(f64)
                d = t if first else d + t
                c1 = t1 if first else c1 + t1
                c2 = t2 if first else c2 + t2
                if metric == "p":
                    e1 = x.astype(f64) if first else e1 + x.astype(f64)
                    e2 = y.astype(f64) if first else e2 + y.astype(f64)
            elif metric == "bc":
                t, u = np.where(x < y, x, y).astype(f64), (x + y).astype(f64)
                d = t if first else d + t
                s = u if first else s + u
            elif metric == "chi2":
                T = (x - y).astype(f64)
                t = T * T / (x + y).astype(f64)
                d = np.where(T != 0, t, 0.0) if first else np.where(T != 0, d + t, d)
            elif metric == "linf":
                t = (x - y).astype(f64)
                d = np.where(t < 0, -t, t) if first else np.where(d < t, t, np.where((t < 0) & (d < -t), -t, d))
            else:
                t = (x - y).astype(f64)
                u = np.where(t < 0, -t, t)
                if metric == "l2":
                    u = t * t
                elif metric == "ln":
                    u = np.power(u, exponent)
                else:
                    assert metric == "l1", metric
                d = u if first else d + u
        if metric == "cos":
            r = 1 - d / np.sqrt(c1 * c2)
            return np.where((c1 == 0) | (c2 == 0), -1.0, np.where(r < 0, 0.0, r))
        if metric == "p":
            nn = f64(n)
            v11 = c1 - e1 * e1 / nn
            v12 = d - e1 * e2 / nn
            v22 = c2 - e2 * e2 / nn
            return np.where((v11 == 0) | (v22 == 0), 0.0, v12 / np.sqrt(v11 * v22))
        if metric == "bc":
            r = 1 - 2 * d / s
            return np.where(r < 0, 0.0, r)
        if metric in ("l2", "chi2"):
            return np.sqrt(d)
        if metric == "ln":
            r = np.power(d, 1.0 / exponent)
            return np.where(r < 0, 0.0, r)
        return d


def format_phy(D, m, flag=1, precision=9):
    """tsv2phy.c:64-108: "%10d", per row "\\n%d" (flag & 1) or "\\n%-10d" and
    the cells "\\t%.*g", a closing newline."""
    out = ["%10d" % m]
    f = 0
    for i in range(m):
        out.append(("\n%d" if flag & 1 else "\n%-10d") % i)
        out.extend("\t%.*g" % (precision, float(v)) for v in D[f:f + i])
        f += i
    out.append("\n")
    return "".join(out).encode()


def parse_phy(data):
    """(m, packed LT) of a tsv2phy output."""
    lines = data.decode().split("\n")
    m = int(lines[0])
    cells = []
    for i in range(m):
        tok = lines[1 + i].split("\t")
        assert tok[0].strip() == str(i) and len(tok) == i + 1, (i, tok[:2])
        cells.extend(float(t) for t in tok[1:])
    return m, np.array(cells, dtype=np.float64)


# ------------------------------------------------------------------ goldens
TSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsv")
CASES = []   # (empty only while gen_tsv_golden.py writes the first set)
if os.path.exists(os.path.join(TSV, "tsv.json")):
    with open(os.path.join(TSV, "tsv.json")) as _f:
        CASES = json.load(_f)["cases"]
PHY = [c for c in CASES if "tree" not in c]


def case_options(args):
    """tsv2phy CLI args of a golden case -> dict."""
    o = dict(inp=None, d="cos", sep="\t", vtype=8, prec=9, flag=1)
    k = 1
    while k < len(args):
        a = args[k]
        if a == "-i": o["inp"] = args[k + 1]; k += 1
        elif a == "-d": o["d"] = args[k + 1]; k += 1
        elif a == "-S": o["sep"] = args[k + 1]; k += 1
        elif a == "-x": o["prec"] = int(args[k + 1]); k += 1
        elif a == "-f": o["flag"] = int(args[k + 1]); k += 1
        elif a == "-p": o["vtype"] = 4
        k += 1
    return o


def case_bytes(case):
    with open(os.path.join(TSV, case["out"]), "rb") as f:
        return f.read()
