"""A numpy / Python restatement of `ccphylo dist -y` (methylation motif
masking): the motif file parser (methparse.c:254 getMethMotifs), strrcMeth
(methparse.c:84) as it is, the site rule (meth.c:76 / :122 / :141) and where
ltdMsaMatrix_get (cdist.c:196-322) applies it.  The motif parts are written
here from scratch; the parts of the loader that `-y` does not touch (the code
table, packing, the N / gap / -P mask update, getNpos) come from the host
library's long-standing primitives, the all-pairs counts from oracle/pyoracle.

tests/test_meth_oracle.py pins this module to the reference's bytes
(tests/golden/meth); tests/test_gpu_meth.py compares the engine with it."""
import ctypes as C
import gzip
import os

import numpy as np

MOTIF_DTYPE = np.dtype([("len", np.int32), ("meth", np.uint32), ("allow", np.uint8, (32,))])
IUPAC = {"a": 1, "c": 2, "g": 4, "t": 8, "u": 8, "r": 5, "y": 10, "s": 6, "w": 9, "k": 12, "m": 3, "b": 14, "d": 13,
         "h": 11, "v": 7, "x": 15, "n": 15}


class MotifRefused(ValueError):
    pass


def _code(byte):
    ch = chr(byte)
    if ch.lower() in IUPAC and ch.isascii():
        return IUPAC[ch.lower()] | (16 if ch.isupper() else 0)
    return None


def motif_records(data):
    """[(name, [5-bit codes])]: a header line, then every IUPAC letter up to the next '>'."""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    recs, p = [], 0
    while p < len(data):
        name = b""
        if data[p:p + 1] == b">":
            e = data.find(b"\n", p)
            e = len(data) if e < 0 else e
            name = data[p + 1:e].replace(b"\r", b"")
            p = min(e + 1, len(data))
        e = data.find(b">", p)
        e = len(data) if e < 0 else e
        recs.append((name.decode("latin-1"), [c for c in map(_code, data[p:e]) if c is not None]))
        p = e
    return recs


def comp(c):
    return (c & 16) | ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3)


def strrc(q):
    """strrcMeth: pairs swapped and complemented from the ends inward; an odd
    length then complements the last LEFT element written again, so the middle
    base stays as written and its left neighbour ends up uncomplemented."""
    q = list(q)
    n = len(q)
    for i in range(n // 2):
        q[i], q[n - 1 - i] = comp(q[n - 1 - i]), comp(q[i])
    if n & 1:
        q[n // 2 - 1] = comp(q[n // 2 - 1])
    return q


def motif_text(q):
    inv = {1: "a", 2: "c", 4: "g", 8: "t", 5: "r", 10: "y", 6: "s", 9: "w", 12: "k", 3: "m", 14: "b", 13: "d", 11: "h",
           7: "v", 15: "n"}
    return "".join(inv[c & 15].upper() if c & 16 else inv[c & 15] for c in q)


def check_record(k, name, q):
    """The motifs the engine refuses (the reference is undefined there)."""
    where = f'record {k} ("{name}")'
    if len(q) == 0:
        raise MotifRefused(f"{where}: has no bases")
    if len(q) == 1:
        raise MotifRefused(f"{where}: has one base")
    if len(q) > 32:
        raise MotifRefused(f"{where}: is longer than 32 bases")
    widest = max(bin(c & 15).count("1") for c in q)
    if any((c & 16) and bin(c & 15).count("1") < widest for c in q):
        raise MotifRefused(f"{where}: marks a site (uppercase) on a base narrower than its widest")


def strands(data):
    """The motif file as the engine's table: per record the motif as written, then strrcMeth of it."""
    out = []
    for k, (name, q) in enumerate(motif_records(data), 1):
        check_record(k, name, q)
        out += [q, strrc(q)]
    tab = np.zeros(len(out), dtype=MOTIF_DTYPE)
    for t, q in zip(tab, out):
        t["len"] = len(q)
        t["meth"] = sum(0x80000000 >> k for k, c in enumerate(q) if c & 16)
        t["allow"][:len(q)] = [c & 15 for c in q]
    return tab


def strands_of(*texts):
    return strands("".join(f">m{k}\n{t}\n" for k, t in enumerate(texts)).encode())


def unpack(row, length):
    """2-bit codes of a qseq2nibble row (position p at bits 63 - 2p, 62 - 2p of word p / 32)."""
    row = np.asarray(row, dtype=np.uint64)
    p = np.arange(length)
    return ((row[p >> 5] >> (62 - 2 * (p & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)


def pack(codes, W=None):
    codes = np.asarray(codes, dtype=np.uint64)
    L = len(codes)
    W = L // 32 + 1 if W is None else W
    row = np.zeros(W, dtype=np.uint64)
    p = np.arange(L)
    np.bitwise_or.at(row, p >> 5, codes << (62 - 2 * (p & 31)).astype(np.uint64))
    return row


def sites(codes, tab):
    """(cleared positions bool[len], matches) of one row: strand j matches at
    start p <= len - m when code[p + k] is in allow[k] for all k."""
    L = len(codes)
    cleared = np.zeros(L, dtype=bool)
    found = 0
    for t in tab:
        m = int(t["len"])
        if m > L:
            continue
        ns = L - m + 1
        ok = np.ones(ns, dtype=bool)
        for k in range(m):
            ok &= ((int(t["allow"][k]) >> codes[k:k + ns]) & 1).astype(bool)
        found += int(ok.sum())
        for k in range(m):
            if int(t["meth"]) & (0x80000000 >> k):
                cleared[k:k + ns] |= ok
    return cleared, found


def to_words(bits, W):
    """bool per position -> include-mask words (bit 31 - pos % 32 of word pos / 32)."""
    w = np.zeros(W, dtype=np.uint32)
    p = np.nonzero(bits)[0]
    np.bitwise_or.at(w, p >> 5, (0x80000000 >> (p & 31)).astype(np.uint32))
    return w


def mask_rows(seqs, incs, n, length, tab, pair):
    """What ccg_meth_mask computes: (incs, inc_count[n], matches)."""
    seqs = np.asarray(seqs, dtype=np.uint64).reshape(n, -1)
    out = np.array(incs, dtype=np.uint32)
    stride = seqs.shape[1]
    Wd = (length + 31) // 32
    total = 0
    for t in range(n):
        cl, f = sites(unpack(seqs[t], length), tab)
        total += f
        w = to_words(cl, stride)
        if pair:
            out[t] &= ~w
        else:
            out &= ~w
    npos = lambda m: int(sum(bin(int(x)).count("1") for x in m[:Wd]))
    cnt = np.array([npos(out[t]) if pair else npos(out) for t in range(n)], dtype=np.int32)
    return out, cnt, total


# ------------------------------------------------------------------ the loader with -y
def fasta_records(data):
    """FileBuffgetFsa's records: the header line ('>' included, trailing white
    space trimmed) and the bytes up to the next '>'; a header that ends the
    input ends it without a record."""
    p = 0
    while p < len(data):
        e = data.find(b"\n", p)
        if e < 0 or e + 1 >= len(data):
            return
        nx = data.find(b">", e + 1)
        nx = len(data) if nx < 0 else nx
        yield data[p:e + 1].rstrip(), data[e + 1:nx]
        p = nx


def load_dist(fasta, tab, flag=1, min_length=1, min_cov=0.5, proxi=0):
    """ltdMsaMatrix_get with a motif table: dict(headers, seqs, incs, len, W,
    pair, minLength, log) -- log the stderr lines up to the matrix."""
    from ccphylo_amd import native
    lib = native.host_lib()
    table = np.zeros(256, dtype=np.uint8)
    lib.ccq_code_table(flag, table.ctypes.data)
    variant = 32 if flag & 32 else 8 if flag & 8 else 0
    pair = bool(flag & 2)
    heads, rows, masks, log = [], [], [], []
    ref = gmask = None
    L = W = 0

    def own_mask(codes, row):
        m = np.zeros(W, dtype=np.uint32)
        lib.ccq_init_inc(m.ctypes.data, L)
        m &= ~to_words(sites(unpack(row, L), tab)[0], W)   # maskMotifs
        c = codes.copy()
        lib.ccq_inc_update(m.ctypes.data, c.ctypes.data, c.ctypes.data, L, proxi, variant)
        return m

    for hdr, body in fasta_records(fasta):
        name = hdr[1:].decode("latin-1")
        codes = table[np.frombuffer(body, dtype=np.uint8)]
        codes = np.ascontiguousarray(codes[codes < 8])
        if ref is None:
            L = len(codes)
            if min_length < min_cov * L:
                min_length = int(min_cov * L)
            W = L // 32 + 1
        elif len(codes) != L:
            raise RuntimeError("Sequences does not match")
        row = pack(np.where(codes == 4, 0, codes), W)
        if ref is None or pair:
            m = own_mask(codes, row)
            inc = lib.ccq_npos(m.ctypes.data, L)
            keep = inc >= min_length
            if keep and ref is None:
                ref = codes
                if not pair:
                    gmask = m
        else:
            inc = L - int((codes == 4).sum())
            keep = min_length < inc
            if keep:
                gmask &= ~to_words(sites(unpack(row, L), tab)[0], W)
                c, r = codes.copy(), ref.copy()
                lib.ccq_inc_update(gmask.ctypes.data, c.ctypes.data, r.ctypes.data, L, proxi, variant)
        log.append("# %s:\t%s\t( %d / %d )\n" % ("Included" if keep else "Excluded", name, inc, L))
        if keep:
            heads.append(name)
            rows.append(row)
            if pair:
                masks.append(m)
    n = len(heads)
    seqs = np.array(rows, dtype=np.uint64).reshape(n, W) if n else np.zeros((0, max(W, 1)), np.uint64)
    incs = (np.array(masks, dtype=np.uint32).reshape(n, W) if pair else gmask) if n else np.zeros(max(W, 1), np.uint32)
    return dict(headers=heads, seqs=seqs, incs=incs, len=L, W=W, pair=pair, minLength=min_length, log="".join(log))


def expected_cli(golden_dir, case):
    """(stdout, stderr) of a golden `dist -y` case, from this restatement."""
    import conftest
    from oracle import pyoracle
    o = conftest.parse_dist_args([a for a in case["args"]])
    with open(os.path.join(golden_dir, case["motifs"]), "rb") as f:
        tab = strands(f.read())
    with open(os.path.join(golden_dir, case["input"]), "rb") as f:
        M = load_dist(f.read(), tab, o["flag"], o["minLength"], o["minCov"], o["proxi"])
    n, err, out = len(M["headers"]), M["log"], b""
    if n * (n - 1) // 2 < 1:
        err += "Adjustning number of nodes to %d, to conform with the matrix size.\n" % (n * (n - 1) // 2)
    if n == 0:
        err += "All sequences were trimmed away.\n"
    elif not M["pair"]:
        inc = int(sum(bin(int(x)).count("1") for x in M["incs"]))
        err += "# %d / %d bases included in distance matrix.\n" % (inc, M["len"])
    if n > 1:
        D, N, _ = pyoracle.snp_ltd(M["seqs"], M["incs"], n, M["len"], pair=M["pair"], norm=o["norm"],
                                   min_length=M["minLength"], proxi=o["proxi"] if M["pair"] else 0, etype=o["et"],
                                   byte_scale=o["bs"], want_n=M["pair"] and o["nout"])
        out = conftest.print_phylip(D, n, M["headers"], o["flag"], o["prec"], o["et"], o["bs"])
        if M["pair"] and o["nout"]:
            out += conftest.print_phylip(N, n, M["headers"], o["flag"], o["prec"], o["et"], o["bs"])
    return out, err.encode("latin-1")
