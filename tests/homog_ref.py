"""A small numpy restatement of `wgbstools homog` (the reference's homog.py:83-131 + homog.cpp:154-260), for tests only: the
product never imports it.  Inputs: the pat text, the blocks table's text, the command-line options."""
import gzip
import hashlib

import numpy as np


def edges_of(rlen, thresholds=None):
    """the bin edges as float32: the reference's text, each number parsed once to float32 (strtof)"""
    import ctypes
    libc = ctypes.CDLL(None)
    libc.strtof.restype = ctypes.c_float
    libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    if thresholds:
        text = f'0,{thresholds},1'
    else:
        text = f'0,{round(1 - (rlen - 1) / rlen, 3) + 0.001},{round((rlen - 1) / rlen, 3)},1'
    return text, np.array([libc.strtof(t.encode(), None) for t in text.split(',')], dtype=np.float32)


def bin_of(nc, nt, edges):
    meth = np.float32(nc) / np.float32(nc + nt) if nc + nt else np.float32(np.nan)
    if meth < edges[0]:
        return -1
    for b in range(edges.size - 1):
        if edges[b] <= meth < edges[b + 1]:
            return b
    return edges.size - 2


def parse_blocks(text):
    """rows of a blocks table: [(chr, start, end) text, startCpG, endCpG]; '#' lines skipped, a header line skipped"""
    rows = []
    for ln in text.splitlines():
        if not ln or ln.startswith('#'):
            continue
        t = ln.split('\t')
        if not rows and not t[1].isdigit():
            continue
        rows.append(((t[0], t[1], t[2]), int(t[3]), int(t[4])))
    return rows


def count_sorted(pat_text, starts, ends, edges, rlen, inclusive):
    """int64 counts[n][bins] of blocks sorted by (start, end), wrapped to int32 like the reference's counters"""
    n, nb = starts.size, edges.size - 1
    c = np.zeros((n, nb), dtype=np.int64)
    pmax = np.maximum.accumulate(ends)
    last_end = int(ends[-1])
    for ln in pat_text.decode().splitlines():
        if not ln:
            continue
        t = ln.split('\t')
        s, pat, cnt = int(t[1]), t[2], int(t[3])
        if s >= last_end:
            break
        L = len(pat)
        if L < rlen:
            continue
        j0 = int(np.searchsorted(pmax, s, 'right'))
        j1 = int(np.searchsorted(starts, s + L - 1, 'right'))
        whole = (pat.count('C') + pat.count('H'), pat.count('T'))
        for j in range(j0, j1):
            os_, oe = max(s, int(starts[j])), min(s + L, int(ends[j]))
            if os_ >= oe:
                continue
            if inclusive:
                nc, nt = whole
            else:
                if oe - os_ < rlen:
                    continue
                piece = pat[os_ - s:oe - s]
                nc, nt = piece.count('C') + piece.count('H'), piece.count('T')
            if nc + nt < rlen:
                continue
            b = bin_of(nc, nt, edges)
            if b >= 0:
                c[j, b] += cnt
    return (c + 2 ** 31) % 2 ** 32 - 2 ** 31


def homog(pat_text, blocks_text, rlen=3, thresholds=None, inclusive=False):
    """-> (rows of the output table: [chr, start, end, startCpG, endCpG, U, X, M] as text fields, the merged int64 counts)"""
    rows = parse_blocks(blocks_text)
    s = np.array([r[1] for r in rows], dtype=np.int64)
    e = np.array([r[2] for r in rows], dtype=np.int64)
    _, edges = edges_of(rlen, thresholds)
    order = np.lexsort((e, s))
    cs = count_sorted(pat_text, s[order], e[order], edges, rlen, inclusive)
    # the wrapper's re-ordering: the row of sorted position r goes where a stable argsort of startCpG alone puts it
    counts = cs[np.argsort(np.argsort(s, kind='stable'), kind='stable')]
    # the left merge on the five coordinate columns
    keys = [(r[0], r[1], r[2]) for r in rows]
    where = {}
    for i, k in enumerate(keys):
        where.setdefault(k, []).append(i)
    out_rows, out_vals = [], []
    for i, k in enumerate(keys):
        for j in where[k]:
            out_rows.append(list(rows[i][0]) + [str(rows[i][1]), str(rows[i][2])] + [str(v) for v in counts[j].tolist()])
            out_vals.append(counts[j])
    return out_rows, np.array(out_vals, dtype=np.int64).reshape(-1, edges.size - 1)


def trim(vals, nr_bits):
    top = 2 ** nr_bits - 1
    d = vals.astype(np.int64).copy()
    for i in range(d.shape[0]):
        m = d[i].max()
        if m > top:
            d[i] = [int(v / m * top) for v in d[i].tolist()]
    return d.astype(np.uint16 if nr_bits == 16 else np.uint8)


def digests(pat_text, blocks_text, args):
    """the golden record's digests for a case's command-line arguments"""
    rlen = int(args[args.index('-l') + 1]) if '-l' in args else 3
    th = args[args.index('-t') + 1] if '-t' in args else None
    rows, vals = homog(pat_text, blocks_text, rlen, th, '--inclusive' in args)
    if '--binary' in args:
        nb = int(args[args.index('--nr_bits') + 1]) if '--nr_bits' in args else 8
        return dict(bin_sha1=hashlib.sha1(trim(vals, nb).tobytes()).hexdigest())
    text = ''.join('\t'.join(r) + '\n' for r in rows).encode()
    return dict(text_sha1=hashlib.sha1(text).hexdigest())


def read_output(path):
    with gzip.open(path, 'rb') as f:
        return f.read()
