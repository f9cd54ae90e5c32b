"""`wgbstools frag_len` restated in plain Python, from the contract alone: which lines of a sorted pat text a block list lets
through (cview without --strict), twice — `select_walk` streams the reads past the blocks with a cursor that only moves forward, as
the tool does; `select_rule` tests every read on its own, as the kernel does — and the histogram of their lengths.  No numpy in the
counting: Python integers do not overflow."""
import re

import numpy as np

_INT = re.compile(rb'[ \v\f\r]*([+-]?)([0-9]+)')


class Refused(Exception):
    """kind: 'bad' (a malformed line) or 'desc' (a read starting before the read before it); offset: its first byte"""

    def __init__(self, kind, offset):
        super().__init__('%s at byte offset %d' % (kind, offset))
        self.kind, self.offset = kind, offset


def _stoi(field):
    """std::stoi on a field: leading white space, a sign, digits, anything behind them ignored; None when there is no digit or the
    value does not fit 31 bits"""
    m = _INT.match(field)
    if not m:
        return None
    v = int(m.group(2))
    if v > 2 ** 31 - 1:
        return None
    return -v if m.group(1) == b'-' else v


def reads_of(text):
    """[(byte offset, start, length, count)] of the non-empty lines; the first malformed one (fewer than four fields, a start or count
    that is no number, an empty pattern) raises Refused('bad')"""
    out, pos = [], 0
    for line in text.split(b'\n'):
        off, pos = pos, pos + len(line) + 1
        if not line:
            continue
        tok = line.split(b'\t')
        site = _stoi(tok[1]) if len(tok) >= 4 else None
        count = _stoi(tok[3]) if len(tok) >= 4 else None
        if site is None or count is None or not tok[2]:
            raise Refused('bad', off)
        out.append((off, site, len(tok[2]), count))
    return out


def cview_order(pairs):
    """(startCpG text, endCpG text) rows -> (starts, ends) int64 arrays as `sort -k1,1n` in the C locale orders the lines
    "startCpG\\tendCpG": by the first field as a number, equal ones by the bytes of the whole line"""
    rows = sorted(pairs, key=lambda p: (int(p[0]), (p[0] + '\t' + p[1]).encode()))
    return np.array([int(a) for a, _ in rows], dtype=np.int64), np.array([int(b) for _, b in rows], dtype=np.int64)


def check_sorted(reads):
    prev = None
    for off, site, _, _ in reads:
        if prev is not None and site < prev:
            raise Refused('desc', off)
        prev = site
    return reads


def select_walk(reads, starts, ends):
    """the reads passed on, by streaming: stop at the first read starting at or behind the LAST block's end; move the cursor past
    the blocks that end at or before the read's start; skip the read when it ends before the cursor's block starts"""
    starts, ends = [int(v) for v in starts], [int(v) for v in ends]
    out, cur = [], 0
    for r in reads:
        _, rs, ln, _ = r
        if rs >= ends[-1]:
            break
        while cur < len(ends) and rs >= ends[cur]:
            cur += 1
        if cur >= len(ends):
            break
        if rs + ln - 1 < starts[cur]:
            continue
        out.append(r)
    return out


def select_rule(reads, starts, ends):
    """the same, read by read: dropped when it starts at or behind the last block's end; else cur = the first block whose running
    maximum of endCpG exceeds the start, and the read counts iff it reaches startCpG[cur]"""
    starts, ends = [int(v) for v in starts], [int(v) for v in ends]
    pmax, run = [], 0
    for e in ends:
        run = max(run, e)
        pmax.append(run)
    out = []
    for r in reads:
        _, rs, ln, _ = r
        if rs >= ends[-1]:
            continue
        cur = next(j for j, p in enumerate(pmax) if p > rs)
        if rs + ln - 1 >= starts[cur]:
            out.append(r)
    return out


def histogram(reads, m):
    h = [0] * m
    for _, _, ln, count in reads:
        h[min(ln, m) - 1] += count
    return h


def frag_hist(text, m, blocks=None, walk=False):
    """the m sums of `text` (bytes) as Python integers; blocks: (starts, ends) in cview's order, None: every line.  With blocks an
    unsorted text raises Refused('desc') — after any Refused('bad'), which comes first wherever it lies."""
    reads = reads_of(text)
    if blocks is not None:
        check_sorted(reads)
        reads = (select_walk if walk else select_rule)(reads, blocks[0], blocks[1])
    return histogram(reads, m)


def line_of(hist):
    """what -v prints: nothing for an all-zero histogram"""
    return ' '.join(str(v) for v in hist) + '\n' if any(hist) else ''
