"""A plain-Python restatement of the contract of `wgbstools view` (wgbs_tools_amd/view.py's docstring), written from the contract:
parse and refuse, select, clip, strip, filter, sort, collapse, print.  tests/test_view_cpu.py holds it against every golden the
reference's own tools wrote, the GPU tests hold the device against it."""
import re

_INT = re.compile(rb'[ \x0b\x0c\r]*[+-]?(\d+)')
MAX_SUM = 10 ** 15


class Refused(Exception):
    def __init__(self, kind, offset=None):
        super().__init__('%s at %s' % (kind, offset))
        self.kind, self.offset = kind, offset


def _number(field, whole):
    """std::stoi's reading of a field (white space, a sign, digits; what follows is ignored unless `whole`), below 2^31; else None"""
    m = _INT.match(field)
    if not m or (whole and m.end() != len(field)):
        return None
    v = int(m.group(1))
    if v > 2 ** 31 - 1:
        return None
    return -v if b'-' in field[:m.start(1)] else v


def reads_of(text):
    """-> [(chrom, rs, pattern, count)] of the non-empty lines; Refused('bad', offset) for the first malformed line, else
    Refused('desc', offset) for the first read that starts before the read before it"""
    out, bad, desc, pos, prev = [], None, None, 0, None
    for line in text.split(b'\n'):
        off, pos = pos, pos + len(line) + 1
        if not line:
            continue
        tok = line.split(b'\t')
        rs = _number(tok[1], False) if len(tok) >= 2 else None
        count = _number(tok[3], True) if len(tok) == 4 else None
        if rs is None or count is None or not tok[2]:
            bad = off if bad is None else bad
            prev = None
            continue
        if prev is not None and rs < prev and desc is None:
            desc = off
        prev = rs
        out.append((tok[0], rs, tok[2], count))
    if bad is not None:
        raise Refused('bad', bad)
    if desc is not None:
        raise Refused('desc', desc)
    return out


def cut(rs, pat, s, e, strict=False, strip=False, no_gaps=False, min_len=1):
    """steps 1-5 on one read -> (rs', pattern) or None"""
    if rs >= e or rs + len(pat) - 1 < s:
        return None
    if strict:
        pat = pat[max(0, s - rs):]
        rs = max(rs, s)
        pat = pat[:e - rs]
    if strip:
        pat = pat.rstrip(b'.')
        if not pat:
            return None
        lead = len(pat) - len(pat.lstrip(b'.'))
        pat, rs = pat[lead:], rs + lead
    if min_len > len(pat):
        return None
    if no_gaps and b'.' in pat:
        return None
    return rs, pat


def sort_key(line):
    """`LC_ALL=C sort -k2,2n -k3,3` and its last resort as far as it can show, on (chrom, rs, pattern, count)"""
    return line[1], line[2], line[0]


def collapse(lines):
    out, run, total = [], None, 0
    for chrom, rs, pat, count in lines:
        if run is not None and run == (chrom, rs, pat):
            total += count
            continue
        if run is not None and total > 0:
            out.append(run + (total,))
        run, total = (chrom, rs, pat), count
    if run is not None and total > 0:
        out.append(run + (total,))
    return out


def survivors(text, s, e, **flags):
    out = []
    for chrom, rs, pat, count in reads_of(text):
        c = cut(rs, pat, s, e, **flags)
        if c is not None:
            out.append((chrom, c[0], c[1], count))
    return out


def view(text, s, e, sort=False, **flags):
    """the output text (bytes) for the interval [s, e)"""
    lines = survivors(text, s, e, **flags)
    if sort:
        lines = sorted(lines, key=sort_key)                       # (stable: ties keep the input order)
    runs = collapse(lines)
    if any(r[3] >= MAX_SUM for r in runs):
        raise Refused('sum')
    return b''.join(b'%s\t%d\t%s\t%d\n' % r for r in runs)
