"""A plain restatement of `wgbstools bam2pat` (include/wgbsseg.h, wgbsseg_patview_set_sam) for the tests: SAM text -> the collapsed pat
text, the way the reference gets there — the adjusted sequence of clean_CIGAR is really made, the mates are found by walking the lines
one after the other, the result is sorted and counted with Python's own tools.  Nothing of csrc/sam_core.h's shape is shared with it.

    bam2pat(text, loci, chroms, ...) -> (pat text as bytes, counters)

loci: the bp position of every CpG, the chromosomes' sites one after the other; chroms: [(name, number of sites)] in that order; site
numbers count from 1 over all chromosomes."""
import bisect
import collections

MAX_QNAME, MAX_PE = 254, 300
HEADER, FILTERED, UNKNOWN, INVALID, EMPTY, PAT = 1, 2, 3, 4, 5, 6
COUNTERS = ('lines', 'header', 'filtered', 'invalid', 'unknown_chrom', 'empty', 'short', 'pairs', 'left_single', 'too_long')


def tokens_of(line):
    """patter's line2tokens: split at tabs, a last empty field is no token"""
    tok = line.split(b'\t')
    if tok and tok[-1] == b'':
        tok.pop()
    return tok


def number(field, most):
    """decimal digits and nothing else, at most `most`: the value, else None"""
    if not field or not field.isdigit() or not field.isascii():
        return None
    v = int(field)
    return v if v <= most else None


def keep(flag, mapq, paired, exclude=1796, include=0, min_mapq=10, strand=0):
    if flag & exclude or (flag & include) != include or mapq < min_mapq:
        return False
    if strand == 1:
        return flag in (99, 147) if paired else flag == 0
    if strand == 2:
        return flag in (83, 163) if paired else flag == 16
    return True


def is_bottom(flag, paired):
    return (flag & 0x53) == 83 or (flag & 0xA3) == 163 if paired else bool(flag & 0x10)


def clean_cigar(seq, cigar):
    """the adjusted sequence, or None when the CIGAR is refused"""
    out, num = [], b''
    for c in cigar:
        c = bytes([c])
        if c.isdigit():
            num += c
            continue
        if not num or int(num) > 2 ** 31 - 1:
            return None
        k, num = int(num), b''
        if c in b'M=X':
            if k > len(seq):
                return None
            out.append(seq[:k])
            seq = seq[k:]
        elif c in b'DN':
            out.append(b'N' * k)
        elif c in b'IS':
            if k > len(seq):
                return None
            seq = seq[k:]
        elif c != b'H':
            return None
    return b''.join(out)


def line_pat(tok, paired, sites, clip):
    """(state, first site, pattern) of a line that passed the filter; sites: (loci of its chromosome, the site number of the first)"""
    pos = number(tok[3], 2 ** 32 - 1)
    if len(tok[0]) > MAX_QNAME or pos is None:
        return INVALID, 0, b''
    seq = clean_cigar(tok[9], tok[5])
    if seq is None:
        return INVALID, 0, b''
    bottom = is_bottom(int(tok[1]), paired)
    loci, site0 = sites
    calls = []
    a = bisect.bisect_left(loci, pos)
    while a < len(loci) and loci[a] - pos < len(seq):
        i = loci[a] - pos
        j = i + 1 if bottom else i
        two = seq[i:i + 2]
        c = {b'CG': 'C', b'TG': 'T'}.get(two, '.') if not bottom else {b'CG': 'C', b'CA': 'T'}.get(two, '.')
        if not (clip <= j < len(seq) - clip):
            c = '.'
        calls.append((site0 + a, c))
        a += 1
    called = [k for k, (_, c) in enumerate(calls) if c != '.']
    if not called:
        return EMPTY, 0, b''
    part = calls[called[0]:called[-1] + 1]
    return PAT, part[0][0], ''.join(c for _, c in part).encode()


def merge(a, b):
    """merge_PE of two (start, pattern): (start, pattern), 'long' or 'empty'"""
    if a[0] > b[0]:
        a, b = b, a
    s, last = a[0], max(a[0] + len(a[1]), b[0] + len(b[1]))
    if last - s > MAX_PE:
        return 'long'
    m = ['.'] * (last - s)
    for i, c in enumerate(a[1].decode()):
        m[i] = c
    for i, c in enumerate(b[1].decode()):
        k = i + b[0] - s
        if m[k] == '.':
            m[k] = c
        elif c != '.' and m[k] != c:
            m[k] = '.'
    text = ''.join(m).rstrip('.')
    if not text:
        return 'empty'
    lead = len(text) - len(text.lstrip('.'))
    return s + lead, text[lead:].encode()


def classify(line, paired, table, exclude, include, mapq, strand, clip):
    """-> (state, key of the pairing or None, chromosome, first site, pattern)"""
    if line.startswith(b'@'):
        return HEADER, None, None, 0, b''
    tok = tokens_of(line)
    qname = tok[0] if tok else b''
    chrom = tok[2] if len(tok) >= 3 else None
    key = (qname, chrom if chrom in table else None) if len(qname) <= MAX_QNAME else object()
    flag = number(tok[1], 2 ** 31 - 1) if len(tok) >= 11 else None
    q = number(tok[4], 2 ** 31 - 1) if len(tok) >= 11 else None
    if flag is None or q is None:
        return (INVALID, key, chrom, 0, b'') if chrom in table else (UNKNOWN, None, chrom, 0, b'')
    if not keep(flag, q, paired, exclude, include, mapq, strand):
        return FILTERED, None, chrom, 0, b''
    if chrom not in table:
        return UNKNOWN, None, chrom, 0, b''
    state, start, pat = line_pat(tok, paired, table[chrom], clip)
    return state, key, chrom, start, pat


def bam2pat(text, loci, chroms, paired=False, exclude=1796, include=0, mapq=10, strand=0, clip=0, min_cpg=1):
    table, at = {}, 0
    loci = [int(x) for x in loci]
    for name, size in chroms:
        table[name.encode() if isinstance(name, str) else name] = (loci[at:at + size], at + 1)
        at += size
    n = dict.fromkeys(COUNTERS, 0)
    kept = []
    for line in text.split(b'\n'):
        if not line:
            continue
        n['lines'] += 1
        got = classify(line, paired, table, exclude, include, mapq, strand, clip)
        what = {HEADER: 'header', FILTERED: 'filtered', UNKNOWN: 'unknown_chrom', INVALID: 'invalid', EMPTY: 'empty'}.get(got[0])
        if what:
            n[what] += 1
        if got[0] >= INVALID:
            kept.append(got)
    out = collections.Counter()

    def emit(chrom, start, pat):
        if len(pat) < min_cpg:
            n['short'] += 1
        else:
            out[(start, pat, chrom)] += 1

    k = 0
    while k < len(kept):
        a = kept[k]
        b = kept[k + 1] if paired and k + 1 < len(kept) and kept[k + 1][1] == a[1] else None
        if b is None:
            n['left_single'] += 1 if paired else 0
            if a[0] == PAT:
                emit(a[2], a[3], a[4])
            k += 1
            continue
        n['pairs'] += 1
        k += 2
        if a[0] == PAT and b[0] == PAT:
            m = merge((a[3], a[4]), (b[3], b[4]))
            if m == 'long':
                n['too_long'] += 1
            elif m == 'empty':
                n['empty'] += 1
            else:
                emit(a[2], m[0], m[1])
        elif a[0] == PAT or b[0] == PAT:
            one = a if a[0] == PAT else b
            emit(one[2], one[3], one[4])
    lines = [b'%s\t%d\t%s\t%d\n' % (chrom, start, pat, count) for (start, pat, chrom), count in sorted(out.items())]
    return b''.join(lines), n
