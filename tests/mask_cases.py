"""Seeded inputs of the `wgbstools mask_pat` cases (tests/golden/make_golden_mask.py records what the reference's cview, mask_pat, sort and
collapse script print for them in tests/golden/mask_cases.json; tests/test_mask_pat_cpu.py and tests/test_gpu_mask_pat.py rebuild the
inputs).  Pat texts over the tiny genome of frag_cases.genome_dir (chr1: sites 1 .. 2500, chr2: 2501 .. 4000): every read lies inside the
chromosome it names and every count is at least 1 — where this build and the reference's pipe agree."""
import numpy as np

import homog_cases as HC
import merge_cases as MC

N_SITES = MC.N_SITES
genome_dir = MC.genome_dir
region_text = MC.region_text
_DOTS = b'CCTT.C.T'


def lines_text(reads, chrom=b'chr1'):
    return b''.join(b'%s\t%d\t%s\t%d\n' % (chrom, rs, pat, count) for rs, pat, count in reads)


def table_text(pairs, header=False, comments=False):
    """a 5-column blocks table of (startCpG, endCpG) pairs in the order given; comments: '#' lines, empty lines and a sixth column"""
    rows = ['chr1\t%d\t%d\t%d\t%d\n' % (50 * s, 50 * (e - 1) + 2, s, e) for s, e in pairs]
    if comments:
        rows = [r[:-1] + '\tsnp%d\n' % k for k, r in enumerate(rows)]
        rows.insert(len(rows) // 2, '\n')
        rows.insert(1, '# hidden on purpose\n')
        rows.insert(0, '#chr\tstart\tend\tstartCpG\tendCpG\tname\n')
    return ('chr\tstart\tend\tstartCpG\tendCpG%s\n' % ('\tname' if comments else '') if header else '') + ''.join(rows)


def seeded_blocks(seed, n, lo, hi, max_len=4):
    """n blocks with starts in [lo, hi] in hashed (unsorted) order: they overlap, nest and repeat"""
    U = HC.U
    s = (HC._rand(seed, 1, n) % U(hi - lo + 1)).astype(np.int64) + lo
    ln = 1 + (HC._rand(seed, 2, n) % U(max_len)).astype(np.int64)
    pairs = list(zip(s.tolist(), (s + ln).tolist()))
    return pairs + pairs[:n // 10]                                   # duplicates


# the issue's worked case: sites 6, 8, 9 and 12 are hidden
WORKED_BLOCKS = [(12, 13), (6, 7), (8, 10), (9, 10)]
WORKED_READS = [(5, b'CT', 1), (6, b'TCC', 2), (7, b'CC', 3), (8, b'C', 1), (8, b'C.T', 1), (9, b'.TC', 2), (10, b'TCTT', 1), (40, b'..', 1)]
WORKED_OUT = b'chr1\t5\tC\t1\nchr1\t7\tC\t5\nchr1\t10\tT\t1\nchr1\t10\tTC\t2\nchr1\t10\tTC.T\t1\n'

# bitmap edges: lo = 100; one-site blocks at lo, lo + 31, lo + 32, lo + 63, lo + 64; a block over the three whole words 3 .. 5 of the
# bitmap ([196, 292)); nested, overlapping, duplicate blocks; the last block ends at hi = 401
EDGE_LO, EDGE_HI = 100, 401
EDGE_BLOCKS = [(400, 401), (163, 164), (100, 101), (196, 292), (132, 133), (131, 132), (164, 165), (300, 310), (303, 306), (305, 315), (300, 310),
               (320, 321), (322, 323)]


def edge_reads():
    """short reads at every start from 90 to 410 (before lo, across it, inside, across hi, behind it), dots beside hidden sites; long reads
    whose hidden head ends behind a 32- and a 64-site boundary, a hidden tail, a wholly hidden read, and reads far outside"""
    letters = b'CTCCT.TC.CTT'
    reads = []
    for rs in range(90, 411):
        for ln in (1 + rs % 5, 3 + rs % 7):
            reads.append((rs, bytes(letters[(rs + i * (1 + ln % 3)) % 12] for i in range(ln)).replace(b'.', b'C', 1) if rs % 4 else b'C' * ln, 1 + rs % 3))
    reads += [(196, b'C' * 100, 2),                                 # head hidden up to 291: the start moves over 96 sites, 3 words
              (196, b'C' * 40 + b'.' * 56 + b'.T', 1),              # dots in the file behind a hidden head: the start moves to 293
              (180, b'T' * 16 + b'C' * 96, 1),                      # hidden tail
              (196, b'C' * 96, 5), (200, b'T' * 64, 1),             # wholly hidden: dropped
              (170, b'CT' * 75, 1),                                  # hidden interior: 96 dots kept inside
              (131, b'CC', 1), (163, b'CC', 1), (99, b'CC', 1), (399, b'CC', 1), (400, b'C', 7),
              (10, b'CTC', 1), (50, b'T' * 45, 1), (402, b'CT', 1), (2000, b'CCC', 2), (50, b'C' * 400, 1), (95, b'C' * 10, 1), (396, b'T' * 10, 1)]
    reads.sort(key=lambda r: r[0])                                   # (stable: equal starts keep the order above)
    return lines_text(reads)


LONG_BLOCKS = [(k, k + 1) for k in range(250, 1900, 2)]             # alternating one-site blocks


def long_reads():
    """one read of 1,500 sites (its line runs far past the staged tile) over alternating hidden sites, short reads around it"""
    body = bytes(b'CT'[(i // 3) % 2] for i in range(1500))
    reads = [(298, b'CT', 1), (299, b'TCC', 2), (300, body, 1), (300, b'CCTT', 3), (301, b'C', 1), (1795, b'TTTTTTT', 2), (1899, b'CC', 1), (1900, b'CC', 1)]
    return lines_text(reads)


# name -> pat: the text (bytes, or a callable that makes it); blocks: the pairs in table order; table: keywords of table_text;
# where: [] | ['-s', text] | ['-r', text]
CASES = {
    'worked': dict(pat=lines_text(WORKED_READS), blocks=WORKED_BLOCKS, where=[]),
    'worked_header_comments': dict(pat=lines_text(WORKED_READS), blocks=WORKED_BLOCKS, table=dict(header=True, comments=True), where=['-s', '1-100']),
    'edges': dict(pat=edge_reads, blocks=EDGE_BLOCKS, where=[]),
    'long_read': dict(pat=long_reads, blocks=LONG_BLOCKS, where=[]),
    'wg_short': dict(pat=lambda: MC.reads_text(91, 3000, 1, N_SITES, max_len=12, alphabet=_DOTS), blocks=lambda: seeded_blocks(92, 400, 1, N_SITES), where=[]),
    'sites_interval': dict(pat=lambda: MC.reads_text(93, 500, 1150, 1260, max_len=9, alphabet=_DOTS), blocks=lambda: seeded_blocks(94, 30, 1190, 1240, max_len=3),
                           where=['-s', '1200-1230']),
    'region': dict(pat=lambda: MC.reads_text(95, 500, 2750, 2960, max_len=5), blocks=lambda: seeded_blocks(96, 40, 2700, 3000, max_len=6), table=dict(header=True),
                   where=['-r', region_text]),
}


def _made(x):
    return x() if callable(x) else x


def case_pat(case):
    return _made(case['pat'])


def case_blocks(case):
    return [tuple(b) for b in _made(case['blocks'])]


def case_table(case):
    return table_text(case_blocks(case), **case.get('table', {}))


def case_where(case):
    return [_made(w) for w in case['where']]
