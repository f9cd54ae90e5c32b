"""Inputs of the `wgbstools bed2beta` cases (tests/golden/make_golden_bed2beta.py records what the reference's own load_bed, left merge and
trim_to_uint8 give for them in tests/golden/bed2beta_cases.json; tests/test_bed2beta_cpu.py and tests/test_gpu_bed2beta.py rebuild the
inputs): BED texts over the tiny genome of frag_cases.genome_dir (chr1: 2,500 CpGs, chr2: 1,500), every line with meth <= total, so that
the reference itself stays inside the contract; and the random worlds of the comparison with tests/bed2beta_ref.py."""
import numpy as np

import frag_cases as FC
from wgbs_tools_amd import synth

CHROMS = FC.GENOME_CHROMS
N_SITES = FC.N_SITES
N1 = CHROMS[0][1]
HEADER = 'chr\tstart\tend\tmeth\ttotal\n'
TOP = 2 ** 31 - 1


def loci():
    return synth.synth_loci(FC.GENOME_SEED, [s for _, s in CHROMS]).astype(np.int64)


_L = loci()
L1, L2 = _L[:N1], _L[N1:]
COMMON = np.intersect1d(L1, L2)                    # positions that are a CpG on both chromosomes
assert COMMON.size >= 2


def line(chrom, start, meth, total, end=None, extra=''):
    return '%s\t%d\t%d\t%d\t%d%s\n' % (chrom, start, start + 2 if end is None else end, meth, total, extra)


def _rand(stream, n):
    return (synth.hash_at(20261021, 700 + stream, np.arange(n)) >> np.uint64(20)).astype(np.int64)


def _pairs(stream, n, top=40):
    r = _rand(stream, n)
    total = r % top
    meth = (r >> 8) % (total + 1)
    return meth.tolist(), total.tolist()


def _basic(k0=3, n=12, chrom='chr1', shift=0, stream=1):
    src = L1 if chrom == 'chr1' else L2
    m, t = _pairs(stream, n)
    return [line(chrom, int(src[k0 + 7 * i]) - shift, m[i], t[i] + 1) for i in range(n)]


def _big():
    """one line per CpG, some twice or three times with other values (the later ones far behind the first: other tiles), lines at
    positions that are no CpG, lines on chromosomes the genome does not have; order shuffled"""
    m, t = _pairs(9, N_SITES, top=700)
    rows = []
    for i in range(N_SITES):
        chrom, p = ('chr1', int(L1[i])) if i < N1 else ('chr2', int(L2[i - N1]))
        rows.append(line(chrom, p, m[i], t[i] + 1))
        if i % 11 == 0:
            rows.append(line(chrom, p, t[i] + 1, t[i] + 1, extra=''))
        if i % 97 == 0:
            rows.append(line(chrom, p, 0, 3))
        if i % 13 == 0:
            rows.append(line(chrom, p + 1, 5, 9))
        if i % 101 == 0:
            rows.append(line('chr10' if i % 2 else 'chrUn_gl000220', p, 4, 4))
    o = np.argsort(_rand(10, len(rows)), kind='stable')
    return [rows[i] for i in o.tolist()]


def _unsorted():
    rows = _basic(40, 30, 'chr1', stream=4) + _basic(10, 30, 'chr2', stream=5) + _basic(40, 10, 'chr1', stream=6)     # (the last ten: duplicates)
    o = np.argsort(_rand(11, len(rows)), kind='stable')
    return [rows[i] for i in o.tolist()]


# name -> lines: the BED lines in file order; add_one; header: the file begins with HEADER
CASES = {
    'header': dict(lines=_basic(), header=True),
    'no_header': dict(lines=_basic()),
    'add_one': dict(lines=_basic(shift=1) + [line('chr1', int(L1[200]), 3, 4), line('chr2', int(L2[9]) - 1, 2, 2)], add_one=True),
    'add_one_header': dict(lines=_basic(shift=1, chrom='chr2'), add_one=True, header=True),
    'dup_first_not_largest': dict(lines=[line('chr1', int(L1[50]), 3, 10), line('chr1', int(L1[51]), 1, 1), line('chr1', int(L1[50]), 9, 10),
                                         line('chr1', int(L1[50]), 1, 10), line('chr2', int(L2[50]), 0, 300), line('chr2', int(L2[50]), 300, 300)]),
    'dup_of_unmatched': dict(lines=[line('chr1', int(L1[60]) + 1, 3, 10), line('chr1', int(L1[60]), 2, 5), line('chr1', int(L1[60]) + 1, 4, 10),
                                    line('chrQ', int(L1[61]), 1, 2), line('chrQ', int(L1[61]), 2, 2)]),
    'unknown_chrom': dict(lines=[line('chrX', int(L1[5]), 1, 2), line('chr1', int(L1[5]), 2, 3), line('chrM', 16000, 7, 7), line('1', int(L1[6]), 1, 1),
                                 line('CHR1', int(L1[7]), 1, 1)]),
    'chr1_beside_chr10': dict(lines=[line('chr10', int(L1[5]), 1, 2), line('chr1', int(L1[5]), 2, 3), line('chr', int(L1[6]), 7, 7), line('chr11', int(L1[7]), 1, 1),
                                     line('chr2x', int(L2[7]), 1, 1), line('chr2', int(L2[7]), 5, 6), line('chr1 ', int(L1[8]), 1, 1), line('chr10', int(L1[9]), 1, 2)]),
    'same_position_two_chroms': dict(lines=[line('chr2', int(COMMON[0]), 1, 7), line('chr1', int(COMMON[0]), 6, 7), line('chr1', int(COMMON[1]), 2, 9),
                                            line('chr2', int(COMMON[1]), 8, 9)]),
    'first_and_last_cpg': dict(lines=[line('chr1', int(L1[0]), 1, 2), line('chr1', int(L1[-1]), 3, 4), line('chr2', int(L2[0]), 5, 6), line('chr2', int(L2[-1]), 7, 8),
                                      line('chr1', int(L1[0]) - 2, 1, 1), line('chr2', int(L2[-1]) + 2, 1, 1), line('chr1', 0, 1, 1), line('chr2', 2 ** 32 + int(L2[3]), 1, 1)]),
    'one_off': dict(lines=[line('chr1', int(L1[70]) - 1, 1, 2), line('chr1', int(L1[70]) + 1, 1, 2), line('chr1', int(L1[71]), 4, 5), line('chr2', int(L2[70]) + 1, 1, 2)]),
    'extra_columns': dict(lines=[line('chr1', int(L1[80 + i]), i, 2 * i + 1, end=i, extra='\t+\t%d.5\tnote %d' % (i, i)) for i in range(8)]
                          + [line('chr2', int(L2[80]), 2, 2, end=0, extra='\t-\tNA\t')]),
    'blank_lines': dict(lines=[line('chr1', int(L1[90]), 1, 2), '\n', line('chr1', int(L1[91]), 2, 3), '\n', '\n', '\n', line('chr2', int(L2[90]), 3, 4), '\n']),
    'totals': dict(lines=[line('chr1', int(L1[100 + i]), t, t) for i, t in enumerate((255, 256, 600, TOP))]
                   + [line('chr2', int(L2[100 + i]), m, t) for i, (m, t) in enumerate(((254, 255), (100, 256), (255, 256), (599, 600), (1, 600), (1, TOP), (TOP - 1, TOP),
                                                                                     (0, TOP), (2 ** 30, TOP), (3, 257), (85, 256), (171, 511)))]),
    'unsorted': dict(lines=_unsorted()),
    'big_mixed': dict(lines=_big(), header=True),
}


def case_text(case):
    return ((HEADER if case.get('header') else '') + ''.join(case['lines'])).encode()


def case_flags(case):
    return ['--add_one'] if case.get('add_one') else []


def sparse(rows):
    """the non-zero rows of a result as [[site, meth, total], ...]"""
    nz = np.flatnonzero(rows.any(axis=1))
    return [[int(i), int(rows[i, 0]), int(rows[i, 1])] for i in nz.tolist()]


def dense(pairs, n=N_SITES):
    rows = np.zeros((n, 2), dtype=np.uint8)
    for i, m, c in pairs:
        rows[i] = (m, c)
    return rows


def random_world(rng):
    """-> (BED text, add_one): lines over the tiny genome — CpGs, near misses, unknown chromosomes, duplicates close by and far apart,
    totals around 255 and up to 2^31 - 1, blank lines, sometimes a header, sometimes no last newline"""
    n = int(rng.integers(1, 3000))
    add_one = bool(rng.random() < 0.5)
    sites = rng.integers(0, N_SITES, n)
    if rng.random() < 0.5:
        sites = np.sort(sites)
    if rng.random() < 0.5:
        sites[rng.integers(0, n, n // 3 + 1)] = sites[rng.integers(0, n, n // 3 + 1)]       # duplicates
    names = ('chr1', 'chr2', 'chr10', 'chr', 'chrX')
    out = []
    for s in sites.tolist():
        chrom, p = ('chr1', int(L1[s])) if s < N1 else ('chr2', int(L2[s - N1]))
        u = rng.random()
        if u < 0.08:
            p += int(rng.choice([-1, 1]))
        elif u < 0.14:
            chrom = names[int(rng.integers(0, len(names)))]
        total = int(rng.choice([1, 9, 255, 256, 257, 1000, TOP])) if rng.random() < 0.3 else int(rng.integers(0, 400))
        meth = int(rng.integers(0, total + 1))
        extra = '\tx\ty' if rng.random() < 0.05 else ''
        out.append(line(chrom, p - (1 if add_one else 0), meth, total, extra=extra))
        if rng.random() < 0.01:
            out.append('\n')
    text = ''.join(out)
    if rng.random() < 0.3:
        text = HEADER + text
    if rng.random() < 0.3:
        text = text.rstrip('\n')
    return text.encode(), add_one
