"""Seeded pat files, blocks tables and command lines of the `wgbstools test_bimodal` cases (tests/golden/make_golden_bimodal.py
writes the reference's output for them into tests/golden/bimodal_cases.json; tests/test_bimodal_cpu.py and tests/test_gpu_bimodal.py
rebuild the inputs).  Deterministic across platforms: every random number is synth.hash_at (splitmix64), as in homog_cases."""
import numpy as np

from wgbs_tools_amd import synth
from wgbs_tools_amd.synth import hash_at

U = np.uint64
GENOME_SEED = 20261015
CHROMS = [('chr1', 3000), ('chr2', 2000), ('chr3', 1000)]     # the genome; blocks on 'chrUn' are on a chromosome it lacks


def _rand(seed, stream, n):
    return hash_at(seed, stream, np.arange(n, dtype=np.int64))


def n_sites():
    return sum(s for _, s in CHROMS)


def chrom_of(cpg):
    cum = np.cumsum([s for _, s in CHROMS])
    return [CHROMS[min(int(i), len(CHROMS) - 1)][0] for i in np.searchsorted(cum, np.asarray(cpg) - 1, 'right')]


def is_bimodal_site(x, period=300):
    """regions of two read populations: sites in the first third of every `period`"""
    return (np.asarray(x) % period) < period // 3


def pat_text(seed, n_reads, max_len=10, long_every=0, long_len=160, max_count=6, zero_every=0, gap=None, period=300, noise=8, flat=False):
    """A pat file's text (bytes), sorted by start (1 .. n_sites): reads of 1..max_len sites; in the bimodal regions a read is
    all-C or all-T (one allele each, with 1 in `noise` sites flipped), elsewhere C (3 in 4) or T at random; '.' and 'H' (unobserved) here
    and there; flat: outside the bimodal regions too a read is mostly C (one population).  long_every > 0: every long_every-th read is long_len..long_len + 63 sites (longer than the reference's 150-site
    look-back); zero_every > 0: every zero_every-th count is 0; gap = (a, b): no read starts in [a, b)."""
    N = n_sites()
    start = np.sort(1 + (_rand(seed, 1, n_reads) % U(N)).astype(np.int64))
    if gap is not None:
        start = start[(start < gap[0]) | (start >= gap[1])]
    n = start.size
    h = _rand(seed, 2, n)
    ln = 1 + (h % U(max_len)).astype(np.int64)
    if long_every:
        ln[::long_every] = long_len + ((h[::long_every] >> U(40)) % U(64)).astype(np.int64)
    cum = np.cumsum([c for _, c in CHROMS])
    ln = np.minimum(ln, cum[np.searchsorted(cum, start - 1, 'right')] - start + 1)     # a read stays on its chromosome
    cnt = 1 + ((h >> U(8)) % U(max_count)).astype(np.int64)
    if zero_every:
        cnt[::zero_every] = 0
    allele = ((h >> U(20)) & U(1)).astype(bool)
    chars = []
    r = _rand(seed, 3, int(ln.sum()))
    pos = 0
    for i in range(n):
        k = int(ln[i])
        rr = r[pos:pos + k]
        pos += k
        bim = is_bimodal_site(start[i] + np.arange(k), period)
        flip = (rr % U(noise)) == 0
        meth = np.where(bim, allele[i] ^ flip, ~flip if flat else ((rr >> U(8)) % U(4)) != 0)
        ch = np.where(meth, 'C', 'T')
        ch = np.where(((rr >> U(16)) % U(13)) == 0, '.', ch)
        ch = np.where(((rr >> U(24)) % U(29)) == 0, 'H', ch)
        chars.append(''.join(ch.tolist()))
    chroms = chrom_of(start)
    return ''.join('%s\t%d\t%s\t%d\n' % (chroms[i], start[i], chars[i], cnt[i]) for i in range(n)).encode()


def blocks(seed, kind='segmentation', max_len=12, wide=0, every=1):
    """(startCpG, endCpG, extra chromosome names) of a blocks table, in the genome's order.  segmentation: a partition into
    blocks of 1..max_len sites with gaps; 'nested': plus blocks nested in and duplicating others; wide > 0: plus blocks of
    `wide` sites; every: only every every-th block of the partition; 'chrUn' rows are added by blocks_text."""
    N = n_sites()
    m = 2 * N // max(1, max_len // 2) + 16
    ln = 1 + (_rand(seed, 11, m) % U(max_len)).astype(np.int64)
    ends = 1 + np.cumsum(ln)
    starts = ends - ln
    keep = (ends <= N + 1) & ((_rand(seed, 12, m) % U(5)) != 0)
    s, e = starts[keep][::every], ends[keep][::every]
    if kind == 'nested':
        h = _rand(seed, 13, s.size)
        pick = (h % U(9)) == 0
        s2 = s[pick]
        e2 = np.minimum(e[pick] + 1 + (h[pick] >> U(8)) % U(20), N + 1).astype(np.int64)
        dup = (h % U(11)) == 1
        s = np.concatenate([s, s2, s[dup]])
        e = np.concatenate([e, e2, e[dup]])
    if wide:
        w = np.array([100, N // 2 + 50, N - wide - 10], dtype=np.int64)
        s = np.concatenate([s, w])
        e = np.concatenate([e, w + wide])
    o = np.lexsort((e, s))
    return s[o], e[o]


def blocks_text(s, e, seed=0, chr_un=0, comments=False, extra_col=False):
    """the text of a blocks table: chr, start, end (base pairs, 50 per CpG), startCpG, endCpG (and a name column with
    extra_col), sorted by chromosome then start; chr_un rows on 'chrUn' (a chromosome the genome lacks) at the end"""
    chroms = chrom_of(s)
    rows = []
    for i in range(len(s)):
        r = '%s\t%d\t%d\t%d\t%d' % (chroms[i], 50 * s[i], 50 * (e[i] - 1) + 2, s[i], e[i])
        if extra_col:
            r += '\tblk%d' % i
        rows.append(r + '\n')
    for k in range(chr_un):
        rows.append('chrUn\t%d\t%d\t%d\t%d\n' % (100 * k, 100 * k + 60, 10 + k, 20 + k))
    if comments:
        rows.insert(0, '#chr\tstart\tend\tstartCpG\tendCpG\n')
    return ''.join(rows)


_P = dict(seed=41, n_reads=6000, long_every=37, zero_every=23, gap=(2300, 2700))
_PN = dict(seed=41, n_reads=6000, zero_every=23, gap=(2300, 2700))        # without long reads: see 'L_default'
_B = dict(seed=5, kind='nested', wide=300, every=6)

# name -> generator parameters and the command-line arguments after the pat file (the blocks file / a site range)
CASES = {
    # without --strict a read of 150+ sites makes rows of hundreds of observations, whose likelihoods the reference sums in
    # BLAS's order: near-ties of the assignment then depend on the host, so those reads are exercised by the --strict cases
    'L_default': dict(pat=_PN, blocks=_B, bed=dict(chr_un=3), args=[]),
    'L_strict': dict(pat=_P, blocks=_B, bed=dict(chr_un=3), args=['--strict']),
    'L_min_len3': dict(pat=_PN, blocks=_B, bed=dict(chr_un=3), args=['--min_len', '3']),
    'L_strict_min_len3_all': dict(pat=_P, blocks=_B, bed=dict(chr_un=3, comments=True, extra_col=True),
                                  args=['--strict', '--min_len', '3', '--print_all_regions']),
    'L_all_regions': dict(pat=_PN, blocks=_B, bed=dict(chr_un=0), args=['--print_all_regions']),
    # only unimodal reads: the best p is not significant, so the first block is not rejected -> empty output
    'L_first_not_rejected': dict(pat=dict(seed=42, n_reads=3000, period=1, noise=16, flat=True),
                                 blocks=dict(seed=6, kind='segmentation', every=4), bed=dict(), args=[]),
    # deep two-population blocks only: every block rejected -> empty output (the reference's argmax quirk)
    'L_all_rejected': dict(pat=dict(seed=43, n_reads=8000, max_len=8, max_count=10), blocks=dict(seed=7, kind='few'), bed=dict(), args=[]),
    'L_all_rejected_printed': dict(pat=dict(seed=43, n_reads=8000, max_len=8, max_count=10), blocks=dict(seed=7, kind='few'), bed=dict(),
                                   args=['--print_all_regions']),
    # single regions: the printed likelihoods carry every digit, so only blocks whose row sums do not depend on the order of
    # summation (few observations per row) can be pinned to the reference's text
    's_bimodal_strict': dict(pat=_P, sites=(20, 32), args=['--strict']),
    's_short_strict': dict(pat=_P, sites=(21, 24), args=['--strict']),
    's_short': dict(pat=_P, sites=(3301, 3303), args=['--strict', '--min_len', '2']),
    's_unimodal_strict': dict(pat=_P, sites=(150, 154), args=['--strict']),
    's_pair': dict(pat=_P, sites=(4005, 4007), args=['--strict']),
    's_empty': dict(pat=_P, sites=(2500, 2510), args=['--strict']),
}


def case_blocks(spec):
    """-> (startCpG, endCpG) of the case's blocks in the genome's order (the chrUn rows excluded)"""
    if spec['kind'] == 'few':                                     # six blocks inside bimodal regions, all chromosomes
        s = np.array([10, 40, 610, 3020, 3610, 5110], dtype=np.int64)
        return s, s + 30
    return blocks(spec['seed'], spec['kind'], wide=spec.get('wide', 0), every=spec.get('every', 1))


def case_inputs(case):
    """-> (pat text, blocks text or None, [argv after the pat path, the blocks / sites option excluded])"""
    pat = pat_text(**case['pat'])
    if 'sites' in case:
        return pat, None, case['args']
    s, e = case_blocks(case['blocks'])
    return pat, blocks_text(s, e, **case['bed']), case['args']


def write_genome(refdir):
    """the cases' synthetic genome (loci from synth.synth_loci) as a reference directory"""
    names = [c for c, _ in CHROMS]
    sizes = [s for _, s in CHROMS]
    return synth.write_genome(refdir, names, sizes, synth.synth_loci(GENOME_SEED, sizes))
