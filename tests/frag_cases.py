"""Seeded inputs of the `wgbstools frag_len` cases (tests/golden/make_golden_frag.py records what the reference's tools print for
them in tests/golden/frag_cases.json; tests/test_frag_len_cpu.py and tests/test_gpu_frag_len.py rebuild the inputs): pat texts from
homog_cases.pat_text (every random number is synth.hash_at) or written out line by line, a tiny genome directory for -r, block
tables with nested blocks, equal starts, NA rows and a header; and the random worlds of the comparison with tests/frag_ref.py."""
import os.path as op

import numpy as np

import homog_cases as HC

GENOME_SEED = 20261021
GENOME_CHROMS = [('chr1', 2500), ('chr2', 1500)]
N_SITES = 4000
LDS_BINS = 2048                                    # csrc/frag_plan.h WG_FRAG_LDS_BINS (tests/test_frag_len_cpu.py checks it)

# the issue's boundary list, in file order; cview takes equal starts by the bytes of "startCpG\tendCpG": [40, 45) before [40, 50)
BOUNDARY_BLOCKS = [(10, 20), (40, 50), (40, 45)]
# the same with a long middle block, whose text "40\t100" sorts before "40\t45": [40, 45) is then the block that sorts LAST, and a
# read at 46 is dropped although [40, 100) holds it
BOUNDARY_BLOCKS_LAST_NESTED = [(10, 20), (40, 100), (40, 45)]
# (start, length, count): ending at start - 1 and at start; starting at end - 1 and at end; in the gap; the same around 40 / 45 / 50.
# The counts are powers of two: a sum names its reads.
BOUNDARY_READS = [(7, 3, 1), (8, 3, 2), (19, 2, 4), (20, 2, 8), (25, 3, 16), (37, 3, 32), (38, 3, 64), (44, 1, 128), (45, 1, 256),
                  (46, 2, 512), (49, 1, 1024), (50, 1, 2048)]


def genome_dir(td):
    """references/synth under `td`: two chromosomes, N_SITES CpGs -> (its path, loci)"""
    from wgbs_tools_amd import synth
    names = [c for c, _ in GENOME_CHROMS]
    sizes = [s for _, s in GENOME_CHROMS]
    loci = synth.synth_loci(GENOME_SEED, sizes)
    return synth.write_genome(op.join(td, 'references', 'synth'), names, sizes, loci), loci


def region_text():
    """a region of chr2 that begins between two CpGs and ends on one"""
    from wgbs_tools_amd import synth
    loci = synth.synth_loci(GENOME_SEED, [s for _, s in GENOME_CHROMS]).astype(np.int64)
    c2 = loci[GENOME_CHROMS[0][1]:]
    return 'chr2:%d-%d' % (c2[300] - 1, c2[420])


def lines_text(reads, chrom='chr1'):
    return ''.join('%s\t%d\t%s\t%d\n' % (chrom, s, 'CT' * (ln // 2) + 'C' * (ln % 2), c) for s, ln, c in reads).encode()


def blocks_text(pairs, header=False, na_rows=False):
    """a 5-column blocks table of (startCpG, endCpG) pairs in the order given (na_rows: an NA row in front and one inside)"""
    rows = ['chr1\t%d\t%d\t%d\t%d\n' % (50 * s, 50 * (e - 1) + 2, s, e) for s, e in pairs]
    if na_rows:
        rows.insert(len(rows) // 2, 'chr1\t77\t79\tNA\tNA\n')
        rows.insert(0, 'chr1\t5\t7\tNA\tNA\n')
    return ('chr\tstart\tend\tstartCpG\tendCpG\n' if header else '') + ''.join(rows)


def _nested_pairs():
    s, e = HC.nested_blocks(8, N_SITES, 300)                   # the first block spans almost everything and ends behind the last one
    o = np.argsort(HC._rand(8, 41, s.size), kind='stable')      # rows shuffled
    return list(zip(s[o].tolist(), e[o].tolist()))


def _tied_pairs():
    """blocks with equal starts whose ends differ in their number of digits (9 / 10, 99 / 100 ...): byte order is not numeric order"""
    out = []
    for k, s in enumerate(range(5, 3900, 37)):
        out.append((s, s + 4 + k % 9))
        if k % 3 == 0:
            out.append((s, s + 95 + k % 12))
        if k % 5 == 0:
            out.append((s, s + 995 + k % 7))
    o = np.argsort(HC._rand(9, 42, len(out)), kind='stable')
    return [out[i] for i in o.tolist()]


_PAT = dict(seed=41, n_sites=N_SITES, n_reads=6000, n_chroms=2)
_PAT_LONG = dict(seed=42, n_sites=N_SITES, n_reads=3000, n_chroms=2, long_every=40, long_len=1500)

# name -> pat: generator parameters of homog_cases.pat_text, or reads: explicit (start, length, count) lines; m: --max_frag_size;
# where: the selecting arguments ('-L' is followed by the blocks table's text, which the test writes to a file)
CASES = {
    'wg_default': dict(pat=_PAT, m=30, where=[]),
    'wg_m1': dict(pat=_PAT, m=1, where=[]),
    'wg_m8_long': dict(pat=_PAT_LONG, m=8, where=[]),
    'wg_lds_plus5_long': dict(pat=_PAT_LONG, m=LDS_BINS + 5, where=[]),
    'wg_signed': dict(pat=dict(seed=43, n_sites=N_SITES, n_reads=3000, n_chroms=2, signed=True), m=12, where=[]),
    'sites': dict(pat=_PAT, m=30, where=['-s', '1200-1300']),
    'sites_long_reach': dict(pat=_PAT_LONG, m=40, where=['-s', '2000-2010']),       # long reads that start far in front still count
    'sites_one': dict(pat=_PAT, m=30, where=['-s', '2600']),
    'sites_empty': dict(reads=[(5, 3, 2), (900, 4, 1)], m=30, where=['-s', '100-200']),
    'region': dict(pat=_PAT, m=30, where=['-r', region_text]),
    'L_boundary': dict(reads=BOUNDARY_READS, m=30, where=['-L', blocks_text(BOUNDARY_BLOCKS)]),
    'L_boundary_last_nested': dict(reads=BOUNDARY_READS, m=30, where=['-L', blocks_text(BOUNDARY_BLOCKS_LAST_NESTED)]),
    'L_seg_header_na': dict(pat=_PAT, m=30, where=['-L', lambda: blocks_text(list(zip(*[a.tolist() for a in HC.segmentation_blocks(6, N_SITES, 12, 3)])),
                                                                                header=True, na_rows=True)]),
    'L_nested_shuffled': dict(pat=_PAT, m=16, where=['-L', lambda: blocks_text(_nested_pairs())]),
    'L_tied_starts': dict(pat=_PAT_LONG, m=30, where=['-L', lambda: blocks_text(_tied_pairs(), na_rows=True)]),
}


def case_pat(case):
    return HC.pat_text(**case['pat']) if 'pat' in case else lines_text(case['reads'])


def case_where(case):
    """the selecting arguments with their texts made: [] | ['-s', text] | ['-r', text] | ['-L', the table's text]"""
    return [w() if callable(w) else w for w in case['where']]


def table_pairs(text):
    """the usable (startCpG text, endCpG text) rows of a blocks table's text, in file order (no header, no NA rows)"""
    out = []
    for line in text.splitlines():
        tok = line.split('\t')
        if len(tok) >= 5 and tok[3].lstrip('-').isdigit() and tok[4].lstrip('-').isdigit():
            out.append((tok[3], tok[4]))
    return out


def random_world(rng):
    """-> (pat text, m, (starts, ends) in cview's order or None): sorted reads, some long, some counts large; blocks that nest, tie
    and leave gaps, or one block, or none"""
    n_sites = int(rng.integers(30, 3000))
    nr = int(rng.integers(1, 2500))
    st = np.sort(rng.integers(-3, n_sites + 5, nr))
    ln = rng.integers(1, int(rng.choice([6, 30, 400])), nr)
    if rng.random() < 0.3:
        ln[rng.integers(0, nr)] = int(rng.integers(1100, 2300))
    cnt = rng.integers(-20, int(rng.choice([50, 2 ** 31])), nr)
    alphabet = np.array(list('CTH.'))
    lines = ['chr%d\t%d\t%s\t%d\n' % (1 + st[i] % 2, st[i], ''.join(rng.choice(alphabet, ln[i])), cnt[i]) for i in range(nr)]
    for _ in range(int(rng.integers(0, 4))):
        lines.insert(int(rng.integers(0, len(lines) + 1)), '\n')
    text = ''.join(lines)
    if rng.random() < 0.3:
        text = text.rstrip('\n')                                    # a last line without its newline: BGZF feeds only (see the tests)
    m = int(rng.choice([1, 2, 7, 30, 500, LDS_BINS, LDS_BINS + 9]))
    kind = rng.random()
    if kind < 0.2:
        return text.encode(), m, None
    if kind < 0.4:
        s = int(rng.integers(1, n_sites))
        return text.encode(), m, (np.array([s]), np.array([s + int(rng.integers(1, 60))]))
    nb = int(rng.integers(2, 200))
    s = rng.integers(1, n_sites, nb)
    e = s + rng.integers(1, int(rng.choice([5, 40, 2 * n_sites])), nb)
    import frag_ref
    return text.encode(), m, frag_ref.cview_order([(str(a), str(b)) for a, b in zip(s.tolist(), e.tolist())])
