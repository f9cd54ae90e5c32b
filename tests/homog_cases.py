"""Seeded pat files and blocks tables of the `wgbstools homog` cases (tests/golden/make_golden_homog.py writes the reference's
output for them into tests/golden/homog_cases.json; tests/test_homog_cpu.py and tests/test_gpu_homog.py rebuild the inputs).
Deterministic across platforms: every random number is synth.hash_at (splitmix64)."""
import numpy as np

from wgbs_tools_amd.synth import hash_at

U = np.uint64


def _rand(seed, stream, n):
    return hash_at(seed, stream, np.arange(n, dtype=np.int64))


def genome(n_sites, n_chroms):
    """chromosome names and their CpG counts: n_chroms chromosomes of about equal size"""
    cut = np.linspace(0, n_sites, n_chroms + 1).astype(np.int64)
    return ['chr%d' % (c + 1) for c in range(n_chroms)], np.diff(cut).tolist()


def _chrom_of(cpg, names, sizes):
    cum = np.cumsum(sizes)
    return [names[min(int(i), len(names) - 1)] for i in np.searchsorted(cum, np.maximum(cpg, 1) - 1, 'right')]


def pat_text(seed, n_sites, n_reads, n_chroms=1, max_len=12, long_every=0, long_len=2000, max_count=40, signed=False):
    """A pat file's text (bytes), sorted by start: reads of 1..max_len sites over {C, T, H, .} starting at -3 .. n_sites + 4
    (a few hang over both ends of the genome), counts 1..max_count; long_every > 0: every long_every-th read is long_len..
    long_len + 63 sites long; signed: some counts negative, some written with a '+'."""
    start = np.sort((_rand(seed, 1, n_reads) % U(n_sites + 8)).astype(np.int64) - 3)
    h = _rand(seed, 2, n_reads)
    ln = 1 + (h % U(max_len)).astype(np.int64)
    if long_every:
        ln[::long_every] = long_len + ((h[::long_every] >> U(40)) % U(64)).astype(np.int64)
    cnt = 1 + ((h >> U(8)) % U(max_count)).astype(np.int64)
    neg = np.zeros(n_reads, dtype=bool)
    plus = np.zeros(n_reads, dtype=bool)
    if signed:
        neg = ((h >> U(24)) % U(7)) == 0
        plus = ~neg & (((h >> U(32)) % U(5)) == 0)
    alphabet = np.frombuffer(b'CCCTTTH.', dtype=np.uint8)
    chars = alphabet[(_rand(seed, 3, int(ln.sum())) & U(7)).astype(np.int64)].tobytes().decode()
    off = np.concatenate([[0], np.cumsum(ln)]).tolist()
    names, sizes = genome(n_sites, n_chroms)
    chroms = _chrom_of(start, names, sizes)
    out = []
    for i in range(n_reads):
        c = int(cnt[i])
        ctext = ('-%d' % c) if neg[i] else (('+%d' % c) if plus[i] else str(c))
        out.append('%s\t%d\t%s\t%s\n' % (chroms[i], start[i], chars[off[i]:off[i + 1]], ctext))
    return ''.join(out).encode()


def segmentation_blocks(seed, n_sites, max_len=16, gap_every=5):
    """a partition of CpGs 1..n_sites into blocks of 1..max_len sites, every gap_every-th one dropped (a gap): the shape of
    what `segment` writes -> (startCpG, endCpG) int64 arrays, sorted"""
    n = 2 * n_sites // max(1, max_len // 2) + 16
    ln = 1 + (_rand(seed, 11, n) % U(max_len)).astype(np.int64)
    ends = 1 + np.cumsum(ln)
    starts = ends - ln
    keep = (ends <= n_sites + 1) & ((_rand(seed, 12, n) % U(gap_every)) != 0)
    return starts[keep], ends[keep]


def nested_blocks(seed, n_sites, n_blocks):
    """overlapping and nested blocks, sorted by (startCpG, endCpG); the first block spans almost everything and runs past the
    last block's end (the reference's end-of-blocks rule then drops the reads in its tail)"""
    h = _rand(seed, 21, n_blocks)
    s = 1 + (h % U(n_sites - 20)).astype(np.int64)
    e = s + 1 + ((h >> U(20)) % U(30)).astype(np.int64)
    s = np.concatenate([[2], s])
    e = np.concatenate([[n_sites + 2], e])
    o = np.lexsort((e, s))
    s, e = s[o], e[o]
    assert e[0] > e[-1]
    return s, e


def blocks_text(starts, ends, n_sites, n_chroms=1, header=False, comments=False, order=None):
    """the text of a blocks table: chr, start, end (base pairs, 50 per CpG), startCpG, endCpG; rows in `order` (default: as
    given); header: the reference's header line; comments: '#' lines before it and between rows"""
    names, sizes = genome(n_sites, n_chroms)
    chroms = _chrom_of(starts, names, sizes)
    rows = ['%s\t%d\t%d\t%d\t%d\n' % (chroms[i], 50 * starts[i], 50 * (ends[i] - 1) + 2, starts[i], ends[i]) for i in range(len(starts))]
    if order is not None:
        rows = [rows[i] for i in order]
    out = []
    if comments:
        out.append('# blocks of a synthetic genome\n')
    if header:
        out.append('chr\tstart\tend\tstartCpG\tendCpG\n')
    for i, r in enumerate(rows):
        if comments and i and i % 97 == 0:
            out.append('#\tskipped\n')
        out.append(r)
    return ''.join(out)


def _seg(seed=1):
    return dict(kind='segmentation', seed=seed, n_sites=60000, n_chroms=3, max_len=12, gap_every=5)


# name -> generator parameters of the pat file, the blocks table, and the command-line arguments after the file names
CASES = {
    'seg_l3': dict(pat=dict(seed=31, n_sites=60000, n_reads=90000, n_chroms=3), blocks=_seg(), args=[]),
    'seg_l5': dict(pat=dict(seed=31, n_sites=60000, n_reads=90000, n_chroms=3), blocks=_seg(), args=['-l', '5']),
    'seg_l2_t': dict(pat=dict(seed=31, n_sites=60000, n_reads=90000, n_chroms=3), blocks=_seg(), args=['-l', '2', '-t', '0.25,0.75']),
    'seg_inclusive': dict(pat=dict(seed=31, n_sites=60000, n_reads=90000, n_chroms=3), blocks=_seg(), args=['--inclusive']),
    'nested': dict(pat=dict(seed=32, n_sites=3000, n_reads=20000), blocks=dict(kind='nested', seed=2, n_sites=3000, n_blocks=700), args=[]),
    'nested_inclusive_l4': dict(pat=dict(seed=32, n_sites=3000, n_reads=20000), blocks=dict(kind='nested', seed=2, n_sites=3000, n_blocks=700),
                                args=['--inclusive', '-l', '4']),
    'unsorted': dict(pat=dict(seed=33, n_sites=4000, n_reads=20000), blocks=dict(kind='unsorted', seed=3, n_sites=4000), args=[]),
    'duplicates': dict(pat=dict(seed=34, n_sites=4000, n_reads=20000), blocks=dict(kind='duplicates', seed=4, n_sites=4000), args=[]),
    'header_comments': dict(pat=dict(seed=35, n_sites=4000, n_reads=20000), blocks=dict(kind='segmentation', seed=5, n_sites=4000, n_chroms=1,
                                                                                        max_len=12, gap_every=4, header=True, comments=True), args=[]),
    'deep_bin8': dict(pat=dict(seed=36, n_sites=60, n_reads=40000, max_count=400), blocks=dict(kind='segmentation', seed=6, n_sites=60, n_chroms=1,
                                                                                               max_len=8, gap_every=6), args=['--binary']),
    'deep_bin16': dict(pat=dict(seed=36, n_sites=60, n_reads=40000, max_count=400), blocks=dict(kind='segmentation', seed=6, n_sites=60, n_chroms=1,
                                                                                                max_len=8, gap_every=6), args=['--binary', '--nr_bits', '16']),
    'long_reads_signed': dict(pat=dict(seed=37, n_sites=8000, n_reads=6000, long_every=50, long_len=2000, signed=True),
                              blocks=dict(kind='segmentation', seed=7, n_sites=8000, n_chroms=1, max_len=40, gap_every=5), args=['-l', '4']),
}


def case_blocks(spec):
    """-> (startCpG, endCpG in file row order, the blocks file's text)"""
    kind = spec['kind']
    n_sites = spec['n_sites']
    n_chroms = spec.get('n_chroms', 1)
    if kind == 'segmentation':
        s, e = segmentation_blocks(spec['seed'], n_sites, spec['max_len'], spec['gap_every'])
        return s, e, blocks_text(s, e, n_sites, n_chroms, spec.get('header', False), spec.get('comments', False))
    if kind == 'nested':
        s, e = nested_blocks(spec['seed'], n_sites, spec['n_blocks'])
        return s, e, blocks_text(s, e, n_sites, n_chroms)
    if kind == 'unsorted':
        # equal starts with unequal ends in both orders, then the rows shuffled: the re-ordering quirk
        s, e = segmentation_blocks(spec['seed'], n_sites, 12, 4)
        s2, e2 = s[::3], np.minimum(e[::3] + 5, n_sites + 1)
        s, e = np.concatenate([s, s2]), np.concatenate([e, e2])
        o = np.argsort(_rand(spec['seed'], 31, s.size), kind='stable')
        return s[o], e[o], blocks_text(s, e, n_sites, n_chroms, order=o)
    if kind == 'duplicates':
        s, e = segmentation_blocks(spec['seed'], n_sites, 12, 4)
        rep = 1 + (np.arange(s.size) % 7 == 0) + (np.arange(s.size) % 21 == 0)       # some rows twice, some three times
        s, e = np.repeat(s, rep), np.repeat(e, rep)
        return s, e, blocks_text(s, e, n_sites, n_chroms)
    raise ValueError(kind)


def case_pat(spec):
    return pat_text(**spec)
