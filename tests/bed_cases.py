"""Seeded worlds and command lines of the beta2bed tests (tests/test_beta2bed_cpu.py, tests/test_gpu_beta2bed.py,
tests/golden/make_golden_beta2bed.py).  Everything is regenerated from the seed; tests/golden/bed_cases.json holds only what the
reference printed for it.

  small        3,000 sites on 4 chromosomes of 1, 255, 257 and 2,487 CpGs: chromosome borders inside a wavefront, on a workgroup
               border (site 256) and one past one (site 513); a two-character name and a long one; loci of 1 to 10 decimal digits, the
               last at 4,294,967,294; 600 consecutive sites without reads (sites 1000-1599: workgroups 4 and 5 write nothing); a
               .beta and an .lbeta
  every_pair   65,536 sites, (meth, cov) = (i >> 8, i & 255): every uint8 pair once, meth > cov included
  ties         uint16 pairs: every exact rational tie of the 3-digit rounding for cov in TIE_COVS, its neighbours one count either
               side, and 1/65535, 65535/1, 65535/65535
"""
import functools
import itertools
import os
import os.path as op

import numpy as np

SEED = 20261021
SMALL_NAMES = ['chr1', 'MT', 'chr7_KI270803v1_alternate', 'chrX']
SMALL_SIZES = [1, 255, 257, 2487]
SMALL_SITES = sum(SMALL_SIZES)
EMPTY_RUN = (1000, 1600)                                  # 0-based sites without reads
TIE_COVS = (16, 32, 64, 2000, 4000, 62500, 64000)
GRID = [dict(min_cov=c, mean=m, keep_na=k) for c, m, k in itertools.product((1, 2, 10), (False, True), (False, True))]


def small_loci():
    low = np.arange(9, 9 + 2 * 600, 2, dtype=np.int64)                                  # 1 to 4 digits
    high = np.unique(np.round(np.geomspace(2000, 4294967294, SMALL_SIZES[3] - low.size)).astype(np.int64))
    assert high.size == SMALL_SIZES[3] - low.size
    high[-1] = 4294967294
    parts = [np.array([5], dtype=np.int64), 7 + 3 * np.arange(SMALL_SIZES[1], dtype=np.int64),
             1000 + 301 * np.arange(SMALL_SIZES[2], dtype=np.int64), np.concatenate([low, high])]
    return np.concatenate(parts).astype(np.uint32)


def small_rows(elem):
    """[n, 2] (meth, cov): shallow sites around the thresholds 2 and 10, deep ones, meth > cov, orphans (meth > 0 = cov), the run
    without reads"""
    rng = np.random.default_rng([SEED, elem])
    n, top = SMALL_SITES, (255 if elem == 1 else 65535)
    cov = np.where(rng.random(n) < 0.7, rng.integers(0, 14, n), rng.integers(0, top + 1, n))
    meth = rng.integers(0, cov + 1)
    kind = rng.random(n)
    meth = np.where(kind < 0.05, rng.integers(0, top + 1, n), meth)
    orphan = (kind >= 0.05) & (kind < 0.07)
    cov = np.where(orphan, 0, cov)
    meth = np.where(orphan, rng.integers(1, top + 1, n), meth)
    rows = np.stack([meth, cov], axis=1).astype(np.uint8 if elem == 1 else np.uint16)
    rows[EMPTY_RUN[0]:EMPTY_RUN[1]] = 0
    rows[0] = (3, 7)
    rows[-1] = (top, top)
    return rows


def every_pair_rows():
    i = np.arange(65536)
    return np.stack([i >> 8, i & 255], axis=1).astype(np.uint8)


def tie_pairs():
    """(m, c) with m * 10^k / c exactly half way between two 3-digit numbers, for c in TIE_COVS, found by integer search"""
    out = []
    m = np.arange(1, 65536, dtype=np.int64)
    for c in TIE_COVS:
        e = np.full(m.size, -9, dtype=np.int64)            # floor(log10(m / c))
        for k in range(-5, 5):
            e = np.where(m * 10 ** max(-k, 0) >= c * 10 ** max(k, 0), k, e)
        num = np.where(e <= 2, m * 10 ** np.clip(2 - e, 0, None), m)
        den = np.where(e <= 2, c, c * 10 ** np.clip(e - 2, 0, None))
        out += [(int(x), c) for x in m[2 * (num % den) == den]]
    return out


@functools.lru_cache(maxsize=None)
def tie_rows():
    ties = tie_pairs()
    pairs = []
    for m, c in ties:
        pairs += [(m, c), (m, c - 1), (m, c + 1)] + ([(m - 1, c)] if m > 1 else []) + ([(m + 1, c)] if m < 65535 else [])
    pairs += [(1, 65535), (65535, 1), (65535, 65535)]
    return np.array(pairs, dtype=np.uint16), len(ties)


def one_chrom_loci(n):
    return (10 + 2 * np.arange(n, dtype=np.int64)).astype(np.uint32)


def worlds():
    """name -> dict(names, sizes, loci, files: {file name: rows})"""
    ties, _ = tie_rows()
    return {
        'small': dict(names=SMALL_NAMES, sizes=SMALL_SIZES, loci=small_loci(), files={'small.beta': small_rows(1), 'small.lbeta': small_rows(2)}),
        'every_pair': dict(names=['chr1'], sizes=[65536], loci=one_chrom_loci(65536), files={'every_pair.beta': every_pair_rows()}),
        'ties': dict(names=['chr1'], sizes=[len(ties)], loci=one_chrom_loci(len(ties)), files={'ties.lbeta': ties}),
    }


def small_beds(w):
    """name -> text of the bed files of the -L cases of the small world"""
    loci, cum = w['loci'].astype(np.int64), np.concatenate([[0], np.cumsum(w['sizes'])])
    x = loci[cum[3]:]                                      # chrX
    m = loci[cum[1]:cum[2]]                                # MT
    row = '%s\t%d\t%d\n'
    disjoint = [('MT', m[3], m[9] + 1), ('MT', m[200] - 1, m[254] + 40), ('chrX', x[5] - 1, x[5] + 1), ('chrX', x[700], x[703]),
                ('chr7_KI270803v1_alternate', 1, 1700), ('chr1', 1, 100)]
    deep = [('chrX', x[40], x[90]), ('chrX', x[50], x[80]), ('chrX', x[60], x[70]), ('chrX', x[65], x[300]), ('MT', m[0], m[254]), ('MT', m[250], m[254] + 5)]
    edges = [('chrX', x[1000] - 7, x[1000]), ('chrX', x[1700], x[1700] + 9), ('chrX', x[2486], x[2486]), ('chrX', x[2000] + 1, x[2001] - 1)]
    absent = [('chr9', 1, 100000), ('chrX', x[10], x[12]), ('chrY', 5, 50)]
    nothing = [('chrX', x[EMPTY_RUN[0] - cum[3] + 10], x[EMPTY_RUN[0] - cum[3] + 200]), ('chr9', 1, 5)]
    return {'disjoint.bed': ''.join(row % r for r in disjoint), 'deep.bed': '#chr\tstart\tend\n' + ''.join(row % r for r in deep),
            'edges.bed': ''.join(row % r for r in edges), 'absent.bed': ''.join(row % r for r in absent),
            'nothing.bed': ''.join(row % r for r in nothing)}


def cases():
    """name -> dict(world, file, opts (min_cov, mean, keep_na), where: None | ('-s', text) | ('-r', text) | ('-L', bed name), gz)"""
    out = {}
    for world, files in (('small', ('small.beta', 'small.lbeta')), ('every_pair', ('every_pair.beta',)), ('ties', ('ties.lbeta',))):
        for f in files:
            for o in GRID:
                name = '%s_c%d%s%s' % (f.replace('.', '_'), o['min_cov'], '_mean' if o['mean'] else '', '_na' if o['keep_na'] else '')
                out[name] = dict(world=world, file=f, opts=o, where=None, gz=False)
    x0 = sum(SMALL_SIZES[:3])
    plain, mean = dict(min_cov=1, mean=False, keep_na=True), dict(min_cov=2, mean=True, keep_na=False)
    extra = {
        'sites_inside': ('-s', '%d-%d' % (x0 + 300, x0 + 700)), 'sites_one': ('-s', '%d' % (x0 + 2487)), 'sites_border': ('-s', '250-260'),
        'region': ('-r', 'chrX:100-1,001'), 'region_mt': ('-r', 'MT'),
        'L_disjoint': ('-L', 'disjoint.bed'), 'L_deep': ('-L', 'deep.bed'), 'L_edges': ('-L', 'edges.bed'), 'L_absent': ('-L', 'absent.bed'),
        'L_nothing': ('-L', 'nothing.bed'),
    }
    for name, where in extra.items():
        out['small_' + name] = dict(world='small', file='small.beta', opts=plain, where=where, gz=False)
        out['small_' + name + '_mean'] = dict(world='small', file='small.lbeta', opts=mean, where=where, gz=False)
    out['small_empty_run'] = dict(world='small', file='small.beta', opts=dict(min_cov=1, mean=False, keep_na=False), where=('-s', '%d-%d' % (EMPTY_RUN[0] + 1, EMPTY_RUN[1] + 1)), gz=False)
    out['small_gz'] = dict(world='small', file='small.beta', opts=dict(min_cov=1, mean=True, keep_na=True), where=None, gz=True)
    return out


def argv_of(case, beta_path, ref, out_path, bed_dir=None):
    """the command line of a case (after `wgbstools beta2bed`)"""
    o = case['opts']
    argv = [beta_path, '--genome', ref, '-o', out_path, '-c', str(o['min_cov'])]
    argv += (['--mean'] if o['mean'] else []) + (['--keep_na'] if o['keep_na'] else [])
    if case['where']:
        flag, val = case['where']
        argv += [flag, op.join(bed_dir, val) if flag == '-L' else val]
    return argv


def write_world(td, name, w=None):
    """the genome directory, the beta files and (small) the bed files of a world under td/<name>/ -> dict(ref, dir)"""
    from wgbs_tools_amd import synth
    w = w or worlds()[name]
    d = op.join(td, name)
    os.makedirs(d, exist_ok=True)
    ref = synth.write_genome(op.join(d, 'references', name), w['names'], w['sizes'], w['loci'])
    for f, rows in w['files'].items():
        rows.tofile(op.join(d, f))
    if name == 'small':
        for f, text in small_beds(w).items():
            with open(op.join(d, f), 'w') as fh:
                fh.write(text)
    return dict(ref=ref, dir=d)
