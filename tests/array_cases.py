"""Seeded worlds, map files, ref files and command lines of the beta_to_450k tests (tests/test_450k_cpu.py, tests/test_gpu_450k.py,
tests/golden/make_golden_450k.py).  Everything is regenerated from the seed; tests/golden/array_cases.json holds only what the
reference printed for it.

  small        3,000 sites on 3 chromosomes, up to 65 samples (sample k of a width is drawn from (SEED, width, k)), as .beta and as
               .lbeta; a THREE-column map of 420 probes in no order: 450 and 850 rows, sites 1 and 3,000, two probes on one site,
               rows with an empty cpg, an ID with two rows, an ID that holds a comma
  small2       the same genome and files behind a TWO-column map
  every_pair   65,536 sites, (meth, cov) = (i >> 8, i & 255): every uint8 pair once, meth > cov included; a probe per site
  ties         uint16 pairs on an exact tie of the "%.3f" rounding, 2000 m = odd x c (every c that has one, its first TIE_ODDS odd
               multiples), then 65535/1, 1/65535, 0/0 and 7/0; a probe per site, two-column map
"""
import functools
import gzip
import math
import os
import os.path as op

import numpy as np

import bed_cases as BC

SEED = 20261102
SMALL_NAMES = ['chr1', 'chr2', 'chrX']
SMALL_SIZES = [700, 1300, 1000]
SMALL_SITES = sum(SMALL_SIZES)
MAX_SAMPLES = 65
TIE_ODDS = 16
COMMA_ID = 'cg,0000comma'
TWICE_ID = 'cg00000777'                                    # two rows of the map
EMPTY_IDS = ['cg00009001', 'cg00009002', 'cg00009003']     # rows with an empty cpg
THRESHOLDS = (0, 1, 3, 300, 70000)


def sample_rows(elem, k):
    """[n, 2] (meth, cov) of sample k: shallow sites around the threshold 3, deep ones, sites without reads, meth > cov, orphans"""
    rng = np.random.default_rng([SEED, elem, k])
    n, top = SMALL_SITES, (255 if elem == 1 else 65535)
    cov = np.where(rng.random(n) < 0.6, rng.integers(0, 7, n), rng.integers(0, top + 1, n))
    meth = rng.integers(0, cov + 1)
    kind = rng.random(n)
    meth = np.where(kind < 0.04, rng.integers(0, top + 1, n), meth)
    orphan = (kind >= 0.04) & (kind < 0.08)
    cov = np.where(orphan, 0, cov)
    meth = np.where(orphan, rng.integers(1, top + 1, n), meth)
    return np.stack([meth, cov], axis=1).astype(np.uint8 if elem == 1 else np.uint16)


@functools.lru_cache(maxsize=None)
def tie_pairs():
    """(m, c) with 1000 m / c exactly half way between two integers: 2000 m = k c with k odd.  With g = gcd(c, 2000) this asks for
    2000 / g odd (16 divides c) and k = (2000 / g) j, j odd: m = j c / g."""
    out = []
    for c in range(16, 65536, 16):
        g = math.gcd(c, 2000)
        assert (2000 // g) % 2 == 1
        out += [(j * (c // g), c) for j in range(1, 2 * TIE_ODDS, 2) if j * (c // g) <= 65535]
    return out


def tie_rows():
    return np.array(tie_pairs() + [(65535, 1), (1, 65535), (0, 0), (7, 0)], dtype=np.uint16)


def small_map():
    """rows (ilmn, cpg or None, array) of the small world's map"""
    rng = np.random.default_rng([SEED, 7])
    cpg = rng.integers(1, SMALL_SITES + 1, 420)
    cpg[:6] = (1, SMALL_SITES, 1500, 1500, 701, 700)
    arr = np.where(rng.random(420) < 0.6, 450, 850)
    ids = ['cg%08d' % i for i in rng.permutation(90000)[:420] + 1000]
    rows = [[i, int(c), int(a)] for i, c, a in zip(ids, cpg, arr)]
    rows[10][0] = rows[200][0] = TWICE_ID
    rows[10][2], rows[200][2] = 450, 850
    rows[20][0], rows[20][2] = COMMA_ID, 450
    for at, i in zip((30, 31, 300), EMPTY_IDS):
        rows[at] = [i, None, 450 if at != 31 else 850]
    return rows


def dense_map(n):
    return [['cg%08d' % (i + 1), i + 1, 450] for i in range(n)]


def map_text(rows, columns):
    return ''.join('\t'.join('' if v is None else str(v) for v in r[:columns]) + '\n' for r in rows)


@functools.lru_cache(maxsize=None)
def worlds():
    """name -> dict(names, sizes, loci, elem -> list of sample rows | files, map rows, map columns)"""
    small = dict(names=SMALL_NAMES, sizes=SMALL_SIZES, loci=BC.one_chrom_loci(SMALL_SITES), map=small_map())
    small['samples'] = {elem: [sample_rows(elem, k) for k in range(MAX_SAMPLES)] for elem in (1, 2)}
    ties = tie_rows()
    return {
        'small': dict(small, map_columns=3),
        'small2': dict(small, map_columns=2),
        'every_pair': dict(names=['chr1'], sizes=[65536], loci=BC.one_chrom_loci(65536), map=dense_map(65536), map_columns=3,
                           samples={1: [BC.every_pair_rows()]}),
        'ties': dict(names=['chr1'], sizes=[len(ties)], loci=BC.one_chrom_loci(len(ties)), map=dense_map(len(ties)), map_columns=2, samples={2: [ties]}),
    }


def small_refs():
    """name -> text of the --ref files of the small worlds"""
    m = small_map()
    ids = [r[0] for r in m]
    rng = np.random.default_rng([SEED, 8])
    pick = [i for i in (ids[j] for j in rng.permutation(420)) if i not in EMPTY_IDS][:60]
    quote = lambda i: '"%s"' % i if ',' in i else i
    unknown = ['cg99%06d' % i for i in range(7)]
    return {
        'ref_header.csv': 'IlmnID,Name,CHR\n' + ''.join('%s,%s,7\n' % (quote(i), quote(i)) for i in pick),
        'ref_plain.csv': ''.join(quote(i) + '\n' for i in pick[::-1]),
        'ref_extra.csv': ''.join('%s,0.5,x y\n' % quote(i) for i in pick[10:40]),
        'ref_unknown1.csv': ''.join(i + '\n' for i in [pick[0], unknown[0], pick[1]]),
        'ref_unknown7.csv': 'probe\n' + ''.join(i + '\n' for i in unknown[:3] + pick[5:9] + unknown[3:] + [EMPTY_IDS[2]]),
        'ref_repeats.csv': ''.join(i + '\n' for i in [pick[2], TWICE_ID, pick[2], pick[3], TWICE_ID, pick[2]]),
        'ref_empty_first.csv': ',1\n' + ''.join('%s,2\n' % i for i in pick[20:25]),
        'ref_quoted.csv': ''.join(i + '\n' for i in [pick[4], '"%s"' % COMMA_ID, ids[0], ids[1]]),
        'ref_none_known.csv': ''.join(i + '\n' for i in unknown[:2]),
    }


def file_name(elem, k):
    return 's%02d.%s' % (k, 'beta' if elem == 1 else 'lbeta')


def cases():
    """name -> dict(world, elem, files: list of (directory under the world's or '', sample index), c, epic, ref: name or None)"""
    out = {}

    def add(name, world, elem, files, c, epic=False, ref=None):
        out[name] = dict(world=world, elem=elem, files=[f if isinstance(f, tuple) else ('', f) for f in files], c=c, epic=epic, ref=ref)

    for n in (1, 2, 33):
        for c in THRESHOLDS:
            add('small_beta_f%d_c%d' % (n, c), 'small', 1, range(n), c)
    for n, cs in ((1, (0, 3, 300)), (2, (0, 3, 300)), (33, (3,))):
        for c in cs:
            add('small_lbeta_f%d_c%d' % (n, c), 'small', 2, range(n), c)
    add('small_beta_f2_c3_epic', 'small', 1, range(2), 3, epic=True)
    add('small_lbeta_f1_c1_epic', 'small', 2, range(1), 1, epic=True)
    for ref in small_refs():
        add('small_beta_f2_c3_' + ref[:-4], 'small', 1, (3, 4), 3, ref=ref)
    add('small_beta_f1_c3_ref_unknown7_epic', 'small', 1, (5,), 3, epic=True, ref='ref_unknown7.csv')
    add('small_lbeta_f2_c0_ref_plain', 'small', 2, (1, 0), 0, ref='ref_plain.csv')
    add('small_beta_same_base_name', 'small', 1, [('a', 0), ('', 1), ('b', 2)], 3)
    add('small2_beta_f1_c3', 'small2', 1, range(1), 3)
    add('small2_beta_f1_c3_epic', 'small2', 1, range(1), 3, epic=True)
    add('small2_lbeta_f1_c1_ref_unknown1', 'small2', 2, range(1), 1, ref='ref_unknown1.csv')
    for c in (0, 1, 3, 300):
        add('every_pair_c%d' % c, 'every_pair', 1, range(1), c)
    for c in (0, 1):
        add('ties_c%d' % c, 'ties', 2, range(1), c)
    add('small_beta_short_first_file', 'small', 1, [('short', 0), ('', 1)], 3)
    return out


def case_paths(case, where):
    """the case's beta files under a written world"""
    d = where[case['world']]['dir']
    return [op.join(d, sub, 'ab.beta' if sub == 'short' else file_name(case['elem'], 0 if sub in ('a', 'b') else k)) for sub, k in case['files']]


def case_rows(case, w):
    """the rows the case's files hold, in argument order"""
    return [w['samples'][case['elem']][k] for _, k in case['files']]


def argv_of(case, where, out_path):
    """the command line of a case (after `wgbstools beta_to_450k`)"""
    d = where[case['world']]
    argv = case_paths(case, where) + ['--genome', d['ref'], '-o', out_path, '-c', str(case['c'])]
    argv += ['--EPIC'] if case['epic'] else []
    argv += ['--ref', op.join(d['dir'], case['ref'])] if case['ref'] else []
    return argv


def write_world(td, name, w=None, n_samples=33):
    """the genome directory with its map, the beta files of the first n_samples samples and (small worlds) the ref files, the two
    directories a/ and b/ that hold samples 0 and 2 under sample 0's file name and a file of 10 sites under td/<name>/
    -> dict(ref, dir, map)"""
    from wgbs_tools_amd import synth
    w = w or worlds()[name]
    d = op.join(td, name)
    os.makedirs(d, exist_ok=True)
    ref = synth.write_genome(op.join(d, 'references', 'hg38'), w['names'], w['sizes'], w['loci'])
    map_path = op.join(ref, 'ilmn2CpG.tsv.gz')
    with gzip.open(map_path, 'wt') as f:
        f.write(map_text(w['map'], w['map_columns']))
    for elem, samples in w['samples'].items():
        for k, rows in enumerate(samples[:n_samples]):
            rows.tofile(op.join(d, file_name(elem, k)))
    if name.startswith('small'):
        for f, text in small_refs().items():
            with open(op.join(d, f), 'w') as fh:
                fh.write(text)
        for sub, k in (('a', 0), ('b', 2)):
            os.makedirs(op.join(d, sub), exist_ok=True)
            w['samples'][1][k].tofile(op.join(d, sub, file_name(1, 0)))
        os.makedirs(op.join(d, 'short'), exist_ok=True)
        w['samples'][1][0][:10].tofile(op.join(d, 'short', 'ab.beta'))
    return dict(ref=ref, dir=d, map=map_path)
