"""Seeded inputs of the per-sample statistics tests (tests/test_stats_cpu.py, tests/test_gpu_stats.py): rows with every kind of
site the kernel distinguishes, and the range lists the issue names.  Everything is regenerated from the seed, nothing stored."""
import numpy as np

SIZES = (1, 63, 64, 65, 1023, 4097, 70001)
SAMPLES = (1, 3, 5)
CARRY_SITES, CARRY_SAMPLES = 5_000_000, 4


def make_rows(rng, n, elem, all_zero=False):
    """[n, 2] (meth, cov) rows of uint8 (elem 1) or uint16 (elem 2): shallow and deep sites, meth > cov sites, orphans
    (cov == 0 < meth), a saturated stretch and an all-zero stretch"""
    dt = np.uint8 if elem == 1 else np.uint16
    top = 255 if elem == 1 else 65535
    if all_zero:
        return np.zeros((n, 2), dtype=dt)
    cov = np.where(rng.random(n) < 0.5, rng.integers(0, 40, n), rng.integers(0, top + 1, n))
    meth = rng.integers(0, cov + 1)
    kind = rng.random(n)
    meth = np.where(kind < 0.05, rng.integers(0, top + 1, n), meth)                   # meth > cov (most of them)
    orphan = (kind >= 0.05) & (kind < 0.08)
    cov = np.where(orphan, 0, cov)
    meth = np.where(orphan, rng.integers(1, top + 1, n), meth)
    rows = np.stack([meth, cov], axis=1).astype(dt)
    if n >= 63:
        k = n // 8
        rows[k:2 * k + 1] = top                                                         # saturated
        rows[5 * k:6 * k + 1] = 0                                                       # no reads at all
    return rows


def world(n, n_samples, elem, seed=0):
    """`n_samples` rows of n sites; with three samples or more the second one is all zero (covered == 0)"""
    rng = np.random.default_rng([20261017, n, n_samples, elem, seed])
    return [make_rows(rng, n, elem, all_zero=(s == 1 and n_samples >= 3)) for s in range(n_samples)]


def range_sets(n, seed=0):
    """name -> list of 0-based half-open ranges over n sites, ascending and disjoint"""
    rng = np.random.default_rng([20261018, n, seed])
    out = {'whole': [(0, n)], 'none': [], 'to_the_end': [(max(0, n - 13), n)]}
    a = 1 if n > 1 else 0
    ln = min(n - a, 2001)
    out['odd'] = [(a, a + ln - (1 - ln % 2))] if n > 1 else [(0, 1)]                   # odd start, odd length
    k = max(1, n // 3) | 1
    out['adjacent'] = [(lo, min(n, lo + k)) for lo in range(0, n, k)][:64]
    out['one_site'] = [(i, i + 1) for i in range(0, min(n, 1500), 3)] + [(i, i + 1) for i in range(min(n, 1500), min(n, 1540))]
    long_at = set(rng.integers(0, 2000, 3).tolist())
    r, pos = [], 0
    for i in range(2000):
        pos = min(n, pos + int(rng.integers(0, 9)))
        ln = int(rng.integers(2000, 5000)) if i in long_at else int(rng.integers(0, 41))
        r.append((pos, min(n, pos + ln)))
        pos = r[-1][1]
    out['random'] = r
    return out


def carry_world():
    """CARRY_SAMPLES uint8 rows of CARRY_SITES sites whose exact ratio sum needs the upper 64 bits and carries into them many
    times (tests/test_stats_cpu.py checks that it does)"""
    rng = np.random.default_rng(20261019)
    rows = []
    for _ in range(CARRY_SAMPLES):
        cov = rng.integers(1, 256, CARRY_SITES, dtype=np.uint8)
        meth = (rng.integers(0, 256, CARRY_SITES, dtype=np.uint16) * cov.astype(np.uint16) >> 8).astype(np.uint8)     # meth <= cov
        rows.append(np.stack([meth, cov], axis=1))
    return rows


CARRY_RANGES = {'whole': [(0, CARRY_SITES)], 'split': [(0, 2_500_001), (2_500_001, CARRY_SITES)], 'inner': [(3, CARRY_SITES - 10)]}


# ---- the world of the command-line cases (tests/golden/make_golden_stats.py records what the reference prints for it) ----
GOLDEN_SEED = 20261020
GOLDEN_SITES = 40000                                    # = the site count of the blocks tables of tests/golden/block_cases.json
GOLDEN_CHROMS = [('chr1', 25000), ('chr2', 12000), ('chrX', 3000)]
LONG_NAMES = ['Liver-Hepatocytes-Z000000T7.hg19.merged.dedup.sorted', 'Blood-Granulocytes-Z000000TZ.hg19.merged.dedup',
              'Colon-Ep-Z000000X1']


def golden_world(td):
    """Write the genome directory (references/synth), four .beta and two .lbeta files and three long-named copies under `td`.
    smp1 has a stretch without reads, smp3 one site with meth > 0 = cov (numpy's inf).  -> dict(ref, names, sizes, loci)"""
    import os
    import os.path as op
    import cases
    from wgbs_tools_amd import synth
    names = [c for c, _ in GOLDEN_CHROMS]
    sizes = [s for _, s in GOLDEN_CHROMS]
    loci = synth.synth_loci(GOLDEN_SEED, sizes)
    ref = synth.write_genome(op.join(td, 'references', 'synth'), names, sizes, loci)
    for s in range(4):
        d = synth.synth_betas(GOLDEN_SEED, s, 0, GOLDEN_SITES)
        if s == 1:
            d[7000:9500] = 0
        if s == 3:
            d[123] = (5, 0)
        d.tofile(op.join(td, 'smp%d.beta' % s))
        if s < 2:
            cases.lbeta_twin(d).tofile(op.join(td, 'smp%d.lbeta' % s))
        if s < 3:
            d.tofile(op.join(td, LONG_NAMES[s] + '.beta'))
    return dict(ref=ref, names=names, sizes=sizes, loci=loci)


def golden_bed(world):
    """text of the 3-column bed of the `beta_stats -L` case: regions that end on a CpG, start on one, touch, repeat, overlap,
    hold no CpG, lie on an unknown chromosome, and a comment line"""
    loci, sizes = world['loci'].astype(np.int64), world['sizes']
    c1, c2 = loci[:sizes[0]], loci[sizes[0]:sizes[0] + sizes[1]]
    rows = [('chr1', c1[10], c1[50]), ('chr1', c1[50], c1[60]), ('chr1', c1[100] - 1, c1[100]), ('chr1', c1[200] + 1, c1[201] - 1),
            ('chr2', c2[5] - 1, c2[4000]), ('chr2', c2[3000], c2[4500] + 1), ('chr1', c1[10], c1[50]), ('chr9', 5, 5000),
            ('chr1', c1[20000] - 1, c1[24999] + 10), ('chr1', c1[700], c1[650])]
    return '#chr\tstart\tend\n' + ''.join('%s\t%d\t%d\textra\n' % r for r in rows)
