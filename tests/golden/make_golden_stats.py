#!/usr/bin/env python3
"""Golden text of `wgbstools beta_cov` and `beta_stats` from the REFERENCE ITSELF: runs only in the build container, imports
/root/reference/src/python/{beta_cov,beta_stats}.py from where they lie and records what their main() prints for the seeded
world of tests/stats_cases.py (golden_world: ~40 K sites, four .beta and two .lbeta files, a tiny genome directory): whole
files, -s, -r, `beta_cov -L` with the `nice` and `ragged` blocks tables of block_cases.json, and the table at widths 120 (with
names long enough to wrap) and 60.

The reference resolves -s / -r through `tabix | awk` pipelines: they run for real on the stand-in of make_golden_convert.py
(the image has no htslib).  `beta_stats -L` needs `tabix -R`, which the stand-in does not speak: when no real tabix is on the
PATH (shutil.which; `tabix_for_L` in the fixture says which it was) the expected text of that case comes from the reference's
own print_stats fed the rows that the rule `start < position <= end` selects (tests/stats_ref.py picks them with plain numpy
comparisons per bed row, no searchsorted), laid out by pandas as the reference's main() does.

The comparison with an exact sum rests on one condition, asserted here for every recorded case: numpy's own mean-methylation
value before .round(2) lies at least 1e-6 from a x.xx5 boundary, so its pairwise float sum and the exact sum print the same
two decimals.  Change the seed (stats_cases.GOLDEN_SEED), not the tolerance, if a case lands closer.

Usage:  python tests/golden/make_golden_stats.py
"""
import contextlib
import io
import json
import os
import os.path as op
import shutil
import stat
import sys
import tempfile

import numpy as np

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
sys.path.insert(0, '/root/reference/src/python')

import stats_cases as SC                       # noqa: E402
from make_golden_convert import TABIX_SHIM     # noqa: E402


def cases_of(world):
    """name -> (command, argv with file names relative to the world's directory)"""
    c1 = world['loci'][:world['sizes'][0]].astype(np.int64)
    betas = ['smp%d.beta' % s for s in range(4)]
    lbetas = ['smp0.lbeta', 'smp1.lbeta']
    longs = [n + '.beta' for n in SC.LONG_NAMES]
    region = 'chr1:%d-%d' % (c1[1000], c1[9000] + 3)
    out = {}
    for cmd in ('beta_cov', 'beta_stats'):
        out[cmd + '_whole'] = (cmd, betas)
        out[cmd + '_lbeta'] = (cmd, lbetas)
        out[cmd + '_sites'] = (cmd, betas + ['-s', '1001-21002'])
        out[cmd + '_sites_lbeta'] = (cmd, lbetas + ['-s', '6999-9600'])
        out[cmd + '_region'] = (cmd, betas[::-1] + ['-r', region])
    out['beta_cov_one_site'] = ('beta_cov', betas + ['-s', '124'])
    out['beta_cov_L_nice'] = ('beta_cov', betas + ['-L', 'nice.bed'])
    out['beta_cov_L_ragged'] = ('beta_cov', betas + ['-L', 'ragged.bed'])
    out['beta_cov_L_nice_lbeta'] = ('beta_cov', lbetas + ['-L', 'short.bed'])
    out['beta_stats_long_names'] = ('beta_stats', longs)
    out['beta_stats_width60'] = ('beta_stats', betas + ['-w', '60'])
    out['beta_stats_long_width60'] = ('beta_stats', longs + betas[:1] + ['--width', '60', '-s', '7001-9400'])
    out['beta_stats_L'] = ('beta_stats', betas + lbetas[:1] + ['-L', 'regions.bed'])
    return out


def write_blocks(path, rows):
    with open(path, 'w') as f:
        for c, s, e, a, b in rows:
            f.write('%s\t%d\t%d\t%s\t%s\n' % (c, s, e, 'NA' if a is None else a, 'NA' if b is None else b))


def main():
    import pandas as pd
    import genomic_region as rg
    import beta_cov as rcov
    import beta_stats as rstats
    import stats_ref as SR
    td = tempfile.mkdtemp()
    world = SC.golden_world(td)
    names, sizes, refdir = world['names'], world['sizes'], world['ref']
    real_tabix = shutil.which('tabix')
    shim = op.join(td, 'bin')
    os.makedirs(shim)
    with open(op.join(shim, 'tabix'), 'w') as f:
        f.write(TABIX_SHIM)
    os.chmod(op.join(shim, 'tabix'), os.stat(op.join(shim, 'tabix')).st_mode | stat.S_IEXEC)
    if not real_tabix:
        os.environ['PATH'] = shim + os.pathsep + os.environ['PATH']
    with open(op.join(HERE, 'block_cases.json')) as f:
        tables = json.load(f)['tables']
    write_blocks(op.join(td, 'nice.bed'), tables['nice']['rows'])
    write_blocks(op.join(td, 'ragged.bed'), tables['ragged']['rows'])
    write_blocks(op.join(td, 'short.bed'), [r for r in tables['nice']['rows'] if r[4] - r[3] < 1000])     # (uint16 rows: blocks of at most 65536 sites)
    with open(op.join(td, 'regions.bed'), 'w') as f:
        f.write(SC.golden_bed(world))

    class FakeGenome:
        def __init__(self, name=None):
            self.genome = 'synth'
            self.dict_path = op.join(refdir, 'CpG.bed.gz')
            self.revdict_path = op.join(refdir, 'rev.CpG.bed.gz')
            self.annotations = None
            self.ilmn2cpg_dict = None

        def get_chrom_cpg_size_table(self):
            return pd.DataFrame({'chr': names, 'size': sizes})

        def get_chrom_size_table(self):
            return pd.read_csv(op.join(refdir, 'chrome.size'), sep='\t', header=None, names=['chr', 'size'])

        def get_chroms(self):
            return tuple(names)

        def get_nr_sites(self):
            return int(sum(sizes))

    class FakePool:
        def __init__(self, n):
            pass

        def starmap(self, f, ps):
            return [f(*p) for p in ps]

        def close(self):
            pass

        def join(self):
            pass

    rg.GenomeRefPaths = FakeGenome
    rg.get_genome_name = lambda gname: 'synth'          # (the reference looks for its own references/default link first)
    rcov.Pool = FakePool
    rstats.Pool = FakePool
    raw_means = []
    print_stats = rstats.print_stats

    def recording_print_stats(beta_path, data):
        with np.errstate(divide='ignore', invalid='ignore'):
            raw_means.append(float(np.nanmean(data[:, 0] / data[:, 1] * 100)))
        return print_stats(beta_path, data)
    rstats.print_stats = recording_print_stats

    def bed_selected_rows(beta_path):
        """the rows `tabix -R` would select, by the rule alone: position p of the bed row's chromosome with start < p <= end"""
        loci = world['loci'].astype(np.int64)
        first = dict(zip(names, np.cumsum([0] + sizes[:-1]).tolist()))
        take = np.zeros(len(loci), dtype=bool)
        for line in SC.golden_bed(world).splitlines():
            if line.startswith('#'):
                continue
            c, a, b = line.split('\t')[:3]
            if c in first:
                lo, n = first[c], sizes[names.index(c)]
                take[lo:lo + n] |= (loci[lo:lo + n] > int(a)) & (loci[lo:lo + n] <= int(b))
        dt = np.uint16 if beta_path.endswith('.lbeta') else np.uint8
        return np.fromfile(beta_path, dtype=dt).reshape(-1, 2)[take]

    fixture = {'seed': SC.GOLDEN_SEED, 'n_sites': SC.GOLDEN_SITES, 'tabix_for_L': 'tabix' if real_tabix else 'print_stats on the rows of the rule',
               'cases': {}}
    cwd = os.getcwd()
    os.chdir(td)
    try:
        for name, (cmd, argv) in cases_of(world).items():
            del raw_means[:]
            out = io.StringIO()
            sys.argv = [cmd] + argv + ['--genome', 'synth', '-@', '1']
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
                if name == 'beta_stats_L' and not real_tabix:
                    betas = [a for a in argv if a.endswith('beta')]
                    df = pd.concat([rstats.print_stats(b, bed_selected_rows(b)) for b in betas], axis=1)
                    pd.set_option('display.max_columns', None)
                    pd.set_option('display.max_rows', None)
                    pd.set_option('display.width', 120)
                    print(df.T)
                else:
                    (rcov if cmd == 'beta_cov' else rstats).main()
            for v in raw_means:                                     # the condition the exact sum rests on
                if np.isfinite(v):
                    frac = (v * 100.0) % 1.0
                    assert abs(frac - 0.5) >= 1e-4, (name, v)       # 1e-6 in the mean = 1e-4 in hundredths
            fixture['cases'][name] = {'cmd': cmd, 'args': argv, 'stdout': out.getvalue(), 'raw_means': [repr(v) for v in raw_means]}
            print('==', name, ' '.join(argv[-4:]))
            print(out.getvalue(), end='')
    finally:
        os.chdir(cwd)
        shutil.rmtree(td, ignore_errors=True)
    path = op.join(HERE, 'stats_cases.json')
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=0)
    print('wrote stats_cases.json (%.0f KB)' % (op.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
