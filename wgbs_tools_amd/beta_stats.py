"""`wgbstools beta_stats` on MI355X: per beta file the mean methylation, the covered sites (any depth and 10+), the largest
and the mean depth — the table a user reads before choosing the samples that go into `segment`.

Drop-in for the reference's src/python/beta_stats.py (same flags, same printed table), written against its contract
(beta_stats.py:28-56 print_stats, :59-70 load_beta_by_bed, :96-100 the table):

    numbers   all five come from the integers of ONE launch of k_sample_stats over all the files (csrc/stats_kernels.h,
              wgbsseg_sample_stats; beta_cov.file_stats), made into text exactly as the reference makes them:
                mean meth. (%)       np.nanmean(meth / cov * 100).round(2): the sum of the doubles fl(fl(meth / cov) * 100) over the
                                     covered sites, divided by their number.  The device returns that sum EXACTLY (a 128-bit
                                     integer of 2^-62 units); it is rounded once to a double here.  numpy's own pairwise float
                                     sum may differ from it in the last bits, which shows in the two printed decimals only when the
                                     mean lies within ~1e-12 of a x.xx5 boundary.  'nan' without a covered site; 'inf' when a site
                                     has meth > 0 = cov (numpy's inf).
                covered sites        f'{(cov > 0).sum():,}';   covered sites (10+): f'{(cov >= 10).sum():,}'
                max depth            f'{cov.max():,}';   mean depth: f'{cov.mean().round(2):,}' = cov_sum / n_sites
    -s / -r   only that slice of every file is read and uploaded
    -L BED    the UNIQUE CpGs `tabix -R` returns from the CpG dictionary for columns 1-3 of the bed: tabix reads such a file as
              0-based half-open, so the CpG at 1-based position p is taken when start < p <= end (NOT `convert -L`'s join).  The
              sets are built per chromosome with numpy.searchsorted over the genome's loci, merged into ascending disjoint
              ranges, and handed to the kernel with the whole files resident.
    table     what print(df.T) prints under display.max_columns = display.max_rows = None and display.width = --width:
              table_text below (pandas is not needed)

Deliberate deviations from the reference: `tabix` is not run (see -L); -@ is accepted and ignored (no process pool).
No CPU fallback.
"""
import argparse
from fractions import Fraction

import numpy as np

from .beta_cov import beta_width, file_stats, pretty_name
from .cliutil import add_threads_option, add_where_options
from .genome import GenomicRegion, IllegalArgumentError, beta_sanity_check

ROW_NAMES = ('mean meth. (%)', 'covered sites', 'covered sites (10+)', 'max depth', 'mean depth')
RATIO_UNIT_BITS = 62
MAX_COLWIDTH = 50                 # pandas' display.max_colwidth: a longer cell (an index entry too) is cut and ends in '...'


def mean_meth_text(ratio, covered, orphans):
    """str(np.nanmean(meth / cov * 100).round(2)) from the exact sum `ratio` (Python int, units of 2^-62)"""
    if orphans > 0:
        return 'inf'
    if covered == 0:
        return 'nan'
    total = float(Fraction(ratio, 1 << RATIO_UNIT_BITS))          # the correctly rounded double of the exact sum
    return str(np.float64(total / covered).round(2))


def stat_strings(s):
    """the five values of print_stats (beta_stats.py:35-51) from one sample's integers"""
    ratio = (s['ratio_hi'] << 64) | s['ratio_lo']
    return [mean_meth_text(ratio, s['covered'], s['orphans']),
            f"{s['covered']:,}",
            f"{s['covered_at']:,}",
            f"{s['max_cov']:,}",
            f"{np.float64(s['cov_sum'] / s['n_sites']).round(2):,}"]


def _cut(text):
    return text if len(text) <= MAX_COLWIDTH else text[:MAX_COLWIDTH - 3] + '...'


def table_text(names, values, width=120, header='names', columns=ROW_NAMES):
    """The text of print(df.T) for a frame of strings: one row per sample.  An index column (left-aligned, headed by the
    columns' name), right-aligned value columns one space apart; when index + columns exceed `width` the columns continue in
    further blocks, separated by an empty line, every block but the last ending its header line in ' \\'."""
    if not names:
        return 'Empty DataFrame\nColumns: [%s]\nIndex: []' % ', '.join(columns)
    idx = [header] + [_cut(str(n)) for n in names]
    iw = max(len(x) for x in idx)
    idx = [x.ljust(iw) for x in idx]
    cols = []
    for j, c in enumerate(columns):
        cells = [c] + [_cut(v[j]) for v in values]
        w = max(len(x) for x in cells)
        cols.append([x.rjust(w) for x in cells])
    room = width - (iw + 1)
    bins, cur = [], 0
    for i, col in enumerate(cols):                              # pandas' _binify: a column that would pass the width opens a block
        w = len(col[0]) + 1
        cur += w
        if i > 0 and cur + (1 if i == len(cols) - 1 else 2) > room:
            bins.append(i)
            cur = w
    bins.append(len(cols))
    blocks, start = [], 0
    for b, end in enumerate(bins):
        block = [idx] + cols[start:end]
        if len(bins) > 1:
            block.append([' \\'] + ['  '] * len(names) if b < len(bins) - 1 else [' '] * (len(names) + 1))
        blocks.append('\n'.join(' '.join(col[r] for col in block) for r in range(len(names) + 1)))
        start = end
    return '\n\n'.join(blocks)


def merge_ranges(starts, ends):
    """half-open [start, end) pairs in any order, overlapping, touching, repeated or empty -> [n, 2] int64 array of ascending,
    disjoint, non-empty ranges with the same union (touching ones joined)"""
    s = np.asarray(starts, dtype=np.int64)
    e = np.asarray(ends, dtype=np.int64)
    keep = e > s
    s, e = s[keep], e[keep]
    if not s.size:
        return np.zeros((0, 2), dtype=np.int64)
    order = np.argsort(s, kind='stable')
    s, e = s[order], e[order]
    reach = np.maximum.accumulate(e)
    first = np.concatenate([[True], s[1:] > reach[:-1]])           # a range that begins behind everything before it
    last = np.concatenate([first[1:], [True]])
    return np.stack([s[first], reach[last]], axis=1)


def bed_rows(bed_path):
    """(chrom, start, end) of a bed file's first three columns; '#' lines and empty lines are skipped"""
    import gzip
    opener = gzip.open if bed_path.endswith('.gz') else open
    rows = []
    try:
        with opener(bed_path, 'rt') as f:
            for line in f:
                if not line.strip() or line.startswith('#'):
                    continue
                tok = line.rstrip('\n').split('\t')
                try:
                    rows.append((tok[0], int(tok[1]), int(tok[2])))
                except (IndexError, ValueError):
                    raise IllegalArgumentError(f'Invalid bed file: {bed_path}\nline: {line.strip()[:80]}')
    except OSError:
        raise IllegalArgumentError(f'Invalid file: {bed_path}')
    return rows


def sites_of_regions(genome, rows):
    """0-based site ranges (merged) of the CpGs `tabix -R` selects for the bed rows (chrom, start, end): 1-based position p with
    start < p <= end; a chromosome the genome does not have selects nothing"""
    names, sizes = genome.get_chrom_cpg_sizes()
    first = dict(zip(names, (np.cumsum(sizes) - sizes).tolist()))
    size = dict(zip(names, sizes.tolist()))
    loci = genome.loci()
    by_chrom = {}
    for c, a, b in rows:
        if c in first:
            by_chrom.setdefault(c, []).append((a, b))
    starts, ends = [], []
    for c, ab in by_chrom.items():
        ab = np.asarray(ab, dtype=np.int64)
        pos = loci[first[c]:first[c] + size[c]]
        starts.append(first[c] + np.searchsorted(pos, ab[:, 0], 'right'))
        ends.append(first[c] + np.searchsorted(pos, ab[:, 1], 'right'))
    if not starts:
        return np.zeros((0, 2), dtype=np.int64)
    return merge_ranges(np.concatenate(starts), np.concatenate(ends))


def beta_stats(betas, gr=None, bed_path=None, device=0):
    """[(name, the five strings)] of the files, in argument order"""
    for b in betas:
        beta_width(b)
    ranges_of = None
    if bed_path:
        ranges = sites_of_regions(gr.genome, bed_rows(bed_path))

        def ranges_of(n_sites):
            r = ranges[ranges[:, 0] < n_sites].copy()              # (a file shorter than the genome: what indexing it would reach)
            if len(r) and r[-1, 1] > n_sites:
                raise IllegalArgumentError(f'the bed file selects site {int(r[-1, 1])}, the beta files have {n_sites:,} sites')
            return r
    else:
        for b in betas:
            beta_sanity_check(b, gr.genome)
    stats = file_stats(betas, None if bed_path else gr.sites, ranges_of, 10, device)
    for b, s in zip(betas, stats):
        if s['n_sites'] == 0:
            raise AssertionError(b + ': Data table is empty!')
    return [(pretty_name(b), stat_strings(s)) for b, s in zip(betas, stats)]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('betas', nargs='+', help='one or more beta files')
    parser.add_argument('--width', '-w', type=int, default=120, help='max width to print output table [120]')
    add_where_options(parser, bed_file=True)
    add_threads_option(parser)
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Print global stats of one or more beta/lbeta file(s)
    """
    args = parse_args(argv)
    gr = GenomicRegion(args)
    res = beta_stats(args.betas, gr, args.bed_file, args.device)
    print(table_text([n for n, _ in res], [v for _, v in res], args.width))


if __name__ == '__main__':
    main()
