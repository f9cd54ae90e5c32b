"""`wgbstools compare_betas` on MI355X: a 2-D histogram of methylation for every pair of beta files — do the samples agree, are
the replicates concordant, is one of them an outlier.

Drop-in for the reference's src/python/compare_betas.py (same flags, same figure), written against its contract:

    input     `.beta` / `.bin` (uint8 pairs) and `.lbeta` (uint16 pairs) files, as load_beta_data takes them; with -s / -r only
              that slice of every file is read and uploaded.  There is no -L.
    pairs     all (i, j) with j <= i, the diagonal included; x is file j, y is file i (comp2(tables[i], tables[j]))
    mask      the sites where min(cov_i, cov_j) >= --min_cov
    values    meth / cov in float64, one division (numpy's uint8 / uint8); nothing checks meth <= cov
    cells     np.histogram2d(x, y, bins) with no range given: per pair and axis the edges are np.linspace(lo, hi, bins + 1)
              over the masked values' own min and max — (0, 1) when nothing is masked in, (lo - 0.5, hi + 0.5) when lo == hi —
              and the cell of a value is searchsorted(edges, v, 'right') - 1, the last edge falling in the last cell
    figure    an N x N grid, lower triangle: pcolormesh(xedges, yedges, counts.T, cmap=jet, norm=LogNorm()), both axes 0 .. 1,
              the files' names cut into 20-character lines as labels, the unused axes deleted

The range depends on the pair, so the rows are passed over twice: k_pair_ranges gives every pair's site count and the min and
max of both ratios (exact: they travel as bit patterns), the edges are built HERE with np.linspace — its own doubles — and
k_pair_hist counts against them (csrc/pair_kernels.h; wgbsseg_pair_ranges, wgbsseg_pair_hist).  All files are resident in one
context and all pairs go through one call each way.  No CPU fallback.

Deliberate deviations from the reference:
  1. -o PATH.npz writes the arrays instead of a figure — names, pairs [n_pairs, 2] = (i, j), counts [n_pairs, bins, bins]
     (uint64, [x_cell, y_cell]), xedges and yedges [n_pairs, bins + 1] — and needs no matplotlib.
  2. --min_cov below 1 is refused (the reference fails inside numpy there: a site without coverage has no ratio), and so are
     more --bins than one workgroup's LDS holds (_lib.pair_hist_limits).
  3. `.beta` and `.lbeta` files may be mixed in one call (the reference wants one suffix): the narrow ones are widened.
  4. --device chooses the GPU.
"""
import argparse

import numpy as np

from .beta_cov import beta_width, load_rows, pretty_name
from .cliutil import add_where_options
from .genome import GenomicRegion, IllegalArgumentError, eprint


def all_pairs(n):
    """the reference's pairs, in the order it draws them: (i, j) with j <= i -> int32 [n (n + 1) / 2, 2]"""
    return np.array([(i, j) for i in range(n) for j in range(i + 1)], dtype=np.int32).reshape(-1, 2)


def edges_of(n, lo, hi, bins):
    """np.histogram2d's edges of one axis from the masked values' count, min and max"""
    if n == 0:
        lo, hi = 0.0, 1.0
    elif lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, bins + 1)


def pair_histograms(betas, min_cov=10, bins=101, sites=None, device=0, timings=None):
    """-> (pairs [n_pairs, 2] = (i, j), counts [n_pairs, bins, bins] uint64, xedges [n_pairs, bins + 1], yedges [n_pairs, bins + 1]):
    for every pair what np.histogram2d(ratio_j, ratio_i, bins) returns over the sites both files cover.  `sites`: 1-based
    [start, end) slice read from every file."""
    if min_cov < 1:
        raise IllegalArgumentError(f'--min_cov must be at least 1 (got {min_cov}): a site without coverage has no ratio')
    if bins < 1:
        raise IllegalArgumentError(f'--bins must be at least 1 (got {bins})')
    wide = [beta_width(b) == 2 for b in betas]
    rows = [load_rows(b, sites) for b in betas]
    for b, r in zip(betas, rows):
        if r.size != rows[0].size:
            raise IllegalArgumentError(f'{b} holds {r.size // 2} sites, {betas[0]} holds {rows[0].size // 2}: compare_betas needs files of one length')
    from . import _lib
    pairs = all_pairs(len(betas))
    with _lib.Segmenter(device) as seg:
        if any(wide):
            seg.set_lbetas([r if w else r.astype(np.uint16) for r, w in zip(rows, wide)])      # a mix: widened on the host
        else:
            seg.set_betas(rows)
        try:
            got = seg.pair_ranges(pairs, min_cov)
            if timings is not None:
                timings.append(seg.last_block_sums_ms())
            xedges = np.stack([edges_of(g['n'], float(g['b_min']), float(g['b_max']), bins) for g in got])
            yedges = np.stack([edges_of(g['n'], float(g['a_min']), float(g['a_max']), bins) for g in got])
            counts = seg.pair_hist(pairs, min_cov, bins, np.stack([xedges, yedges], axis=1))
            if timings is not None:
                timings.append(seg.last_block_sums_ms())
        except _lib.SegmentorError as e:
            if e.code == _lib.E_ARG:
                raise IllegalArgumentError(e.msg)
            raise
    return pairs, counts, xedges, yedges


def label_of(name, k=20):
    """a file's name cut into lines of k characters"""
    return '\n'.join(name[i:i + k] for i in range(0, len(name), k))


def draw(pairs, counts, xedges, yedges, names):
    """The reference's figure from the histograms: a len(names) x len(names) grid with pair (i, j) at row i, column j.
    -> the matplotlib figure.  Needs no GPU; matplotlib is imported here and nowhere else."""
    try:
        import matplotlib.pyplot as plt
        from matplotlib.colors import LogNorm
    except ImportError as e:
        raise IllegalArgumentError(f'the figure needs matplotlib, which cannot be imported ({e}): write the arrays with -o PATH.npz instead')
    N = len(names)
    labels = [label_of(n) for n in names]
    fig, axs = plt.subplots(N, N, squeeze=False)
    drawn = set()
    for (i, j), c, xe, ye in zip(pairs, counts, xedges, yedges):
        ax = axs[i, j]
        ax.pcolormesh(xe, ye, np.asarray(c, dtype=np.float64).T, cmap=plt.cm.jet, norm=LogNorm())
        ax.set_ylim(0, 1)
        ax.set_xlim(0, 1)
        drawn.add((int(i), int(j)))
    for i in range(N):
        axs[i, 0].set_ylabel(labels[i], fontsize=8)
        axs[N - 1, i].set_xlabel(labels[i], fontsize=8)
    for i in range(N):
        for j in range(N):
            if (i, j) not in drawn:
                fig.delaxes(axs[i, j])
    for ax in axs.flat:
        ax.label_outer()
    fig.tight_layout()
    return fig


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('betas', nargs='+')
    parser.add_argument('--outpath', '-o', help='Dump figure to this path (e.g., pdf/png), or the histograms to a .npz. '
                                                'If not specified, --show flag is set')
    parser.add_argument('--show', action='store_true', help='Display the figures using matplotlib.pyplot.show.')
    parser.add_argument('--min_cov', '-c', type=int, default=10,
                        help='Minimal coverage to consider. Sites with coverage lower than this value are ignored')
    parser.add_argument('--bins', type=int, default=101, help='Histogram bins (resolution) [101]')
    add_where_options(parser)
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Compare between pairs of beta files, by plotting a 2d histogram
    for every pair.
    Drop sites with low coverage (< cov_thresh argument),
    for performance and robustness.
    """
    args = parse_args(argv)
    if len(args.betas) < 2:
        raise IllegalArgumentError('Input error: at least 2 input files must be given')
    for b in args.betas:
        beta_width(b)
    where = args.sites or args.region or args.array_id
    sites = GenomicRegion(args).sites if where else None          # (whole files need no genome directory)
    pairs, counts, xedges, yedges = pair_histograms(args.betas, args.min_cov, args.bins, sites, args.device)
    names = [pretty_name(b) for b in args.betas]
    if args.outpath is not None and args.outpath.endswith('.npz'):
        np.savez(args.outpath, names=np.array(names), pairs=pairs, counts=counts, xedges=xedges, yedges=yedges)
        eprint(f'[wt cmp] dumped histograms to {args.outpath}')
        return
    draw(pairs, counts, xedges, yedges, names)
    import matplotlib.pyplot as plt
    if args.outpath is not None:
        plt.savefig(args.outpath)
        eprint(f'[wt cmp] dumped figure to {args.outpath}')
    if args.show or args.outpath is None:
        plt.show()


if __name__ == '__main__':
    main()
