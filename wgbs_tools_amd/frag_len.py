"""`wgbstools frag_len` on MI355X: the histogram of the read lengths (in CpGs) of a pat file, every read weighted by its count —
the pat-side QC step, and what `homog -l` is chosen from: it must fit the fragment lengths of the library.

Drop-in for the reference's src/python/frag_len.py (same flags, messages and output), written against its contract
(frag_len.py:21-46, cview.py:25-101, src/cview/cview.cpp:87-128):

    histogram with m = --max_frag_size, a selected line `chr, startCpG, pattern, count` adds count to bin min(len(pattern), m); the
              result is the m sums of the lengths 1..m (exact int64 sums)
    selection whole genome (no -s / -r / -L): every line.  -s / -r: the reads cview passes without --strict for the one block
              [s, e) of the region's CpGs.  -L: the same for the blocks in columns 4-5 of the file, NA rows and a header skipped,
              ordered as cview orders them: `sort -k1,1n` in the C locale of the text "startCpG\\tendCpG" — by startCpG as a number,
              equal starts by the bytes of that text ("50\\t100" before "50\\t60").
    block rule on reads sorted by start: a read covering [rs, rs + len) is dropped when rs >= endCpG of the block that sorts LAST
              (also where an earlier, longer block still holds it: the reference stops reading there); else, with cur the first
              block in that order whose endCpG > rs, the read counts — whole, unclipped — iff rs + len - 1 >= startCpG[cur].
              k_frag_hist (csrc/frag_kernels.h) says why this test on the read alone equals the reference's walk.
    output    per file in argument order: the path on stderr; `[wt frag] Empty list of lengths for {pat}` when nothing was
              counted; -v: the m integers on one line, separated by spaces; --outdir: <outdir>/<name>.png, --display: plt.show()

The reference pipes `tabix` (per chromosome) or its cview into awk; here the file's text — inflated on the host or, with
`--inflate device`, on the GPU — goes through the feed the other pat commands share, and one kernel counts it
(wgbsseg_fraglen_*, include/wgbsseg.h).  No CPU fallback.

Deliberate deviations from the reference:
  1. No `.csi` index is required: the whole file is read.  The reference asks tabix for a window in front of the region (150
     sites for -r / -s, 100 for the blocks of -L) and so misses a read that starts earlier and still reaches the region; here
     such a read counts, as it does on the reference's own `gunzip -c` branch (cview.py:88-89).
  2. Whole genome: lines on chromosomes outside the genome's list count too (the reference asks tabix per listed chromosome).
  3. What the reference mangles silently is refused, naming the byte offset or the row: a malformed pat line (fewer than four
     fields, a site or count that is not a number, or an EMPTY pattern, whose count the reference's awk would take for the
     pattern); with a selection, a read that starts before the read before it (no such check for the whole genome, where the
     order does not matter); a block with endCpG <= startCpG or startCpG < 1, a block list without a usable row;
     --max_frag_size below 1 or above MAX_FRAG_SIZE.

The figure is drawn with matplotlib, imported only when --outdir or --display asks for one; -v needs none.
"""
import argparse
import os
import os.path as op
import sys

import numpy as np

from .cliutil import add_where_options
from .genome import GenomicRegion, IllegalArgumentError, eprint
from .homog import check_pats
from .pat2beta import add_inflate_option, feed_pat, splitextgz

MAX_FRAG_SIZE = 1 << 20           # csrc/frag_plan.h WG_FRAG_MAX_BINS


def cview_order(blocks, path='the blocks file'):
    """(startCpG, endCpG) int64 arrays of the usable rows of a blocks table in the order cview takes them (see the module's
    docstring); deviation 3 for the rows it would stop at, and for a table without a usable row."""
    use = np.flatnonzero(~blocks.na)
    if use.size == 0:
        raise IllegalArgumentError(f'Invalid blocks file: {path}: no row with startCpG and endCpG')
    s, e = blocks.startCpG[use], blocks.endCpG[use]
    wrong = np.flatnonzero((e <= s) | (s < 1))
    if wrong.size:
        r = int(wrong[0])
        what = f'startCpG {int(s[r])} < 1' if s[r] < 1 else f'endCpG {int(e[r])} <= startCpG {int(s[r])}'
        raise IllegalArgumentError(f'Invalid blocks file: {path}: row {int(use[r]) + 1} has {what}')
    order = np.argsort(s, kind='stable')
    ss = s[order]
    tied = np.zeros(ss.size, dtype=bool)
    if ss.size > 1:
        same = ss[1:] == ss[:-1]
        tied[1:] |= same
        tied[:-1] |= same
    pos = np.flatnonzero(tied)
    if pos.size:                                                  # equal starts: by the bytes of the file's own "startCpG\tendCpG"
        rows = use[order[pos]]
        if blocks.parsed is not None:
            a, z = blocks.parsed.cpg_text(rows)
        else:
            a, z = blocks.cpg_text()
            a, z = [a[i] for i in rows.tolist()], [z[i] for i in rows.tolist()]
        key = [(int(v), (x + '\t' + y).encode()) for v, x, y in zip(ss[pos].tolist(), a, z)]
        fixed = sorted(range(pos.size), key=key.__getitem__)
        order[pos] = order[pos][fixed]
    return np.ascontiguousarray(s[order]), np.ascontiguousarray(e[order])


def selection(args):
    """-> (starts, ends) of the blocks that select reads, in cview's order; (None, None) for the whole genome"""
    if args.bed_file:
        from .beta_to_blocks import load_blocks_file
        return cview_order(load_blocks_file(args.bed_file), args.bed_file)
    if args.sites or args.region or getattr(args, 'array_id', None):
        s, e = GenomicRegion(args).sites
        return np.array([s], dtype=np.int64), np.array([e], dtype=np.int64)
    return None, None


def frag_hist(pat, max_frag, starts=None, ends=None, device=0, inflate='host', timings=None):
    """int64 hist[max_frag] of one pat file: wgbsseg_fraglen over its text"""
    from . import _lib
    t = timings if timings is not None else {}
    try:
        with _lib.FragLen(max_frag, starts, ends, device=device) as h:
            feed_pat(h, pat, t, inflate=inflate)
            hist = h.finish()
            t['kernel_ms'] = h.kernel_ms()
    except _lib.SegmentorError as e:
        raise IllegalArgumentError(f'{pat}: {e.msg}')
    return hist


def fig_path(pat, outdir):
    return op.join(outdir, op.basename(splitextgz(pat)[0])) + '.png'


def plot_hist(hist, max_frag, pat):
    """a line plot of the lengths 1..m: major ticks every 5, a minor grid, the title with the file's name below it.  -> pyplot"""
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise IllegalArgumentError(f'the figure needs matplotlib, which cannot be imported ({e}): -v prints the values and needs no figure')
    fig, ax = plt.subplots()
    ax.plot(np.arange(1, hist.size + 1), hist)
    ax.set_xticks(np.arange(1, max_frag, 5))
    ax.set_xticks(np.arange(1, max_frag), minor=True)
    ax.grid(which='minor', alpha=0.2)
    ax.grid(which='major', alpha=0.5)
    ax.set_ylim(bottom=0)
    ax.set_xlim(left=1)
    ax.set_title('Fragment lengths (CpGs)\n' + op.basename(splitextgz(pat)[0]))
    return plt


def run_single_pat(pat, args, starts, ends):
    eprint(pat)
    hist = frag_hist(pat, args.max_frag_size, starts, ends, args.device, args.inflate)
    if not hist.any():
        eprint(f'[wt frag] Empty list of lengths for {pat}')
        return None
    if args.verbose:
        print(' '.join(str(v) for v in hist.tolist()))
        sys.stdout.flush()
    plt = None
    if args.outdir or args.display:
        if args.verbose:
            eprint('[wt frag] plotting...')
        plt = plot_hist(hist, args.max_frag_size, pat)
    if args.outdir:
        fpath = fig_path(pat, args.outdir)
        if args.verbose:
            eprint(f'[wt frag] dumping {fpath}...')
        plt.savefig(fpath)
    return plt


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('pat_paths', nargs='+')
    parser.add_argument('-v', '--verbose', action='store_true', help='print the histogram values to stdout')
    parser.add_argument('-m', '--max_frag_size', type=int, default=30,
                        help='Maximum fragment size. Longer fragments will be trimmed. [30]')
    parser.add_argument('--outdir', '-o', help='output directory for the histogram figure(s) [None]')
    parser.add_argument('--display', action='store_true', help='Display histogram plot(s) (plt.show)')
    add_where_options(parser, bed_file=True)
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    return parser.parse_args(argv)


def main(argv=None):
    """
    Plot histogram of reads lengths (in sites) of pat file
    Output to stdout the histogram values if requested
    """
    args = parse_args(argv)
    check_pats(args.pat_paths)
    if not 1 <= args.max_frag_size <= MAX_FRAG_SIZE:
        raise IllegalArgumentError(f'--max_frag_size must be in [1, {MAX_FRAG_SIZE}] (got {args.max_frag_size})')
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
    starts, ends = selection(args)
    plt = None
    for pat in args.pat_paths:
        plt = run_single_pat(pat, args, starts, ends) or plt
    if args.display and plt is not None:
        plt.show()


if __name__ == '__main__':
    main()
