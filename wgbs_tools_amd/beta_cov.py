"""`wgbstools beta_cov` on MI355X: the mean coverage of one or more beta files — the first thing asked of a cohort before any
sample goes into `segment`.

Drop-in for the reference's src/python/beta_cov.py (same flags, same output lines), written against its contract:

    input     `.beta` / `.bin` (uint8 pairs) and `.lbeta` (uint16 pairs) files, as load_beta_data takes them (utils_wgbs.py:307-330);
              with -s / -r / --array_id only that slice of every file is read (a seek, as the reference) and uploaded
    result    the mean of the cov column (beta_cov.py:66): cov_sum / n_sites, Python float division of two exact integers —
              what numpy's float64 mean of a uint8 / uint16 column is, its sum being exact below 2^53
    -L BED    the reference's rule (beta_cov_by_bed, beta_cov.py:52-59): the 5-column blocks file read with load_blocks_file,
              the blocks' raw cov sums, and sum(cov) / sum(endCpG - startCpG); NA rows add nothing to either sum, overlapping
              blocks count as often as they occur, 0 when the blocks hold no site.  This path needs no new kernel: it is the
              existing block reduction (BlockSumEngine mode 0, wgbsseg_block_sums) summed on the host.
    output    one line per file in argument order: '{name}\\t{cov:.2f}', name = the basename without its last extension

All files of one invocation are resident in ONE context and reduced in one launch of k_sample_stats (csrc/stats_kernels.h,
wgbsseg_sample_stats) — in pieces when they would not fit (PIECE_BYTES) or differ in width or length — instead of one numpy
pass per file in a process pool.  No CPU fallback.

Deliberate deviations from the reference:
  1. --plot and --hist (matplotlib / plotille figures) are accepted and refused, naming the reference command to use.
  2. -@ is accepted and ignored: there is no process pool.
"""
import argparse
import os.path as op

import numpy as np

from .cliutil import add_threads_option, add_where_options
from .genome import GenomicRegion, IllegalArgumentError

PIECE_BYTES = 64 << 30            # rows resident at once: more files than this are reduced piece by piece


def pretty_name(beta_path):
    return op.splitext(op.basename(beta_path))[0]


def beta_width(beta_path):
    """bytes per count of a beta file, after load_beta_data's check of the path (utils_wgbs.py:310-319)"""
    suff = op.splitext(beta_path)[1]
    if not (op.isfile(beta_path) and suff in ('.beta', '.lbeta', '.bin')):
        raise IllegalArgumentError(f'Invalid beta file:\n{beta_path}')
    return 2 if suff == '.lbeta' else 1


def load_rows(beta_path, sites=None):
    """the (meth, cov) rows of a beta file as a flat array of uint8 / uint16 (a read-only map of the whole file; with `sites` =
    1-based [start, end) only that slice, read after a seek); the reference's failure when nothing is selected"""
    elem = beta_width(beta_path)
    dtype = np.uint16 if elem == 2 else np.uint8
    if sites is None:
        n = op.getsize(beta_path) // (2 * elem) * 2
        data = np.memmap(beta_path, dtype=dtype, mode='r', shape=(n,)) if n else np.zeros(0, dtype=dtype)
    else:
        start, end = sites
        data = np.fromfile(beta_path, dtype=dtype, count=(end - start) * 2, offset=(start - 1) * 2 * elem)
        data = data[:data.size // 2 * 2]
    if not data.size:
        raise AssertionError(beta_path + ': Data table is empty!')
    return data


def pieces_of(betas, row_bytes):
    """the files' indexes cut into runs that can be resident together: equal width, equal length, at most PIECE_BYTES"""
    out, cur, size = [], [], 0
    for i, b in enumerate(betas):
        key = (beta_width(b), row_bytes[i])
        if cur and (key != (beta_width(betas[cur[0]]), row_bytes[cur[0]]) or size + row_bytes[i] > PIECE_BYTES):
            out.append(cur)
            cur, size = [], 0
        cur.append(i)
        size += row_bytes[i]
    if cur:
        out.append(cur)
    return out


def file_stats(betas, sites=None, ranges_of=None, depth_at=10, device=0, timings=None):
    """wgbsseg_sample_stats of every file, in argument order -> list of dicts of Python ints.  `sites`: 1-based [start, end) slice
    read from every file; `ranges_of(n_sites)`: the 0-based ranges to reduce over (default: everything resident)."""
    from . import _lib
    rows = [load_rows(b, sites) for b in betas]
    stats = [None] * len(betas)
    with _lib.Segmenter(device) as seg:
        for piece in pieces_of(betas, [r.nbytes for r in rows]):
            wide = beta_width(betas[piece[0]]) == 2
            (seg.set_lbetas if wide else seg.set_betas)([rows[i] for i in piece])
            ranges = [(0, seg.n_sites)] if ranges_of is None else ranges_of(seg.n_sites)
            try:
                got = seg.sample_stats(ranges, depth_at)
            except _lib.SegmentorError as e:
                raise IllegalArgumentError(f'{betas[piece[0]]}: {e.msg}')
            if timings is not None:
                timings.append(seg.last_block_sums_ms())
            for i, g in zip(piece, got):
                stats[i] = {k: int(g[k]) for k in g.dtype.names}
    return stats


def beta_cov_by_bed(betas, blocks, device=0):
    """beta_cov.py:52-59 for every file: sum of the blocks' cov sums / sum of their lengths (0 when they hold no site)"""
    from . import _lib
    from .beta_to_blocks import BlockSumEngine
    ok = ~blocks.na
    nr_sites_covered = int((blocks.endCpG[ok] - blocks.startCpG[ok]).sum())
    if not nr_sites_covered:
        return [0] * len(betas)
    covs = [None] * len(betas)
    sizes = [op.getsize(b) if op.isfile(b) else 0 for b in betas]
    for piece in pieces_of(betas, sizes):
        eng = BlockSumEngine([betas[i] for i in piece], device=device)
        try:
            sums = eng.reduce(blocks, mode=0)
        except _lib.SegmentorError as e:
            raise IllegalArgumentError(f'{betas[piece[0]]}: {e.msg}')
        finally:
            eng.close()
        for k, i in enumerate(piece):
            covs[i] = int(sums[k, :, 1].astype(np.int64).sum()) / nr_sites_covered
    return covs


def beta_cov(betas, sites=None, blocks=None, device=0):
    """the mean coverage of every file, in argument order"""
    if blocks is not None:
        return beta_cov_by_bed(betas, blocks, device)
    return [s['cov_sum'] / s['n_sites'] for s in file_stats(betas, sites, device=device)]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('betas', nargs='+', help='one or more beta files')
    parser.add_argument('--plot', action='store_true', help='Plot histogram of coverages')
    parser.add_argument('--hist', action='store_true', help='Plot in-terminal histogram of coverages')
    add_where_options(parser, bed_file=True)
    add_threads_option(parser)
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Calculate the average coverage of one or more beta files.
    Print the results.
    """
    args = parse_args(argv)
    for flag in ('plot', 'hist'):
        if getattr(args, flag):
            raise IllegalArgumentError(f'--{flag} draws a figure and is not part of this build: use the reference\'s `wgbstools beta_cov --{flag}`')
    sites = GenomicRegion(args).sites
    blocks = None
    if args.bed_file:
        from .beta_to_blocks import load_blocks_file
        blocks = load_blocks_file(args.bed_file)
    for b in args.betas:
        beta_width(b)
    covs = beta_cov(args.betas, sites, blocks, args.device)
    for cov, beta_path in zip(covs, args.betas):
        print('{}\t{:.2f}'.format(pretty_name(beta_path), cov))


if __name__ == '__main__':
    main()
