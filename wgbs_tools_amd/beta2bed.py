"""`wgbstools beta2bed` on MI355X: a .beta / .lbeta file as BED text, a line per CpG — `chr start end meth cov`, or
`chr start end ratio` with --mean — the form other genome tools read.

Drop-in for the reference's src/python/beta2bed.py (same flags, same text), written against its contract (beta2bed.py:11-31,
view.py:35-51, src/view_beta.sh, src/view_lbeta.sh: `gunzip | awk | paste | hexdump`, then up to three awk filters):

    text      every byte is made on the device by ONE library call (wgbsseg_beta2bed: csrc/bed_kernels.h): the file's rows and the
              genome's loci are resident, a length pass and a scan place every line, a second pass formats the lines in LDS and
              stores them; the host only hands finished slabs of text to the output while the next slab is computed.
    base line chrom \\t loc-1 \\t loc+1 \\t meth \\t cov, loc = the CpG's position (column 2 of CpG.bed.gz); uint8 counts of a .beta,
              uint16 counts of an .lbeta; any other suffix is refused as view.py:43 refuses it
    -c N      N > 1: a site with cov < N becomes `0 0`, with or without --mean (what the code does; the help text says otherwise)
    --keep_na not given: sites whose cov is 0 (after -c) are dropped
    --mean    the last two columns become awk's printf "%.3g" of the double meth / cov (csrc/bed_fmt.h reproduces C's rounding
              from the two integers, ties included); -1 where cov is 0
    -s / -r   that range of sites (through GenomicRegion); the file stays resident as a whole
    -L BED    THIS BUILD'S DEFINITION of the reference's `bedtools intersect -a stdin -b BED -wa` over the whole genome's base
              lines: a site's line is written once FOR EVERY row of the bed file on its chromosome with start <= loc <= end
              (the overlap of [loc-1, loc+1) with [start, end)); sites keep their order, the copies of a line are adjacent; a row
              on a chromosome the genome lacks selects nothing.  The number of rows over every site is counted on the host
              (numpy.searchsorted of each row's start and end in its chromosome's loci, a difference array, a cumulative sum)
              and handed to the device as one uint16 per site over the smallest range that holds a nonzero one.  `bedtools` is
              not run.
    -o PATH   default: standard output.  A path ending in .gz is compressed in this process (zlib, through gzip.GzipFile); no
              program is started.  -f / the skip message: delete_or_skip.  A reader that goes away ends the command quietly.
    --deflate device   (with -o PATH.gz only) the text never leaves the device: wgbsseg_beta2bed_bgzf deflates every slab into BGZF
              members there (csrc/deflate_kernels.h) and writes them straight to the file, the end-of-file member last; no pipe, no
              thread.  The file is BGZF, so `gzip -d` reads it as before and `tabix` can index it.  The default, host, is the line above.

Deliberate deviations from the reference: a beta file whose length differs from the genome's is refused after the reference's
warning (its `paste` would print ragged lines); `bedtools`, `tabix`, `hexdump`, `awk` and `gzip` are not run.  No CPU fallback.
"""
import argparse
import gzip
import os
import sys
import threading

import numpy as np

from .beta_cov import load_rows
from .beta_stats import bed_rows
from .cliutil import add_where_options, require_file
from .convert import delete_or_skip
from .genome import GenomicRegion, IllegalArgumentError, beta_sanity_check

MULT_TOO_MANY = 65535              # include/wgbsseg.h: the reserved multiplicity


def beta_elem(beta_path):
    """bytes per count, or view.py:43's refusal"""
    if beta_path.endswith('.beta'):
        return 1
    if beta_path.endswith('.lbeta'):
        return 2
    raise IllegalArgumentError(f'Invalid input format for view beta: {beta_path}')


def multiplicities(genome, rows):
    """How many of the bed rows (chrom, start, end) hold each site — start <= loc <= end on the row's chromosome — as
    (first site, uint16 counts of the sites first .. first + len) over the smallest range with a nonzero count; (0, empty) when no
    site is held.  More than 65534 rows over one site are refused."""
    names, sizes = genome.get_chrom_cpg_sizes()
    first = dict(zip(names, (np.cumsum(sizes) - sizes).tolist()))
    size = dict(zip(names, np.asarray(sizes).tolist()))
    loci = genome.loci()
    by_chrom = {}
    for c, a, b in rows:
        if c in first:
            by_chrom.setdefault(c, []).append((a, b))
    lo_all, hi_all = [], []
    for c, ab in by_chrom.items():
        ab = np.asarray(ab, dtype=np.int64)
        pos = loci[first[c]:first[c] + size[c]]
        lo = first[c] + np.searchsorted(pos, ab[:, 0], 'left')
        hi = first[c] + np.searchsorted(pos, ab[:, 1], 'right')
        keep = hi > lo
        lo_all.append(lo[keep])
        hi_all.append(hi[keep])
    lo = np.concatenate(lo_all) if lo_all else np.zeros(0, dtype=np.int64)
    hi = np.concatenate(hi_all) if hi_all else np.zeros(0, dtype=np.int64)
    if not lo.size:
        return 0, np.zeros(0, dtype=np.uint16)
    a, b = int(lo.min()), int(hi.max())
    diff = np.zeros(b - a + 1, dtype=np.int64)
    np.add.at(diff, lo - a, 1)
    np.add.at(diff, hi - a, -1)
    mult = np.cumsum(diff[:-1])
    if mult.max() >= MULT_TOO_MANY:
        at = int(np.argmax(mult))
        raise IllegalArgumentError(f'the bed file has {int(mult[at]):,} rows over CpG {a + at + 1}: at most {MULT_TOO_MANY - 1:,} are supported')
    return a, mult.astype(np.uint16)


class _GzipSink:
    """A file descriptor whose bytes end up gzip-compressed in `path`: the write end of a pipe, a thread compressing the other end."""

    def __init__(self, path):
        self._r, self.fd = os.pipe()
        self._out = gzip.GzipFile(path, 'wb')
        self._error = None
        self._thread = threading.Thread(target=self._pump, daemon=True)
        self._thread.start()

    def _pump(self):
        try:
            while True:
                piece = os.read(self._r, 1 << 20)
                if not piece:
                    break
                self._out.write(piece)
        except Exception as e:                                     # (kept for close(): the writer sees a broken pipe meanwhile)
            self._error = e
        finally:
            os.close(self._r)

    def close(self):
        os.close(self.fd)
        self._thread.join()
        self._out.close()
        if self._error:
            raise self._error


def check_deflate(deflate, opath):
    """--deflate device needs a .gz path to write BGZF to"""
    if deflate not in ('host', 'device'):
        raise IllegalArgumentError(f"deflate must be 'host' or 'device', not {deflate!r}")
    if deflate == 'device' and (opath is None or opath == '/dev/stdout' or not opath.endswith('.gz')):
        raise IllegalArgumentError('--deflate device compresses the output on the GPU: give -o a path that ends in .gz')


def write_bed(seg, fd, gr, bed_path, min_cov=1, mean=False, keep_na=False, sample=0, slab_sites=0, bgzf=False):
    """the selected lines of resident sample `sample` to the descriptor -> (lines, bytes); bgzf: as BGZF -> (lines, bytes, bytes of text)"""
    names, sizes = gr.genome.get_chrom_cpg_sizes()
    cum = np.cumsum(sizes)
    start0, end0, mult = 0, seg.n_sites, None
    if bed_path:
        start0, mult = multiplicities(gr.genome, bed_rows(require_file(bed_path)))
        end0 = start0 + mult.size
    elif not gr.is_whole():
        start0, end0 = gr.sites[0] - 1, gr.sites[1] - 1
    return seg.beta2bed(fd, sample, names, cum, start0, end0, mult, min_cov=min_cov, mean=mean, keep_na=keep_na, slab_sites=slab_sites, bgzf=bgzf)


def beta_to_bed(beta_path, gr, bed_path, min_cov, mean, keep_na, force, opath, device=0, deflate='host', slab_sites=0):
    """beta2bed.py:22-31"""
    from . import _lib
    check_deflate(deflate, opath)
    if not delete_or_skip(opath, force):
        return
    same_size = beta_sanity_check(beta_path, gr.genome)              # (view.py:36: the warning comes before the suffix is looked at)
    elem = beta_elem(beta_path)
    if not same_size:
        raise IllegalArgumentError(f'{beta_path}: the file and the genome {gr.genome.genome} differ in their number of sites')
    min_cov = max(1, min_cov)                                        # (beta2bed.py:13: only `min_cov > 1` adds the filter)
    rows = load_rows(beta_path)
    to_stdout = opath is None or opath == '/dev/stdout'
    with _lib.Segmenter(device) as seg:
        (seg.set_lbetas if elem == 2 else seg.set_betas)([rows])
        seg.set_loci(gr.genome.loci())
        sink = out = None
        if to_stdout:
            sys.stdout.flush()
            fd = 1
        elif opath.endswith('.gz') and deflate != 'device':
            sink = _GzipSink(opath)
            fd = sink.fd
        else:
            out = open(opath, 'wb')
            fd = out.fileno()
        try:
            try:
                write_bed(seg, fd, gr, bed_path, min_cov, mean, keep_na, slab_sites=slab_sites, bgzf=deflate == 'device')
            except _lib.SegmentorError as e:
                raise IllegalArgumentError(f'{beta_path}: {e.msg}')
        finally:
            if sink:
                sink.close()
            if out:
                out.close()


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('beta_path')
    parser.add_argument('-f', '--force', action='store_true', help='Overwrite existing files if existed')
    parser.add_argument('--keep_na', action='store_true', help='If set, missing CpG sites are not removed from the output')
    parser.add_argument('--mean', action='store_true', help='Output a mean methylation value column instead of <meth,cov> columns')
    parser.add_argument('-c', '--min_cov', type=int, default=1,
                        help='Minimal coverage to consider when computing beta values.'
                             ' Default is 1 (include all observations). '
                             ' Sites with less than MIN_COV coverage are considered as missing.'
                             ' Only relevant if --mean is specified.')
    parser.add_argument('--outpath', '-o', default='/dev/stdout', help='Output path. [stdout]')
    add_where_options(parser, bed_file=True)
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    parser.add_argument('--deflate', choices=['host', 'device'], default='host',
                        help='Where a .gz output is compressed: in this process by zlib [host], or on the GPU into BGZF members (device)')
    parser.add_argument('--slab_sites', type=int, default=0, help='Sites per slab of text; 0: the default of the library. Changes speed only [0]')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Convert beta file to bed file.
    """
    args = parse_args(argv)
    require_file(args.beta_path)
    gr = GenomicRegion(args)
    try:
        beta_to_bed(args.beta_path, gr, args.bed_file, args.min_cov, args.mean, args.keep_na, args.force, args.outpath, args.device, args.deflate, args.slab_sites)
    except BrokenPipeError:                                        # e.g. the output is piped to head (cview.py:12-17)
        os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())


if __name__ == '__main__':
    main()
