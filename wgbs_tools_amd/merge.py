"""`wgbstools merge` on MI355X: the pat files or the beta files of replicates pooled into one file — what is run between `pat2beta` /
`view` and `segment`.

Drop-in for the reference's src/python/merge.py (same flags; same output file), written against its contract (merge.py:46-140,:144-190,
utils_wgbs.py:277-290 trim_to_uint8, cview.py:25-80, src/collapse_pat.pl):

    output    prefix + the first input's extension (`.pat.gz`, `.beta`, `.lbeta`; with -l and `.beta` inputs `prefix.lbeta`).  An
              existing output is skipped with one line on stderr unless -f is given; an output that is one of the inputs is refused.
    .beta     every input has the same extension and the same size.  Per site M = the sum of meth, C = the sum of cov, exact; with
              max = 255 (65535 with -l): where C > max, M = int(M / C * max) — numpy's float64 division, then the product, then the C
              cast — and C = max; then both wrap to uint8 (uint16 with -l), as numpy's astype does.  The rows are uploaded once and
              summed by one kernel (wgbsseg_merge_rows, csrc/merge_kernels.h); the result is written as it comes home.
    .pat.gz   every file's reads over the interval of -s / -r (the whole genome: [1, nr_sites + 1)), cut as --strict / --strip /
              --min_len ask, all sorted together as `LC_ALL=C sort -k2,2n -k3,3` and equal lines collapsed into one with the sum of
              their counts: ONE `view` engine takes every file (view.view_pats: wgbsseg_patview_next_file between two files), sorts
              and collapses the records of all of them and deflates the text into BGZF members on the device; only those are written
              — the reference's output is always bgzipped.  The input is inflated on the host or, with `--inflate device`, on the GPU.

No CPU fallback.

Deliberate deviations from the reference:
  1. --labels and -L / --bed_file are refused as not part of this build.  With labels the reference orders tied lines by the text of
     their per-file sums; that needs a second sort key.
  2. No `.csi` index is written (this build never reads one); one line on stderr says so.
  3. The whole genome is one pass and one sort by (start, pattern, chromosome), not one pass per chromosome in the genome's order.  The
     two agree whenever every read's sites lie inside the range of the chromosome it names.
  4. A count below 1 in a pat file is refused (`failed in view: file K: count < 1 at byte N`, K from 0 in argument order).  The
     reference collapses every file by itself before `sort -m`: a run of one file whose sum is <= 0 vanishes there and would be summed
     into the other files' runs here.  With counts of at least 1 the two agree, and pat files written by wgbstools hold nothing else.
     Like `view`, a malformed line and a read that starts before the read before it in the same file are refused, with the file and the
     byte offset inside it.
  5. `.lbeta` inputs without -l are refused (the reference would write uint8 values into a file named .lbeta); `.bin` is refused as
     not part of this build.
  6. --no_gaps, --no_sort, --shuffle and -np are accepted and change nothing, as in the reference, whose extract_view_flags drops them;
     one line on stderr says so.  -T is accepted and unused: nothing is sorted on disk.

Out of scope: --labels and -L (`mix_pat`, which does label its reads, is mix_pat.py); writing an index; starting the merge passes of the sort from whole-file runs instead of
512-record runs (profiles/view_mi355x.txt: 8.0 M records sort in 7.1 ms beside hundreds of ms of feed).
"""
import argparse
import os
import os.path as op
import sys

import numpy as np

from .cliutil import add_where_options, require_file
from .genome import GenomicRegion, IllegalArgumentError, eprint
from .pat2beta import add_inflate_option, splitextgz
from .view import _write_all, view_pats

IGNORED_VIEW_FLAGS = (('no_gaps', '--no_gaps'), ('no_sort', '--no_sort'), ('shuffle', '--shuffle'), ('nanopore', '-np'))


def merge_interval(gr):
    """[s, e) of a GenomicRegion; the whole genome is [1, nr_sites + 1)"""
    if gr.is_whole():
        return 1, gr.genome.get_nr_sites() + 1
    s, e = gr.sites
    return int(s), int(e)


def merge_pats(pats, out_path, s, e, strict=False, strip=False, min_len=1, device=0, inflate='host', timings=None):
    """the reads of `pats` over [s, e), sorted and collapsed together, as BGZF members to out_path -> (lines, bytes written)"""
    for p in pats:
        require_file(p, '.pat.gz')
    tmp = out_path + '.tmp%d' % os.getpid()                         # (a refused input leaves no half-written output behind)
    try:
        with open(tmp, 'wb') as f:
            got = view_pats(pats, s, e, lambda piece: _write_all(f.fileno(), piece), strict=strict, strip=strip, min_len=min_len, sort=True,
                            device=device, inflate=inflate, deflate=True, timings=timings)
        os.replace(tmp, out_path)
    finally:
        if op.isfile(tmp):
            os.remove(tmp)
    return got


def check_betas(betas):
    """one extension, one size -> bytes per count"""
    ext = op.splitext(betas[0])[1]
    for b in betas:
        require_file(b)
        if op.splitext(b)[1] != ext:
            raise IllegalArgumentError(f'merge: {b} does not end with {ext} as {betas[0]} does: all inputs must have one extension')
    size = op.getsize(betas[0])
    for b in betas:
        if op.getsize(b) != size:
            raise IllegalArgumentError(f'merge: {b} holds {op.getsize(b)} bytes, {betas[0]} holds {size}: all inputs must have one size')
    elem = 2 if ext == '.lbeta' else 1
    if size == 0 or size % (2 * elem):
        raise IllegalArgumentError(f'merge: {betas[0]} holds {size} bytes: not a whole number of sites')
    return elem


def merge_betas(betas, out_path, lbeta=False, device=0, timings=None):
    """the rows of `betas` summed and saturated on the device -> the array written to out_path"""
    from . import _lib
    elem = check_betas(betas)
    dtype = np.uint16 if elem == 2 else np.uint8
    rows = [np.memmap(b, dtype=dtype, mode='r').reshape(-1, 2) for b in betas]
    try:
        with _lib.Segmenter(device) as seg:
            (seg.set_lbetas if elem == 2 else seg.set_betas)(rows)
            data = seg.merge_rows(list(range(len(betas))), lbeta=lbeta)
            if timings is not None:
                timings['kernel_ms'] = seg.last_merge_rows_ms()
    except _lib.SegmentorError as e:
        raise IllegalArgumentError(f'{betas[0]}: {e.msg}')
    data.tofile(out_path)
    return data


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('input_files', nargs='+')
    parser.add_argument('-p', '--prefix', help='Prefix of output file', required=True)
    parser.add_argument('-f', '--force', action='store_true', help='Overwrite existing file if existed')
    parser.add_argument('-T', '--temp_dir', help='accepted and unused: nothing is sorted on disk')
    parser.add_argument('-v', '--verbose', action='store_true')
    parser.add_argument('-l', '--lbeta', action='store_true', help='Use lbeta file (uint16) instead of beta (uint8)')
    parser.add_argument('--labels', nargs='+', help='labels for the mixed reads: refused in this build')
    add_where_options(parser, bed_file=True)
    parser.add_argument('--strict', action='store_true', help='pat: cut every read to the interval of -s / -r')
    parser.add_argument('--strip', action='store_true', help='pat: remove the dots at both ends of a read (its start moves with them)')
    parser.add_argument('--min_len', type=int, default=1, help='pat: drop reads left with fewer than MIN_LEN sites [1]')
    parser.add_argument('--no_gaps', action='store_true', help='accepted; changes nothing (as in the reference)')
    parser.add_argument('--shuffle', action='store_true', help='accepted; changes nothing (as in the reference)')
    parser.add_argument('--no_sort', action='store_true', help='accepted; changes nothing (as in the reference)')
    parser.add_argument('-np', '--nanopore', action='store_true', help='accepted; the whole of every file is read in any case')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    return parser.parse_args(argv)


def output_path(args):
    """prefix + the first input's extension (-l with .beta inputs: .lbeta); refused when it is one of the inputs"""
    ext = splitextgz(args.input_files[0])[1]
    if ext == '.bin':
        raise IllegalArgumentError(f'merge of .bin files is not part of this build ({args.input_files[0]})')
    if ext not in ('.beta', '.lbeta', '.pat.gz'):
        raise IllegalArgumentError(f'merge: unknown input format: {args.input_files[0]} (.pat.gz, .beta or .lbeta)')
    if ext == '.lbeta' and not args.lbeta:
        raise IllegalArgumentError('merge of .lbeta files needs -l / --lbeta: without it the reference writes uint8 values into a file named .lbeta')
    out = args.prefix + ('.lbeta' if ext == '.beta' and args.lbeta else ext)
    if op.realpath(out) in [op.realpath(p) for p in args.input_files]:
        raise IllegalArgumentError(f'merge: the output path is identical to one of the input files: {out}')
    return out, ext


def main(argv=None):
    """
    Merge files.
    Accumulate all reads / observations from multiple (>=2) input files,
    and output a single file of the same format.
    Supported formats: pat.gz, beta, lbeta
    """
    args = parse_args(argv)
    if args.labels:
        raise IllegalArgumentError('merge --labels is not part of this build')
    if args.bed_file:
        raise IllegalArgumentError('merge -L / --bed_file is not part of this build')
    out_path, ext = output_path(args)
    if ext == '.pat.gz':
        for p in args.input_files:
            require_file(p, '.pat.gz')
        if args.min_len < 1:
            raise IllegalArgumentError(f'--min_len must be at least 1 (got {args.min_len})')
    else:
        check_betas(args.input_files)
    if op.isfile(out_path) and not args.force:
        eprint(f'File {out_path} already exists. Skipping it. Use [-f] flag to force overwrite.')
        return
    if ext != '.pat.gz':
        merge_betas(args.input_files, out_path, lbeta=args.lbeta, device=args.device)
        return
    given = [flag for name, flag in IGNORED_VIEW_FLAGS if getattr(args, name)]
    if given:
        eprint(f'[wt merge] {", ".join(given)}: accepted and without effect on merge, as in the reference')
    s, e = merge_interval(GenomicRegion(args))
    t = {}
    lines, nbytes = merge_pats(args.input_files, out_path, s, e, strict=args.strict, strip=args.strip, min_len=args.min_len, device=args.device,
                               inflate=args.inflate, timings=t)
    if args.verbose:
        eprint(f'[wt merge] {len(args.input_files)} files, {t.get("records", 0)} reads -> {lines} lines, {nbytes} bytes in {out_path}')
    eprint(f'[wt merge] no .csi index is written for {out_path}: this build reads pat files without one')


if __name__ == '__main__':
    main()
