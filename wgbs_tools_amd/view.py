"""`wgbstools view` / `wgbstools cview` on MI355X: the reads of a pat file as pat text — those an interval lets through, cut to it,
stripped of dots, sorted and with equal lines collapsed — the read-level command `merge`, `mix_pat` and `cview -L` of the reference
pipe through.

Drop-in for the pat side of the reference's src/python/view.py and cview.py (same flags and output), written against its contract
(view.py:85-115, cview.py:25-80,:117-142, src/cview/cview.cpp:8-17,:87-167 with one block, patter_utils.cpp:260-280,
src/collapse_pat.pl):

    interval  [s, e) in CpG indexes: -s / -r through GenomicRegion; the whole genome is [1, nr_sites + 1)
    per line  `chrom, rs, pattern, count`, in this order:
              1. dropped when rs >= e (the reference stops reading there: on reads that ascend by start, a test on the read) or
                 when rs + len - 1 < s
              2. --strict: the first max(0, s - rs) characters go and rs' = max(rs, s); then at most e - rs' characters stay
              3. --strip: trailing dots go (nothing but dots: the read is dropped), then leading dots, their number added to rs'
              4. --min_len: dropped when it exceeds what is left
              5. --no_gaps: dropped when a '.' is left
    order     with -s / -r and without --no_sort: as `LC_ALL=C sort -k2,2n -k3,3` — by rs' as a number, then the pattern's bytes (a
              prefix first), then the chromosome's; what is still tied differs in the count only and keeps its input order.  For the
              whole genome and with --no_sort the file's order is kept — with --strip the output is then not ascending, as the
              reference's is not.
    collapse  adjacent lines equal in chrom, rs' and pattern become one with the exact int64 sum of their counts; a sum <= 0 prints
              nothing (Perl's `if ($count > 0)`)
    output    `chrom\\trs'\\tpattern\\tsum\\n` to stdout or -o; with `-o x.gz --deflate device` the text is deflated into BGZF members on
              the GPU (beta2bed's member rule, kernels and end-of-file member) and only those are written; without it the reference's
              plain text is written, whatever the name

The file's text — inflated on the host or, with `--inflate device`, on the GPU — goes through the feed the other pat commands share;
the survivors stay on the device, where they are sorted, collapsed and written out (wgbsseg_patview_*, include/wgbsseg.h,
csrc/view_kernels.h).  No CPU fallback.  view_pats() is the same over several files — one engine, wgbsseg_patview_next_file between two
files, the reads of all of them sorted and collapsed together — and what `wgbstools merge` (merge.py) runs; view_pat() is view_pats() of one.

Deliberate deviations from the reference:
  1. No index and no tabix window: the whole file is read.  A read that starts more than 150 sites before s and still reaches it is
     kept, as on the reference's own `gunzip -c` branch.  -np is accepted and changes nothing.
  2. Refused input, with the byte offset and the prefix `failed in view:`: a malformed line (fewer than four fields, a site or count
     that is not a number, an empty pattern, any byte between the count's digits and the newline: a fifth column, a carriage
     return); a read that starts before the read before it — always, the whole genome included, because rs >= e stops the reference
     there.  A collapsed sum of 10^15 or more is refused too: Perl would print it in exponent form.  A start is printed as a plain
     decimal number, and so is a count (the reference passes the file's own text on where it computes nothing: a start "+7"
     stays "+7" when nothing is cut, a count "+3" stays "+3" when its run has one line).
  3. Refused arguments, each saying it is not in this build: --sub_sample, --shuffle, -L / --bed_file, an input that is not .pat.gz
     (for .beta / .lbeta the message names `beta2bed`).  Also refused: --min_len < 1, s < 1, e <= s.
  4. The sort is the C locale's, whatever the caller's locale (the reference sorts in the caller's).
"""
import argparse
import os
import sys

from .beta2bed import check_deflate
from .cliutil import add_where_options, require_file
from .genome import GenomicRegion, IllegalArgumentError
from .pat2beta import add_inflate_option, feed_pat


def view_interval(gr):
    """[s, e) of a GenomicRegion, and whether the reference sorts there (cview.py:27-44)"""
    if gr.is_whole():
        return 1, gr.genome.get_nr_sites() + 1, False
    s, e = gr.sites
    return int(s), int(e), True


def check_interval(s, e, min_len=1):
    if min_len < 1:
        raise IllegalArgumentError(f'--min_len must be at least 1 (got {min_len})')
    if s < 1:
        raise IllegalArgumentError(f'view: the interval starts at site {s} (sites count from 1)')
    if e <= s:
        raise IllegalArgumentError(f'view: the interval [{s}, {e}) is empty')


def view_pats(pats, s, e, sink, strict=False, strip=False, no_gaps=False, min_len=1, sort=True, device=0, inflate='host', deflate=False,
              initial_records=0, timings=None, mask=None, sources=None):
    """the view of the reads of several pat files over [s, e) as if they were one file's (what `merge` is): every file is fed to ONE
    engine, next_file() between two of them; every piece of the result to sink(bytes) -> (lines, bytes).  A refusal of the engine
    names the file by its index in `pats` (from 0) once there is more than one; the message here adds its path in front.
    mask: (starts, ends) of blocks whose sites are hidden from every read (`mask_pat`: _lib.PatView.set_mask).
    sources: ([(label, T, reps) per file], seed, rep) — every file's reads thinned and labelled (`mix_pat`: _lib.PatView.set_labels /
    set_source with stream = rep << 16 | file); None: nothing of it."""
    from . import _lib
    check_interval(s, e, min_len)
    t = timings if timings is not None else {}
    spent = {}
    at = 0
    if sources is not None:
        per_file, seed, rep_no = sources
        if len(per_file) != len(pats):
            raise IllegalArgumentError(f'view: {len(per_file)} sources for {len(pats)} files')
        if not (0 <= int(rep_no) < 65536 and len(pats) <= 65536):
            raise IllegalArgumentError(f'view: repetition {rep_no} of {len(pats)} files (both below 65536)')
    try:
        with _lib.PatView(s, e, strict=strict, strip=strip, no_gaps=no_gaps, sort=sort, min_len=min_len, device=device,
                          initial_records=initial_records, mask=mask) as v:
            ranks = v.set_labels([x[0] for x in per_file]) if sources is not None else None
            for at, pat in enumerate(pats):
                if at:
                    v.next_file()
                if ranks is not None:
                    v.set_source(ranks[at], per_file[at][1], per_file[at][2], seed, (int(rep_no) << 16) | at)
                one = {}
                feed_pat(v, pat, one, inflate=inflate)
                for key, val in one.items():                     # (inflate_ms is the engine's running total)
                    spent[key] = val if key == 'inflate_ms' else spent.get(key, 0.0) + val
            at = None
            lines, nbytes = v.finish(deflate=deflate)
            t.update(spent)
            t['kernel_ms'] = v.kernel_ms()
            t['sort_ms'], t['emit_ms'], t['deflate_ms'] = v.phase_ms()
            t.update(v.info())
            if mask is not None:
                t.update(v.mask_info())
            if sources is not None:
                t.update(v.sample_info())
            for piece in v.chunks():
                sink(piece)
    except _lib.SegmentorError as err:
        where = pats[at] if at is not None else _refused_file(pats, err.msg)
        raise IllegalArgumentError(f'{where}: {err.msg}')
    return lines, nbytes


def _refused_file(pats, msg):
    """the path finish()'s message is about: `file K:` names it when several files were fed"""
    import re
    m = re.search(r'\bfile (\d+):', msg) if len(pats) > 1 else None
    return pats[int(m.group(1))] if m and int(m.group(1)) < len(pats) else pats[0] if len(pats) == 1 else ', '.join(pats)


def view_pat(pat, s, e, sink, strict=False, strip=False, no_gaps=False, min_len=1, sort=True, device=0, inflate='host', deflate=False,
             initial_records=0, timings=None):
    """the view of one pat file over [s, e): every piece of the result to sink(bytes) -> (lines, bytes)"""
    return view_pats([pat], s, e, sink, strict=strict, strip=strip, no_gaps=no_gaps, min_len=min_len, sort=sort, device=device, inflate=inflate,
                     deflate=deflate, initial_records=initial_records, timings=timings)


def _write_all(fd, data):
    view = memoryview(data)
    while len(view):
        view = view[os.write(fd, view):]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('input_file', nargs='?')
    add_where_options(parser, bed_file=True)
    parser.add_argument('--strict', action='store_true',
                        help='cut every read to the interval of -s / -r')
    parser.add_argument('--strip', action='store_true', help='remove the dots at both ends of a read (its start moves with them)')
    parser.add_argument('--min_len', type=int, default=1, help='drop reads left with fewer than MIN_LEN sites [1]')
    parser.add_argument('--no_gaps', action='store_true', help='drop reads that still hold a dot')
    parser.add_argument('--shuffle', action='store_true', help='not part of this build')
    parser.add_argument('--no_sort', action='store_true', help='keep the order of the file (no sort before the collapse)')
    parser.add_argument('--sub_sample', type=float, help='not part of this build')
    parser.add_argument('-o', '--out_path', help='where the text goes [stdout]')
    parser.add_argument('-np', '--nanopore', action='store_true', help='accepted; the whole file is read in any case')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    parser.add_argument('--deflate', choices=['host', 'device'], default='host',
                        help='device: with -o PATH.gz, deflate the output on the GPU into BGZF members; host: plain text, as the reference writes [host]')
    return parser.parse_args(argv)


def check_args(args):
    """deviation 3, and the input file"""
    if args.input_file is None:
        raise IllegalArgumentError('view: no input file given')
    require_file(args.input_file)
    if os.path.splitext(args.input_file)[1] in ('.beta', '.lbeta'):
        raise IllegalArgumentError(f'view of a beta file is not part of this build: `wgbstools beta2bed {args.input_file}` prints its sites')
    if not args.input_file.endswith('.pat.gz'):
        raise IllegalArgumentError(f'view of {args.input_file} is not part of this build: the input must end with .pat.gz')
    for given, flag in ((args.sub_sample is not None, '--sub_sample'), (args.shuffle, '--shuffle'), (bool(args.bed_file), '-L / --bed_file')):
        if given:
            raise IllegalArgumentError(f'view {flag} is not part of this build')
    if args.min_len < 1:
        raise IllegalArgumentError(f'--min_len must be at least 1 (got {args.min_len})')
    if args.deflate == 'device':
        check_deflate(args.deflate, args.out_path)


def main(argv=None):
    """
    The reads of a pat file as pat text, filtered by a region or a site range,
    cut, sorted and collapsed on the GPU; to stdout unless -o says otherwise
    """
    args = parse_args(argv)
    check_args(args)
    s, e, sort = view_interval(GenomicRegion(args))
    out = None
    try:
        if args.out_path is None or args.out_path == '/dev/stdout':
            sys.stdout.flush()
            fd = 1
        else:
            out = open(args.out_path, 'wb')
            fd = out.fileno()
        try:
            view_pat(args.input_file, s, e, lambda piece: _write_all(fd, piece), strict=args.strict, strip=args.strip, no_gaps=args.no_gaps,
                     min_len=args.min_len, sort=sort and not args.no_sort, device=args.device, inflate=args.inflate,
                     deflate=args.deflate == 'device')
        finally:
            if out:
                out.close()
    except BrokenPipeError:                                        # e.g. the output is piped to head (cview.py:12-17)
        os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())


if __name__ == '__main__':
    main()
