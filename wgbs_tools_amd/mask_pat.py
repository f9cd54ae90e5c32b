"""`wgbstools mask_pat` on MI355X: a pat file with the sites of a blocks table hidden from every read — what is run to blank out SNP,
imprinted or blacklisted CpGs before `segment`, `homog` or `find_markers` see a sample.

Drop-in for the reference's src/python/mask_pat.py and its tool src/pat2beta/mask_pat.cpp (same flags; same output file), written
against their contract (mask_pat.py:13-42, mask_pat.cpp:12-104, cview.py:25-52, cview.cpp:87-128, patter_utils.cpp:270-280,
src/collapse_pat.pl) — the reference's pipe `cview | mask_pat | sort -k2,2n -k3,3 | collapse_pat.pl | bgzip` in one engine:

    output    PREFIX.pat.gz.  An existing output is skipped with one line on stderr unless -f is given; an output that is the input
              is refused.
    select    the interval [s, e) of -s / -r (the whole genome: [1, nr_sites + 1)): a read `rs, pattern` is dropped when rs >= e or
              rs + len - 1 < s; else it passes whole and uncut.  The selection looks at the read as the file has it.
    mask      the hidden sites are the union of [startCpG, endCpG) over the rows of -b: columns 4 and 5 of at least 5, in any order;
              the rows may overlap, nest and repeat.  Empty lines and lines that begin with '#' are skipped, and so is a row in front
              of the first block whose first field is `chr` (a header).  A file that ends with .gz is gunzipped.  Every pattern byte
              that is not '.' and whose site rs + i is hidden becomes '.'.
    strip     always: trailing dots go (nothing but dots: the read is dropped), then leading dots, their number added to rs — also on
              reads the mask did not touch.
    order     as `LC_ALL=C sort -k2,2n -k3,3`: by start as a number, then the pattern's bytes (a prefix first), then the chromosome's.
    collapse  adjacent lines equal in chromosome, start and pattern become one with the exact int64 sum of their counts.
    --beta / --lbeta   this build's `pat2beta` on the output, into the output's directory.

One `view` engine does all of it (view.view_pats with a mask: wgbsseg_patview_set_mask, include/wgbsseg.h, csrc/view_kernels.h): the
hidden sites become a bitmap on the device, the cut that the measure and the pack pass share sees a hidden site as '.', the survivors
are sorted, collapsed and deflated into BGZF members there; only those are written.  The engine runs with STRIP | SORT and min_len 1.
The input is inflated on the host or, with `--inflate device`, on the GPU.  `[mask_pat] loaded N sites` goes to stderr, N the number of
hidden sites as the device's plan counts them.  No CPU fallback.

Deliberate deviations from the reference:
  1. -L / --bed_file as the SELECTING region is refused as not part of this build (`view -L` is not).
  2. No `.csi` index is written (this build never reads one); one line on stderr says so.
  3. An invalid -b table is refused with its row number (from 1, as an editor counts lines) instead of being processed: a startCpG or
     endCpG that is not a number (NA), endCpG <= startCpG, startCpG < 1, fewer than 5 columns, no usable row.  Each of these makes the
     reference's tool print `failed in mask_pat` and exit 0, and its pipe write an empty output.
  4. A fifth column in the pat file is refused, as in `view` (`failed in view: invalid line ...`); the reference passes it through.
     So are a malformed line and a read that starts before the read before it.
  5. The sort is the C locale's, whatever the caller's locale (the reference sorts in the caller's).
  6. A count below 1 is refused (`failed in view: count < 1 at byte N`).  The reference's `cview` collapses the selected reads once
     before the mask: a run whose sum is <= 0 vanishes there and would be summed into what the mask makes equal here.  With counts of
     at least 1 the two agree, and pat files written by wgbstools hold nothing else.
  7. The whole genome is one pass and one sort, as in `merge`.  -@ is accepted and unused.

Out of scope: -L selection; writing an index; `mix_pat`.
"""
import argparse
import gzip
import os
import os.path as op
import re

import numpy as np

from .cliutil import add_threads_option, add_where_options, require_file
from .genome import GenomicRegion, IllegalArgumentError, eprint
from .merge import merge_interval
from .pat2beta import add_inflate_option, pat2beta
from .view import _write_all, view_pats

_INT = re.compile(r'[ \t\n\x0b\x0c\r]*([+-]?\d+)')                  # std::stoi: white space, a sign, digits; what follows is ignored
MAX_SITE = 2 ** 31 - 1


def _stoi(field):
    m = _INT.match(field)
    return int(m.group(1)) if m else None


def mask_blocks_of(text, path='the blocks table'):
    """the (startCpG, endCpG) blocks of a -b table's text, in file order -> (starts, ends) as int64 arrays; deviation 3's refusals"""
    starts, ends = [], []
    for row, line in enumerate(text.split('\n'), 1):
        if not line or line.startswith('#'):
            continue
        tok = line.split('\t')
        if len(tok) < 5:
            raise IllegalArgumentError(f'mask_pat: {path}: row {row} has {len(tok)} columns (chr, start, end, startCpG, endCpG: at least 5)')
        if not starts and tok[0] == 'chr':
            continue
        a, b = _stoi(tok[3]), _stoi(tok[4])
        if a is None or b is None:
            raise IllegalArgumentError(f'mask_pat: {path}: row {row}: startCpG / endCpG "{tok[3]}" / "{tok[4]}" is not a number')
        if b <= a:
            raise IllegalArgumentError(f'mask_pat: {path}: row {row}: endCpG <= startCpG ({a}, {b})')
        if a < 1:
            raise IllegalArgumentError(f'mask_pat: {path}: row {row}: startCpG < 1 ({a})')
        if b > MAX_SITE:
            raise IllegalArgumentError(f'mask_pat: {path}: row {row}: endCpG {b} (at most {MAX_SITE})')
        starts.append(a)
        ends.append(b)
    if not starts:
        raise IllegalArgumentError(f'mask_pat: {path}: no usable row (0 sites to hide)')
    return np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64)


def read_mask_blocks(path):
    require_file(path)
    with (gzip.open(path, 'rb') if path.endswith('.gz') else open(path, 'rb')) as f:
        return mask_blocks_of(f.read().decode('latin-1'), path)


def mask_pat(pat, out_path, starts, ends, s, e, device=0, inflate='host', timings=None):
    """the reads of `pat` over [s, e) with the sites of the blocks hidden, stripped, sorted and collapsed, as BGZF members to out_path
    -> (lines, bytes written)"""
    require_file(pat, '.pat.gz')
    tmp = out_path + '.tmp%d' % os.getpid()                         # (a refused input leaves no half-written output behind)
    try:
        with open(tmp, 'wb') as f:
            got = view_pats([pat], s, e, lambda piece: _write_all(f.fileno(), piece), strip=True, min_len=1, sort=True, device=device,
                            inflate=inflate, deflate=True, timings=timings, mask=(starts, ends))
        os.replace(tmp, out_path)
    finally:
        if op.isfile(tmp):
            os.remove(tmp)
    return got


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('pat_path', help='pat file')
    add_where_options(parser, bed_file=True)
    add_threads_option(parser)
    fmt = parser.add_mutually_exclusive_group(required=False)
    fmt.add_argument('--beta', action='store_true', help='create beta from output pat')
    fmt.add_argument('--lbeta', action='store_true', help='create lbeta from output pat')
    parser.add_argument('-f', '--force', action='store_true', help='Overwrite existing file if existed')
    parser.add_argument('-p', '--prefix', help='Output prefix for the masked pat file', required=True)
    parser.add_argument('-b', '--sites_to_hide', required=True,
                        help='bed file with sites / blocks to mask out. must be 5 column format (chr, start, end, startCpG, endCpG)')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    return parser.parse_args(argv)


def check_args(args):
    """deviation 1, the two input files and the output path -> the output path"""
    require_file(args.pat_path, '.pat.gz')
    require_file(args.sites_to_hide)
    if args.bed_file:
        raise IllegalArgumentError('mask_pat -L / --bed_file is not part of this build')
    out = args.prefix + '.pat.gz'
    if op.realpath(out) == op.realpath(args.pat_path):
        raise IllegalArgumentError(f'mask_pat: the output path is identical to the input file: {out}')
    return out


def main(argv=None):
    """
    mask out sites from a pat file
    """
    args = parse_args(argv)
    out_path = check_args(args)
    if op.isfile(out_path) and not args.force:
        eprint(f'File {out_path} already exists. Skipping it. Use [-f] flag to force overwrite.')
        return
    starts, ends = read_mask_blocks(args.sites_to_hide)
    s, e = merge_interval(GenomicRegion(args))
    t = {}
    mask_pat(args.pat_path, out_path, starts, ends, s, e, device=args.device, inflate=args.inflate, timings=t)
    eprint(f'[mask_pat] loaded {t.get("hidden_sites", 0)} sites')
    eprint(f'[mask_pat] no .csi index is written for {out_path}: this build reads pat files without one')
    if args.beta or args.lbeta:
        eprint(f'generate {"l" if args.lbeta else ""}beta file')
        pat2beta(out_path, op.dirname(out_path) or '.', args=args, force=True)


if __name__ == '__main__':
    main()
