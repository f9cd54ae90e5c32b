"""`wgbstools bed2beta` on MI355X: BED methylation calls -> the `.beta` file every other command here starts from.

Drop-in for the reference's src/python/bed2beta.py (same flags, output names, skip / overwrite rule), written against the formats:

    bed     tab-separated text (optionally gzip): chr, start, end, #meth, #total (+ ignored columns) — Bismark coverage files, bedMethyl
            dumps, published per-CpG tables.  The first line is a header, and is skipped unread, exactly when its second field is not
            made of decimal digits only (bed2beta.py:13-14).  Empty lines are skipped.  With --add_one the position is start + 1.
    .beta   nr_sites x (#meth, #total) uint8: the line whose (chr, position) is a CpG of the genome's dictionary gives that site's pair;
            of several lines at one (chr, position) the first in the file wins (bed2beta.py:19 drop_duplicates); a line on an unknown
            chromosome or at no CpG is dropped (bed2beta.py:50, the left merge); a pair whose #total exceeds 255 is stored as
            (trunc(#meth / #total * 255), 255) (utils_wgbs.py:277-290); a site without a line is 0, 0.

The reference reads the whole file into a pandas frame and left-merges the 28 M rows of the dictionary with it.  Here the text goes to
the GPU in chunks (pat2beta.feed_pat: inflated on the host, or with `--inflate device` the members of a BGZF file on the GPU) and one
kernel pass parses it, finds every line's chromosome and CpG and keeps the first line per site with one 64-bit atomicMin
(wgbsseg_bedbeta_*, include/wgbsseg.h; csrc/bed2beta_kernels.h).  The dictionary is loaded and uploaded once for all files.  No CPU fallback.

Deliberate deviations from the reference:
  - Refused, each with the prefix `failed in bed2beta:` and the byte offset of the lowest such line: a line of fewer than five fields; a
    start, #meth or #total that is not plain decimal digits (no sign, no '.', no exponent, no '\\r') or longer than 18 digits; #meth >
    #total (numpy wraps it); #total > 2^31 - 1.  An empty file is refused too.
  - -d / --debug is not part of this build (it needs `tabix`).
  - stderr reports, per file, the lines read, the lines matched, the lines dropped for an unknown chromosome, the lines dropped for not
    being a CpG and the duplicates dropped among the matched lines (the reference counts duplicates among all lines).  stderr is not
    part of parity.
  - `--inflate device` needs a BGZF file; a plain gzip .bed.gz is inflated on the host, and one line on stderr says so.
"""
import argparse
import gzip
import os.path as op

from .cliutil import require_file
from .convert import delete_or_skip
from .genome import GenomeRefPaths, IllegalArgumentError, eprint
from .pat2beta import add_inflate_option, feed_pat, splitextgz

PEEK_BYTES = 1 << 20


def first_line_is_header(bed_path):
    """bed2beta.py:13-14 on the first line of the (inflated) file: a header exactly when its second tab-separated field is not made of
    ASCII decimal digits only."""
    opener = gzip.open if bed_path.endswith('.gz') else open
    try:
        with opener(bed_path, 'rb') as f:
            line = f.readline(PEEK_BYTES)
    except (OSError, EOFError) as e:
        raise IllegalArgumentError(f'Invalid gzip data in {bed_path}: {e}')
    if not line:
        raise IllegalArgumentError(f'bed2beta: {bed_path} is empty')
    fields = line.rstrip(b'\n').split(b'\t')
    return not (len(fields) > 1 and fields[1].isdigit() and fields[1].isascii())


def out_path_of(bed_path, outdir):
    return op.join(outdir, splitextgz(op.basename(bed_path))[0] + '.beta')


def bed2betas(bed_paths, outdir='.', genome=None, add_one=False, force=False, device=0, inflate='host'):
    """bed2beta.py:28-51 -> [(bed path, output path or None when skipped, the engine's counters + kernel_ms)]"""
    from . import _lib
    done, engine, spent, inflated = [], None, 0.0, 0.0
    try:
        for bed in bed_paths:
            eprint(f'[wt bed] Converting {op.basename(bed)}...')
            out = out_path_of(bed, outdir)
            if not delete_or_skip(out, force):
                done.append((bed, None, None))
                continue
            header = first_line_is_header(bed)
            if engine is None:                                    # the dictionary: loaded and uploaded at most once
                g = GenomeRefPaths(genome)
                names, sizes = g.get_chrom_cpg_sizes()
                engine = _lib.BedBeta(g.loci(), names, sizes, add_one=add_one, header=header, device=device)
            else:
                engine.next_file(add_one=add_one, header=header)
            timings = {}
            try:
                feed_pat(engine, bed, timings, inflate=inflate)
                rows, stats = engine.finish()
            except _lib.SegmentorError as e:
                raise IllegalArgumentError(f'{bed}: {e.msg}')
            total = engine.kernel_ms()
            stats['kernel_ms'], spent = total - spent, total
            on_device = ''
            if 'inflate_ms' in timings:                           # the engine's total over its files, like kernel_ms
                stats['inflate_ms'], inflated = timings['inflate_ms'] - inflated, timings['inflate_ms']
                on_device = ', inflate %.3f ms' % stats['inflate_ms']
            rows.tofile(out)
            eprint('[wt bed] %s: %d lines, %d matched, %d dropped for an unknown chromosome, %d dropped for not being a CpG, '
                   '%d duplicates dropped, scan %.3f ms%s' % (op.basename(bed), stats['lines'], stats['matched'], stats['unknown_chrom'],
                                                             stats['not_cpg'], stats['duplicates'], stats['kernel_ms'], on_device))
            done.append((bed, out, stats))
    finally:
        if engine is not None:
            engine.close()
    return done


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('bed_paths', nargs='+')
    parser.add_argument('-f', '--force', action='store_true', help='Overwrite existing files if existed')
    parser.add_argument('-d', '--debug', action='store_true', help='refused here: it needs tabix')
    parser.add_argument('--add_one', action='store_true', help='Add 1 to start column, to match with CpG.bed.gz notation.')
    parser.add_argument('--outdir', '-o', default='.', help='Output directory. Default is current directory [.]')
    parser.add_argument('--genome', help='Genome reference name.')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    return parser.parse_args(argv)


def main(argv=None):
    """
    Convert bed[.gz] file[s] to beta file[s].
    bed file should be of the format (tab-separated):
    chr    start    end    #meth    #total
    """
    args = parse_args(argv)
    if args.debug:
        raise IllegalArgumentError('bed2beta -d / --debug is not part of this build (it needs tabix)')
    for bed in args.bed_paths:
        require_file(bed)
    if not op.isdir(args.outdir):
        raise IllegalArgumentError(f'Invalid output dir: {args.outdir}')
    bed2betas(args.bed_paths, args.outdir, args.genome, args.add_one, args.force, args.device, args.inflate)


if __name__ == '__main__':
    main()
