"""`wgbstools bam2pat` on MI355X: alignments -> the `.pat.gz` and `.beta` files everything else here starts from.

Drop-in for the head of the reference's pipeline (src/python/bam2pat.py, src/pipeline_wgbs/patter.cpp, patter_utils.cpp), which runs
`samtools view | match_maker | patter | sort -k2,2n -k3,3 | uniq -c | bgzip` per chromosome.  Here the input is SAM TEXT — what
`samtools view [-h]` prints, the very input `patter` reads — as a plain file, gzip, BGZF or standard input (`-`):

    filter    a line stays when (FLAG & F) == 0, (FLAG & f) == f and MAPQ >= q (-F [1796], --include_flags [3 when the file is
              paired-end, else none], -q [10]: samtools view's); --top_strand keeps FLAG 99 / 147 (paired-end) or 0, --bottom_strand 83 /
              163 or 16 (bam2pat.py:159-170).  The file is paired-end when FLAG & 1 is set in its first alignment (bam2pat.py:262-267).
    one line  CIGAR M = X copy bases, D N insert N, I S skip bases, H does nothing (clean_CIGAR); at every CpG of the genome's dictionary
              under the read a top read calls C for CG and T for TG, a bottom read C for CG and T for CA one base on (compareSeqToRef);
              --clip hides the calls in the first and last CLIP bases; the pat runs from the first called site to the last.
    mates     in a paired-end file two consecutive lines that stay, with one QNAME and one RNAME, are a pair — the reference streams every
              chromosome by itself, so only lines of one chromosome meet there; of k such lines (1, 2), (3, 4), ... pair.  The contract is
              patter's own: MATES ARE ADJACENT, as Bismark and bwa-meth write them.  A pair merges as merge_PE does: a site the two call
              differently becomes '.', the dots at both ends go, a span above 300 sites is dropped.
    output    reads shorter than --min_cpg are dropped; the rest is sorted by (start, pattern), equal reads are counted, and the text
              `chrom, start, pattern, count` is deflated into BGZF members on the GPU: dir/x.pat.gz, and dir/x.beta (`.lbeta` with -l) by
              `pat2beta` on that file unless --no_beta is given.  The name follows the reference's pretty_name; with `-` it comes from --name.

Every line's calling, the pairing and the merge run on the GPU (wgbsseg_patview_set_sam, include/wgbsseg.h; csrc/sam_kernels.h over
csrc/sam_core.h), the sort, collapse and deflate are the `view` engine's.  With `--inflate device` the members of a BGZF input are
inflated there too.  No CPU fallback.

Deliberate deviations from the reference:
  - A `.bam` or `.cram` argument is not part of this build (there is no htslib here, and BAM records cannot be split without walking
    them): `samtools view -h x.bam | wgbstools bam2pat - --name x` is the way in.  Matching the mates of coordinate-sorted input
    (`match_maker`) is not part of this build either: a paired-end file whose header says `SO:coordinate` is refused, and the message
    names `samtools collate -O` and `samtools sort -n`.
  - Not part of this build, each refused by name: -r / -s / -L, --blacklist, --mbias, --blueprint, --nanopore (also when one of the first
    200 alignments carries an MM:Z: or Mm:Z: tag), --long, -rg, -d.  -T and -@ are accepted and ignored.
  - FLAG, POS and MAPQ must be plain decimal digits; a line where they are not, a line of fewer than 11 fields and a QNAME above 254
    bytes are invalid (counted, dropped; such a line still separates the lines around it, as in patter).
  - No `.csi` index is written (this build never reads one); one line on stderr says so.
  - stderr reports the lines, header lines, filtered, invalid, unknown-chromosome, empty and short reads, the pairs, the lines of a
    paired-end file left single and the pairs merged too long.  stderr is not part of parity.
"""
import argparse
import gzip
import os
import os.path as op
import sys

from .cliutil import require_file
from .convert import delete_or_skip
from .genome import GenomeRefPaths, IllegalArgumentError, eprint
from .pat2beta import CHUNK_BYTES, add_inflate_option, feed_pat, splitextgz
from .view import _write_all

PAT_SUFF = '.pat.gz'
MAPQ = 10
FLAGS_FILTER = 1796
PEEK_ALIGNMENTS = 200
NOT_HERE = (('region', '-r / --region'), ('sites', '-s / --sites'), ('whitelist', '-L / --whitelist'), ('blacklist', '--blacklist'), ('mbias', '--mbias'),
            ('blueprint', '--blueprint'), ('nanopore', '--nanopore'), ('long', '--long'), ('read_group', '-rg / --read_group'), ('debug', '-d / --debug'))


def pretty_name(path):
    """utils_wgbs.py:423-424"""
    return splitextgz(op.basename(path))[0]


def peek(lines):
    """the head of the input, line by line -> (paired, coordinate-sorted by its @HD, an MM / Mm tag among the first alignments); None when
    there is no alignment"""
    paired, coordinate, mods, seen = None, False, False, 0
    for line in lines:
        if not line.strip(b'\n'):
            continue
        if line.startswith(b'@'):
            if line.startswith(b'@HD') and b'SO:coordinate' in line:
                coordinate = True
            continue
        tok = line.split(b'\t')
        if paired is None:
            if len(tok) < 2 or not tok[1].isdigit():
                raise IllegalArgumentError('bam2pat: the first alignment line has no FLAG')
            paired = bool(int(tok[1]) & 1)
        mods = mods or b'\tMM:Z:' in line or b'\tMm:Z:' in line
        seen += 1
        if seen >= PEEK_ALIGNMENTS:
            break
    return None if paired is None else (paired, coordinate, mods)


def peek_file(path):
    opener = gzip.open if path.endswith('.gz') else open
    try:
        with opener(path, 'rb') as f:
            return peek(f)
    except (OSError, EOFError) as e:
        raise IllegalArgumentError(f'Invalid gzip data in {path}: {e}')


def check_head(head, shown):
    if head is None:
        raise IllegalArgumentError(f'bam2pat: {shown} holds no alignment')
    paired, coordinate, mods = head
    if mods:
        raise IllegalArgumentError(f'bam2pat: {shown} carries MM:Z: / Mm:Z: modification tags: --nanopore is not part of this build')
    if paired and coordinate:
        raise IllegalArgumentError(f'bam2pat: {shown} is paired-end and sorted by coordinate (@HD SO:coordinate): its mates are not adjacent, and matching '
                                   'them is not part of this build; bring them together with `samtools collate -O` or `samtools sort -n` first')
    return paired


def stdin_chunks(first, stream, chunk_bytes=CHUNK_BYTES):
    """standard input as plain text in pieces that end on line boundaries; first: what has been read already"""
    rest = first
    while True:
        buf = stream.read(chunk_bytes)
        if not buf:
            break
        buf = rest + buf
        cut = buf.rfind(b'\n') + 1
        rest = buf[cut:]
        if cut:
            yield buf[:cut]
    if rest:
        yield rest if rest.endswith(b'\n') else rest + b'\n'


def sam2pat(feed, out_path, genome, paired, args, timings=None):
    """feed(engine): the SAM text into the engine -> (lines, bytes) of out_path, the engine's counters; nothing is written when no read is left"""
    from . import _lib
    names, sizes = genome.get_chrom_cpg_sizes()
    include = args.include_flags if args.include_flags is not None else (3 if paired else 0)
    strand = 1 if args.top_strand else 2 if args.bottom_strand else 0
    t = timings if timings is not None else {}
    try:
        with _lib.PatView(1, genome.get_nr_sites() + 1, sort=True, device=args.device) as v:
            v.set_sam(genome.loci(), names, sizes, paired=paired, exclude_flags=args.exclude_flags, include_flags=include, mapq=args.mapq, strand=strand,
                      clip=args.clip, min_cpg=args.min_cpg)
            feed(v)
            lines, nbytes = v.finish(deflate=True)
            t['kernel_ms'] = v.kernel_ms()
            t['sort_ms'], t['emit_ms'], t['deflate_ms'] = v.phase_ms()
            t.update(v.info())
            stats = v.sam_info()
            if lines:
                tmp = out_path + '.tmp%d' % os.getpid()
                try:
                    with open(tmp, 'wb') as f:
                        for piece in v.chunks():
                            _write_all(f.fileno(), piece)
                    os.replace(tmp, out_path)
                finally:
                    if op.isfile(tmp):
                        os.remove(tmp)
    except _lib.SegmentorError as e:
        raise IllegalArgumentError(e.msg)
    return lines, nbytes, stats


def check_input(path, args):
    """-> (the output's name, how the input is called in messages)"""
    if path == '-':
        if not args.name:
            raise IllegalArgumentError('bam2pat: standard input needs --name (the output is NAME.pat.gz)')
        return args.name, 'standard input'
    if path.endswith(('.bam', '.cram')):
        raise IllegalArgumentError(f'bam2pat of {path} is not part of this build (it reads SAM text, not BAM / CRAM): '
                                   f'samtools view -h {path} | wgbstools bam2pat - --name {pretty_name(path)}')
    require_file(path)
    return pretty_name(path), path


def bam2pat(path, args, genome_of):
    """one input -> the pat path written (None: skipped, or no read was left); genome_of(): the genome, loaded when first needed"""
    name, shown = check_input(path, args)
    eprint('[wt bam2pat] sam:', shown)
    pat = op.join(args.out_dir, name + PAT_SUFF)
    if not delete_or_skip(pat, args.force):
        return None
    timings = {}
    if path == '-':
        stream = sys.stdin.buffer
        first = stream.read(CHUNK_BYTES)                            # (the head is looked at where it lies: a pipe cannot be read twice)
        paired = check_head(peek(first.splitlines(keepends=True)), shown)

        def feed(v):
            for chunk in stdin_chunks(first, stream):
                v.feed(chunk)
    else:
        paired = check_head(peek_file(path), shown)

        def feed(v):
            feed_pat(v, path, timings, inflate=args.inflate)
    lines, nbytes, st = sam2pat(feed, pat, genome_of(), paired, args, timings)
    eprint('[wt bam2pat] %s-end: %d lines, %d header, %d filtered, %d invalid, %d on unknown chromosomes, %d empty, %d with too few CpGs, %d pairs, '
           '%d left single, %d pairs merged too long; kernels %.3f ms' % ('paired' if paired else 'single', st['lines'], st['header'], st['filtered'], st['invalid'],
                                                                         st['unknown_chrom'], st['empty'], st['short'], st['pairs'], st['left_single'], st['too_long'],
                                                                         timings.get('kernel_ms', 0.0)))
    if not lines:
        eprint('[wt bam2pat] No reads found. No pat file is generated')
        return None
    eprint(f'[wt bam2pat] generated {pat} ({lines} lines, {nbytes} bytes)')
    eprint(f'[wt bam2pat] no .csi index is written for {pat}: this build reads pat files without one')
    if not args.no_beta:
        from .pat2beta import pat2beta
        beta = pat2beta(pat, args.out_dir, args, force=True)
        eprint(f'[wt bam2pat] generated {beta}')
    return pat


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('sam', nargs='+', help='SAM text as `samtools view [-h]` prints it: x.sam, x.sam.gz (gzip or BGZF), or - for standard input')
    parser.add_argument('--name', help='with -: the name of the output (NAME.pat.gz)')
    parser.add_argument('--out_dir', '-o', default='.')
    parser.add_argument('--force', '-f', action='store_true', help='overwrite existing files if exists')
    parser.add_argument('--genome', help='Genome reference name.')
    parser.add_argument('--min_cpg', type=int, default=1, help='Reads covering less than MIN_CPG sites are removed [1]')
    parser.add_argument('--clip', type=int, default=0, help='Clip for each read the first and last CLIP characters [0]')
    parser.add_argument('--include_flags', type=int, help='flags to include (samtools view parameter -f) [3 for PE, None for SE]')
    parser.add_argument('-F', '--exclude_flags', type=int, default=FLAGS_FILTER, help=f'flags to exclude (samtools view parameter -F) [{FLAGS_FILTER}]')
    parser.add_argument('-q', '--mapq', type=int, default=MAPQ, help=f'Minimal mapping quality (samtools view parameter) [{MAPQ}]')
    strand = parser.add_mutually_exclusive_group()
    strand.add_argument('--top_strand', action='store_true', help='Consider only top strand reads')
    strand.add_argument('--bottom_strand', action='store_true', help='Consider only bottom strand reads')
    parser.add_argument('--no_beta', action='store_true', help='Do not generate a beta file')
    parser.add_argument('-l', '--lbeta', action='store_true', help='Use lbeta file (uint16) instead of beta (uint8)')
    parser.add_argument('--verbose', '-v', action='store_true')
    parser.add_argument('-T', '--temp_dir', help='accepted and ignored: nothing is sorted on disk')
    parser.add_argument('-@', '--threads', type=int, help='accepted and ignored: the reads are processed on the GPU')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    parser.add_argument('-r', '--region', help='not part of this build')
    parser.add_argument('-s', '--sites', help='not part of this build')
    parser.add_argument('-L', '--whitelist', nargs='?', const=True, default=False, help='not part of this build')
    parser.add_argument('--blacklist', nargs='?', const=True, default=False, help='not part of this build')
    parser.add_argument('--mbias', '-mb', action='store_true', help='not part of this build')
    parser.add_argument('--blueprint', '-bp', action='store_true', help='not part of this build')
    parser.add_argument('--nanopore', '-np', action='store_true', help='not part of this build')
    parser.add_argument('--long', action='store_true', help='not part of this build')
    parser.add_argument('-rg', '--read_group', help='not part of this build')
    parser.add_argument('--debug', '-d', action='store_true', help='not part of this build')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Generate pat & beta files out of SAM text (the output of samtools view):
    every read is called against the CpG dictionary, mates are merged,
    equal reads are counted, all on the GPU
    """
    args = parse_args(argv)
    for attr, flag in NOT_HERE:
        if getattr(args, attr):
            raise IllegalArgumentError(f'bam2pat {flag} is not part of this build')
    if not op.isdir(args.out_dir):
        raise IllegalArgumentError(f'Invalid output dir: {args.out_dir}')
    if args.min_cpg < 0 or args.clip < 0:
        raise IllegalArgumentError(f'bam2pat: --min_cpg and --clip must be at least 0 (got {args.min_cpg}, {args.clip})')
    if not (0 <= args.exclude_flags <= 0xffff and 0 <= (args.include_flags or 0) <= 0xffff and 0 <= args.mapq <= 255):
        raise IllegalArgumentError('bam2pat: -F and --include_flags are SAM flags (0 .. 65535), -q is a mapping quality (0 .. 255)')
    if args.sam.count('-') > 1 or ('-' in args.sam and len(args.sam) > 1):
        raise IllegalArgumentError('bam2pat: standard input (-) is the only input when it is given')
    for path in args.sam:
        check_input(path, args)
    loaded = []

    def genome_of():
        if not loaded:
            loaded.append(GenomeRefPaths(args.genome))
        return loaded[0]
    for path in args.sam:
        bam2pat(path, args, genome_of)

if __name__ == '__main__':
    main()
