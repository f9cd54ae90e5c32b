"""`wgbstools init_genome` on MI355X: a FASTA file -> the genome directory `references/NAME/` every other command starts from.

Drop-in for src/python/init_genome.py, which runs `samtools faidx | tail` per chromosome, joins and upper-cases the lines in Python,
applies re.finditer('CG'), builds a 28 M-row DataFrame and hands it to `bgzip` and `tabix`.  Here the text goes through the GPU once:

    scan      every CpG of every sequence (csrc/fasta_core.h has the rule, csrc/fasta_kernels.h the kernels): a header is a line that
              begins with '>', the name ends at the first blank, every other byte but '\\n' and '\\r' is a base, and a site is a C / c
              whose next base in the same sequence is G / g, whatever line breaks lie between.  The text is fed in pieces cut at any
              byte: an unwrapped FASTA (one line of 250 MB per chromosome) is read like a wrapped one.
    select    the sequences that are chromosomes (is_valid_chrome: ^(chr)?([\\d]+|[XYM]|(MT))$), stably sorted by chromosome_order unless
              --no_sort is given; the others are scanned and dropped, sites are numbered over the kept ones.
    write     CpG.bed.gz (`chr \\t locus \\t site`, formatted and deflated into BGZF on the GPU, the end-of-file member last),
              rev.CpG.bed.gz (a relative link to it), chrome.size and CpG.chrome.size (a chromosome without a CpG gets 0), loci.u32 (the
              loci as uint32, written AFTER CpG.bed.gz: genome.py takes the cache that is not older), genome.fa[.gz] (a link to the
              FASTA; its .fai and .gzi beside it when they exist).  Unless --no_default is given, references/default then points to NAME.

The input is plain text, BGZF (inflated on the host, or on the GPU with --inflate device) or plain gzip (inflated on the host).
No CPU fallback.

Deliberate deviations from the reference:
  - --fasta_path is required: downloading a FASTA is not part of this build, and the command never reaches for a host.  -d / --debug is
    not part of this build.  -@ is accepted and ignored.
  - No .fai of our own (that is `samtools faidx`), no .csi / .tbi index (this build never reads one; the closing message says so), no
    supplemental hg19 / hg38 links.
  - A '\\r' is skipped wherever it stands (the reference strips it at the ends of a line only).  A FASTA whose sequence lines carry
    blanks is refused (the reference strips them at the ends of a line and counts them inside it).
  - Text before the first header, a header without a name, a name above 255 bytes, a byte of a sequence outside printable ASCII, a
    sequence above 2^32 - 2 bases and two sequences of one name are refused, with the byte offset in the uncompressed text.
"""
import argparse
import gzip
import os
import os.path as op
import re
import shutil
import time

from .cliutil import require_file
from .genome import IllegalArgumentError, eprint, references_root
from .pat2beta import CHUNK_BYTES, _feed_bgzf, add_inflate_option, bgzf_pieces
from .set_default_ref import set_def_ref
from .view import _write_all

_VALID = re.compile(r'^(chr)?([\d]+|[XYM]|(MT))$')


def is_valid_chrome(chrome):
    """init_genome.py:278-281"""
    return bool(_VALID.match(chrome))


def chromosome_order(c):
    """init_genome.py:263-275"""
    if c.startswith('chr'):
        c = c[3:]
    if c.isdigit():
        return int(c)
    return {'X': 10000, 'Y': 10001, 'M': 10002, 'MT': 10002}.get(c, 10003)


def kept_order(names, no_sort=False):
    """indices of the sequences the dictionary keeps, in its order (init_genome.py:131-137: the filter, then a stable sort)"""
    kept = [i for i, c in enumerate(names) if is_valid_chrome(c)]
    return kept if no_sort else sorted(kept, key=lambda i: chromosome_order(names[i]))


def text_pieces(path, chunk_bytes=CHUNK_BYTES):
    """the text of a FASTA file (plain, BGZF or gzip) in pieces, cut anywhere"""
    if path.endswith('.gz'):
        gen = bgzf_pieces(path)
        bgzf = yield from gen
        if bgzf:
            return
    opener = gzip.open if path.endswith('.gz') else open
    try:
        with opener(path, 'rb') as f:
            while True:
                buf = f.read(chunk_bytes)
                if not buf:
                    return
                yield buf
    except (OSError, EOFError) as e:
        raise IllegalArgumentError(f'Invalid gzip data in {path}: {e}')


def feed_fasta(engine, path, timings, inflate='host'):
    """every piece of the file to the engine; timings['inflate_s'] / ['feed_s'] as pat2beta.feed_pat leaves them"""
    if inflate == 'device':
        done = path.endswith('.gz') and _feed_bgzf(engine, path, timings)
        if done:
            timings['inflate_ms'] = engine.inflate_ms()
            return
        if path.endswith('.gz'):
            eprint(f'[wgbs_tools_amd] {path} is not BGZF: --inflate device does not apply, inflating on the host')
    t_inflate = t_feed = 0.0
    it = iter(text_pieces(path))
    while True:
        t0 = time.perf_counter()
        piece = next(it, None)
        t1 = time.perf_counter()
        t_inflate += t1 - t0
        if piece is None:
            break
        engine.feed(piece)
        t_feed += time.perf_counter() - t1
    timings['inflate_s'], timings['feed_s'] = t_inflate, t_feed


def _text(name):
    try:
        return name.decode('ascii')
    except UnicodeDecodeError:
        raise IllegalArgumentError(f'Invalid FASTA: the sequence name {name!r} is not ASCII')


def build_dictionary(fasta, out_dir, no_sort=False, device=0, inflate='host', timings=None):
    """the files of the dictionary into out_dir (which exists) -> (kept names, bases, sites per chromosome)"""
    from . import _lib
    t = timings if timings is not None else {}
    try:
        with _lib.Fasta(device=device) as eng:
            feed_fasta(eng, fasta, t, inflate=inflate)
            table = eng.finish_scan()
            t['kernel_ms'] = eng.kernel_ms()
            names = [_text(s['name']) for s in table]
            order = kept_order(names, no_sort)
            eng.select(order)                                       # (none kept: the library's refusal)
            lines, nbytes = eng.dict(deflate=True)
            t['gather_ms'], t['emit_ms'], t['deflate_ms'] = eng.phase_ms()
            t['sequences'], t['text_bytes'] = eng.n_seqs, eng.n_text
            dict_path = op.join(out_dir, 'CpG.bed.gz')
            with open(dict_path, 'wb') as f:
                for piece in eng.chunks():
                    _write_all(f.fileno(), piece)
            os.symlink('CpG.bed.gz', op.join(out_dir, 'rev.CpG.bed.gz'))
            kept = [(names[i], table[i]['bases'], table[i]['sites']) for i in order]
            with open(op.join(out_dir, 'chrome.size'), 'w') as f:
                f.writelines('%s\t%d\n' % (c, b) for c, b, _ in kept)
            with open(op.join(out_dir, 'CpG.chrome.size'), 'w') as f:
                f.writelines('%s\t%d\n' % (c, s) for c, _, s in kept)
            eng.loci().tofile(op.join(out_dir, 'loci.u32'))         # after CpG.bed.gz: the cache must not be the older one
    except _lib.SegmentorError as e:
        raise IllegalArgumentError(f'{fasta}: {e.msg}')
    return kept


def link_fasta(fasta, out_dir):
    """init_genome.py:116-123, without a .fai of our own"""
    src = op.abspath(fasta)
    name = 'genome.fa' + ('.gz' if fasta.endswith('.gz') else '')
    os.symlink(src, op.join(out_dir, name))
    for ext in ('.fai', '.gzi'):
        if op.isfile(src + ext):
            os.symlink(src + ext, op.join(out_dir, name + ext))


def setup_dir(name, force):
    """init_genome.py:97-110"""
    out_dir = op.join(references_root(), name)
    if op.lexists(out_dir):
        if not force:
            raise IllegalArgumentError(f'[wt init] Error: genome {name} already exists ({out_dir}). Use -f to overwrite it.')
        if op.islink(out_dir) or not op.isdir(out_dir):
            os.unlink(out_dir)
        else:
            shutil.rmtree(out_dir)
    os.makedirs(out_dir)
    eprint(f'[wt init] Setting up genome reference files in {out_dir}')
    return out_dir


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('name', help='name of the genome (e.g. hg19, mm9...).\nA directory of this name will be created in references/')
    parser.add_argument('--fasta_path', help='path to a reference genome FASTA file (plain, BGZF or gzip)')
    parser.add_argument('-f', '--force', action='store_true', help='Overwrite existing files if existed')
    parser.add_argument('--no_default', action='store_true',
                        help='Do not set this genome as the default reference for wgbstools.\nThis setting can be changed with wgbstools set_default_ref')
    parser.add_argument('-d', '--debug', action='store_true', help='not part of this build')
    parser.add_argument('--no_sort', action='store_true',
                        help='If set, keep the chromosome order of the reference genome.\nDefault behaviour is to sort 1,2,...,10,11,...,X,Y,M')
    parser.add_argument('-@', '--threads', type=int, help='accepted and ignored: the text is scanned on the GPU')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    return parser.parse_args(argv)


def main(argv=None):
    """ Init genome reference. """
    args = parse_args(argv)
    if args.debug:
        raise IllegalArgumentError('init_genome -d / --debug is not part of this build')
    if not args.fasta_path:
        raise IllegalArgumentError('init_genome without --fasta_path is not part of this build: downloading a FASTA is not part of this build '
                                   '(fetch it yourself and pass --fasta_path)')
    if not args.name or '/' in args.name or args.name in ('.', '..', 'default'):
        raise IllegalArgumentError(f'init_genome: invalid genome name: {args.name}')
    require_file(args.fasta_path)
    out_dir = setup_dir(args.name, args.force)
    eprint('[wt init] Processing chromosomes...')
    timings = {}
    try:
        kept = build_dictionary(args.fasta_path, out_dir, no_sort=args.no_sort, device=args.device, inflate=args.inflate, timings=timings)
        link_fasta(args.fasta_path, out_dir)
    except Exception:
        shutil.rmtree(out_dir, ignore_errors=True)                 # (half a genome directory would be taken for a whole one)
        raise
    eprint('[wt init] %d of %d sequences kept, %d CpGs; kernels %.3f ms, gather %.3f ms, emit %.3f ms, deflate %.3f ms' % (
        len(kept), timings['sequences'], sum(s for _, _, s in kept), timings['kernel_ms'], timings['gather_ms'], timings['emit_ms'], timings['deflate_ms']))
    eprint(f'[wt init] no .fai, .csi or .tbi index is written for {out_dir}: this build reads the dictionary without one')
    eprint(f'[wt init] Finished initialization of genome {args.name}')
    if not args.no_default:
        set_def_ref(args.name)


if __name__ == '__main__':
    main()
