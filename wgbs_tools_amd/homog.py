"""`wgbstools homog` on MI355X: per block, the number of reads that are mostly unmethylated (U), mixed (X) or mostly methylated
(M) — the `.uxm` input of the UXM atlas workflow (segment a cohort, homog every sample's pat file against the blocks, pick
markers, deconvolve).

Drop-in for the reference's src/python/homog.py (same flags, checks, messages, output names and bytes after decompression),
written against its contract (homog.py:83-131 + src/homog/homog.cpp:154-260):

    bins      without -t the edges are the text "0,{th1},{th2},1", th1 = round(1 - (l-1)/l, 3) + 0.001, th2 = round((l-1)/l, 3)
              (Python's own formatting of those floats), with -t LOW,HIGH "0,LOW,HIGH,1"; the reference's C++ reads each number
              with `stream >> float` — one correctly rounded decimal -> float32 conversion, done here by the C library's strtof.
    counting  a read covering [s, s + len) adds its count to one bin of every block it overlaps (blocks taken in (startCpG,
              endCpG) order, overlapping and nested ones included) while s < endCpG of the LAST such block; the pattern is
              clipped per block (--inclusive: scored whole) — k_homog_count (csrc/homog_kernels.h) says it in full.
    order     blocks not sorted by (startCpG, endCpG): the reference counts in sorted order, then puts the rows back with a
              stable argsort of startCpG ALONE (homog.py:113-118), so equal starts with unequal ends swap rows.  Reproduced.
    output    blocks.merge(counts, how='left', on the five coordinate columns): k rows with identical coordinates become k^2
              rows (every copy paired with every copy's counts).  Text: chr, start, end, startCpG, endCpG, U, X, M to
              <prefix>.uxm.bed.gz (written here as BGZF, compressed on a thread pool: `gunzip -c` and pandas read it as they
              read the reference's single gzip stream); --binary: <prefix>.uxm, uint8 (uint16 with --nr_bits 16) rows, a row
              whose maximum exceeds 2^nr_bits - 1 scaled to row / max * (2^nr_bits - 1) and cut toward zero.

Deliberate deviations from the reference:
  1. No `.csi` index is required (validate_file_list asks for one): the whole pat file is read, as `pat2beta` does here.
  2. With 5,000 blocks or fewer the reference first runs `cview -L` over the blocks.  Without --strict that passes on whole
     reads that overlap a block, in file order (cview.cpp:88-140; extend_blocks.sh merges the regions); a read it drops
     overlaps no block, so it cannot count: on sorted pat files the counts are those of the full-file path used here always.
  3. What the reference silently mangles is refused, naming the byte offset or the row: a malformed pat line (the reference
     prints "failed calculating homog", exits 0 and leaves NaN rows), a read that starts before the read before it (its
     results then depend on the reads' order), a block with startCpG < 1.

Out of scope: the C++ tool's --chrom and -d (`-d` is accepted and ignored, as the reference's wrapper ignores it).  No CPU
fallback: the counting runs on the GPU (wgbsseg_homog_*, include/wgbsseg.h).
"""
import argparse
import ctypes
import os
import os.path as op
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

from .beta_to_blocks import load_blocks_file
from .convert import delete_or_skip
from .genome import IllegalArgumentError
from .pat2beta import add_inflate_option, feed_pat, splitextgz
from .cliutil import default_threads


def homog_log(*args, **kwargs):
    print('[ wt homog ]', *args, file=sys.stderr, **kwargs)


def range_text(rlen, thresholds=None):
    """the bin edges as the text the reference hands its C++ tool (homog.py:96-104)"""
    if thresholds:
        return f'0,{thresholds},1'
    th1 = round(1 - (rlen - 1) / rlen, 3) + 0.001
    th2 = round((rlen - 1) / rlen, 3)
    return f'0,{th1},{th2},1'


_libc = None


def _strtof(tok):
    global _libc
    if _libc is None:
        _libc = ctypes.CDLL(None)
        _libc.strtof.restype = ctypes.c_float
        _libc.strtof.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
    end = ctypes.c_char_p()
    b = tok.encode()
    v = _libc.strtof(b, ctypes.byref(end))
    return v, end.value


def parse_range(text):
    """"0,a,b,1" -> float32 edges, each decimal rounded once (homog.cpp parse_range with split_float_by_comma: read floats while
    they parse, a ',' after each one skipped); the tool's checks: strictly ascending, inside [0, 1], from 0 to 1."""
    vals = []
    for tok in text.split(','):
        v, rest = _strtof(tok)
        if rest == tok.encode():                                    # nothing parsed: the reference's stream stops here
            break
        vals.append(v)
        if rest.strip():
            break
    r = np.array(vals, dtype=np.float32)
    if r.size < 2 or (np.diff(r) <= 0).any() or (r < 0).any() or (r > 1).any() or r[0] > 0 or r[-1] < 1:
        raise IllegalArgumentError(f'Invalid range: {text}')
    return r


def trim_uxm(data, nr_bits):
    """rows of counts -> uint8 / uint16 (homog.py:48-58): a row whose maximum exceeds M = 2^nr_bits - 1 becomes row / max * M
    (float64, cut toward zero), then every value is stored in the narrow type"""
    data = np.array(data, dtype=np.int64)
    top = 2 ** nr_bits - 1
    mx = data.max(axis=1) if data.size else np.zeros(0, dtype=np.int64)
    big = np.flatnonzero(mx > top)
    data[big, :] = data[big, :] / mx[big][:, None] * top
    return data.astype(np.uint16 if nr_bits == 16 else np.uint8)


def merge_rows(blocks):
    """The row pairs of pandas' left merge of the blocks with a copy of themselves on the five coordinate columns: (left, right)
    index arrays, left ascending, for every left row its matches in ascending order (k identical rows -> k^2 pairs)."""
    n = len(blocks)
    idx = np.arange(n, dtype=np.int64)
    key = (blocks.startCpG << 32) | blocks.endCpG
    order = np.argsort(key, kind='stable')
    ks = key[order]
    dup = np.zeros(n, dtype=bool)
    if n > 1:
        same = ks[1:] == ks[:-1]
        dup[1:] |= same
        dup[:-1] |= same
    cand = order[dup]
    if cand.size == 0:
        return idx, idx
    groups = {}
    for i, c in zip(cand.tolist(), blocks.coords_of(cand)):
        groups.setdefault((c, int(blocks.startCpG[i]), int(blocks.endCpG[i])), []).append(i)
    mult = np.ones(n, dtype=np.int64)
    members = {}
    for g in groups.values():
        if len(g) > 1:
            g.sort()
            for i in g:
                members[i] = g
                mult[i] = len(g)
    left = np.repeat(idx, mult)
    right = left.copy()
    first = np.cumsum(mult) - mult
    for i, g in members.items():
        right[first[i]:first[i] + len(g)] = g
    return left, right


def count_blocks(pat, blocks, edges, args, timings=None):
    """int64 counts[len(blocks)][n_bins] in the blocks' own row order, as the reference's wrapper leaves them (the sorted
    counts put back with a stable argsort of startCpG alone: see the module's docstring)."""
    from . import _lib
    order = np.lexsort((blocks.endCpG, blocks.startCpG))
    t = timings if timings is not None else {}
    with _lib.Homog(blocks.startCpG[order], blocks.endCpG[order], edges, args.rlen, args.inclusive, device=getattr(args, 'device', 0)) as h:
        feed_pat(h, pat, t, inflate=getattr(args, 'inflate', 'host'))
        t0 = time.perf_counter()
        try:
            counts = h.finish()
        except _lib.SegmentorError as e:
            raise IllegalArgumentError(f'{pat}: {e.msg}')
        t['finish_s'] = time.perf_counter() - t0
        t['kernel_ms'] = h.kernel_ms()
    counts = counts.astype(np.int64)
    rank = np.argsort(blocks.startCpG, kind='stable')            # homog.py:113-118: the row of sorted position r goes to rank[r]
    inv = np.argsort(rank, kind='stable')
    return counts, counts[inv]


def _bgzf_member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00' + struct.pack('<H', len(body) + 25) + body +
            struct.pack('<II', zlib.crc32(data) & 0xffffffff, len(data)))


def write_bgzf(path, data, threads=None, deflate='host', device=0):
    """`data` as a BGZF file (gzip members of at most 64 KB with the 'BC' size field, then the empty end-of-file member),
    the members compressed on a pool of threads (zlib releases the interpreter lock); deflate='device': on the GPU, by one library
    call (_lib.bgzf_deflate: other bytes, the same text)"""
    if deflate not in ('host', 'device'):
        raise IllegalArgumentError(f"deflate must be 'host' or 'device', not {deflate!r}")
    if deflate == 'device':
        from . import _lib
        packed = _lib.bgzf_deflate(data, device=device, eof=True)
        with open(path, 'wb') as f:
            f.write(packed)
        return
    from concurrent.futures import ThreadPoolExecutor
    mv = memoryview(data)
    pieces = [mv[p:p + 65280] for p in range(0, len(data), 65280)]
    with open(path, 'wb') as f, ThreadPoolExecutor(max(1, min(32, threads or os.cpu_count() or 1))) as pool:
        for m in pool.map(_bgzf_member, pieces, chunksize=16):
            f.write(m)
        f.write(_bgzf_member(b''))


def table_text(blocks, left, values, outdir):
    """the text rows chr, start, end, startCpG, endCpG of blocks[left], then the values as integers"""
    b = blocks.take(left)
    if b.parsed is not None and len(b):
        from . import _lib
        fd, tmp = tempfile.mkstemp(prefix='.homog.', dir=outdir)
        os.close(fd)
        try:
            _lib.blocks_write_table(tmp, b.parsed, values.astype(np.float64), 0, append=False)
            with open(tmp, 'rb') as f:
                return f.read()
        finally:
            os.remove(tmp)
    s_txt, e_txt = b.cpg_text()
    rows = ['\t'.join([c, s, e, a, z] + [str(v) for v in r])
            for c, s, e, a, z, r in zip(b.chr, b.start, b.end, s_txt, e_txt, values.tolist())]
    return ('\n'.join(rows) + '\n').encode() if rows else b''


def homog_process(pat, blocks, edges, args, outdir, prefix, timings=None):
    """homog.py:83-131 for one pat file; returns the path written (None when skipped)."""
    name = splitextgz(op.basename(pat))[0]
    if prefix is None:
        prefix = op.join(outdir, name)
    opath = prefix + '.uxm' + ('' if args.binary else '.bed.gz')
    if not delete_or_skip(opath, args.force):
        homog_log(f'skipping {name}. Use -f to overwrite')
        return None
    t = timings if timings is not None else {}
    raw, counts = count_blocks(pat, blocks, edges, args, t)
    if int(raw.sum()) == 0:
        homog_log(f' [ {name} ] WARNING: all zeros!')
    t0 = time.perf_counter()
    left, right = merge_rows(blocks)
    vals = counts[right]
    if args.binary:
        trim_uxm(vals, args.nr_bits).tofile(opath)
    else:
        write_bgzf(opath, table_text(blocks, left, vals, op.dirname(opath) or '.'), getattr(args, 'threads', None),
                   deflate=getattr(args, 'deflate', 'host'), device=getattr(args, 'device', 0))
    t['write_s'] = time.perf_counter() - t0
    return opath


def check_blocks(blocks, path):
    """homog.py:31-38 (no NA, endCpG > startCpG: 'Invalid blocks file'), then deviation 3: startCpG >= 1"""
    if len(blocks) == 0:
        raise IllegalArgumentError(f'Invalid blocks file: {path}')
    if blocks.na.any():
        homog_log('Some blocks are empty (NA)')
        raise IllegalArgumentError(f'Invalid blocks file: {path}')
    if not (blocks.endCpG - blocks.startCpG > 0).all():
        homog_log('Some blocks are empty (startCpG==endCpG)')
        raise IllegalArgumentError(f'Invalid blocks file: {path}')
    low = np.flatnonzero(blocks.startCpG < 1)
    if low.size:
        raise IllegalArgumentError(f'Invalid blocks file: {path}: row {int(low[0]) + 1} has startCpG {int(blocks.startCpG[low[0]])} < 1')


def blocks_sorted(blocks):
    s, e = blocks.startCpG, blocks.endCpG
    return bool(((s[1:] > s[:-1]) | ((s[1:] == s[:-1]) & (e[1:] >= e[:-1]))).all())


def check_args(args):
    if args.nr_bits not in (8, 16):
        raise IllegalArgumentError('nr_bits must be in {8, 16}')
    if args.rlen < 2:
        raise IllegalArgumentError('rlen must be >= 2')
    if args.thresholds is not None:
        th = args.thresholds.split(',')
        if not len(th) == 2:
            raise IllegalArgumentError('Invalid thresholds')
        th = float(th[0]), float(th[1])
        if not 1 > th[1] > th[0] > 0:
            raise IllegalArgumentError('Invalid thresholds')
    elif args.rlen == 2:
        raise IllegalArgumentError('for rlen==2, --thresholds must be specified')


def check_pats(pats):
    """utils_wgbs.py:355-406 with force_suff '.pat.gz' (deviation 1: no index asked for)"""
    if len(pats[0]) == 1:
        raise IllegalArgumentError(f'Input is not a list of files: {pats}')
    if not pats[0].endswith('.pat.gz'):
        raise IllegalArgumentError(f'Input file {pats[0]} must end with .pat.gz')
    for p in pats:
        if not op.isfile(p):
            raise IllegalArgumentError(f'No such file: {p}')
        if not p.endswith('.pat.gz'):
            raise IllegalArgumentError(f'file {p} must end with .pat.gz')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('input_files', nargs='+', help='one or more pat files')
    parser.add_argument('-b', '--blocks_file', help='blocks path', required=True)
    out = parser.add_mutually_exclusive_group(required=False)
    out.add_argument('-o', '--out_dir', help='output directory. Default is "."')
    out.add_argument('-p', '--prefix', help='output prefix')
    parser.add_argument('--force', '-f', action='store_true', help='Overwrite files if exist')
    parser.add_argument('--inclusive', action='store_true', help='consider the whole read. Opposite of "strict"')
    parser.add_argument('--verbose', '-v', action='store_true')
    parser.add_argument('--binary', action='store_true', help='Output binary files (uint8)')
    parser.add_argument('--genome', help='Genome reference name.')
    parser.add_argument('--nr_bits', type=int, default=8,
                        help='For binary output, specify number of bits for the output format - 8 or 16. '
                             '(e.g. 8 stands for uint8, which means values are trimmed to [0, 255])')
    parser.add_argument('--thresholds', '-t', help='UXM thresholds, LOW,HIGH. E.g, "0.3334,0.666".\n')
    parser.add_argument('--rlen', '-l', type=int, default=3, help='Minimal read length (in CpGs) to consider. Default is 3')
    parser.add_argument('--debug', '-d', action='store_true')
    parser.add_argument('-@', '--threads', type=int, default=default_threads(), help='Threads compressing the output [all CPUs]')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    parser.add_argument('--deflate', choices=['host', 'device'], default='host',
                        help='Where the .bed.gz output is compressed: on the CPU threads of -@ [host], or on the GPU (device)')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Generage homog files. Given a blocks file and pat[s],
    count the number of U,X,M reads for each block for each file
    """
    args = parse_args(argv)
    check_args(args)
    pats = args.input_files
    check_pats(pats)
    outdir, prefix = args.out_dir, args.prefix
    if prefix is not None:
        outdir = op.dirname(prefix)
    if not outdir:
        outdir = '.'
    os.makedirs(outdir, exist_ok=True)
    edges = parse_range(range_text(args.rlen, args.thresholds))
    blocks = load_blocks_file(args.blocks_file)
    check_blocks(blocks, args.blocks_file)
    if not blocks_sorted(blocks):
        homog_log('WARNING: blocks file is not sorted by startCpG. C++ binary will sort internally.')
    for pat in sorted(pats):
        homog_process(pat, blocks, edges, args, outdir, prefix)


if __name__ == '__main__':
    main()
