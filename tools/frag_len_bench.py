#!/usr/bin/env python3
"""`wgbstools frag_len` on the hg19-shaped synthetic pat file of tools/homog_bench.py (profiles/frag_len_*.txt).

Input: the same BGZF pat file of --reads reads (default 10^8; reads of 1-12 CpGs, counts 1-40, sorted by start, generated in
pieces of disjoint site ranges), so that k_frag_hist and k_homog_count read the same text.

Reports, as median [min, max] of --reps runs:
  kernel   k_frag_hist alone over the decompressed text fed in 64 MB chunks (HIP events): GB/s of text, reads/s — for the whole
           genome (every line counts) and for a block list (the blocks of homog_bench: two searches' worth of selection per line,
           and the sortedness check)
  homog    k_homog_count over the same chunks and blocks (--homog): the kernel this one is measured against
  cli      frag_len.frag_hist from the .pat.gz to the histogram with --inflate host and --inflate device: wall, and its split into
           inflate / feed
"""
import argparse
import json
import os
import os.path as op
import sys
import tempfile
import time

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tools'))

from homog_bench import N_SITES, blocks_table, pat_piece, stats          # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-frag', type=int, default=30)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--homog', action='store_true', help='also time k_homog_count over the same chunks')
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()
    d = args.workdir or tempfile.mkdtemp(prefix='frag_bench_')
    os.makedirs(d, exist_ok=True)
    try:
        run(args, d)
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)


def run(args, d):
    from wgbs_tools_amd import _lib, frag_len, homog

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    n_reads = int(args.reads)
    t0 = time.perf_counter()
    s, e, _ = blocks_table(7, N_SITES)
    step = N_SITES // args.pieces
    per = n_reads // args.pieces
    text = b''.join(pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces))
    pat = op.join(d, 'bench.pat.gz')
    homog.write_bgzf(pat, text, 16)
    res = dict(n_sites=N_SITES, n_blocks=int(s.size), n_reads=per * args.pieces, text_bytes=len(text), pat_gz_bytes=op.getsize(pat),
               max_frag=args.max_frag, input_s=round(time.perf_counter() - t0, 1))
    say(res)
    CH = 64 << 20
    chunks, pos = [], 0
    while pos < len(text):
        cut = text.rfind(b'\n', pos, pos + CH) + 1 if pos + CH < len(text) else len(text)
        chunks.append(text[pos:cut])
        pos = cut

    def kernel(what, make):
        kms, walls, total = [], [], None
        for _ in range(args.reps):
            with make() as h:
                t = time.perf_counter()
                for c in chunks:
                    h.feed(c)
                out = h.finish()
                walls.append(time.perf_counter() - t)
                kms.append(h.kernel_ms())
            total = int(out.astype(np.int64).sum())
        km = stats(kms)
        say(dict(what=what, kernel_ms=km, text_GB_per_s=round(len(text) / km['median'] / 1e6, 1),
                 reads_per_s=float('%.4g' % (res['n_reads'] / km['median'] * 1e3)), feed_finish_wall_s=stats(walls), counted=total))
        return out

    whole = kernel('kernel k_frag_hist, whole genome', lambda: _lib.FragLen(args.max_frag))
    say(dict(what='histogram, whole genome', hist=whole.tolist()))
    kernel('kernel k_frag_hist, block list (%d blocks)' % s.size, lambda: _lib.FragLen(args.max_frag, s, e))
    if args.homog:
        edges = homog.parse_range(homog.range_text(3))
        kernel('kernel k_homog_count, the same chunks and blocks', lambda: _lib.Homog(s, e, edges, 3))
    for inflate in ('host', 'device'):
        parts = {k: [] for k in ('inflate_s', 'feed_s', 'kernel_ms', 'wall_s')}
        for _ in range(args.reps):
            t = {}
            t0 = time.perf_counter()
            got = frag_len.frag_hist(pat, args.max_frag, inflate=inflate, timings=t)
            t['wall_s'] = time.perf_counter() - t0
            assert np.array_equal(got, whole)
            for k in parts:
                parts[k].append(t[k])
        out = {k: stats(v) for k, v in parts.items()}
        say(dict(what='cli (frag_len.frag_hist: .pat.gz -> histogram), --inflate ' + inflate, **out,
                 text_MB_per_s=round(len(text) / out['wall_s']['median'] / 1e6, 1)))


if __name__ == '__main__':
    main()
