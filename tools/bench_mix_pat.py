#!/usr/bin/env python3
"""`wgbstools mix_pat` on the hg19-shaped synthetic inputs of the other profiles (profiles/mix_pat_mi355x.txt).

Input: the BGZF pat files of tools/merge_bench.py (--reads reads per file, default 10^7; reads of 1-12 CpGs, counts 1-40, sorted by
start; copies with shifted counts).  Two and four files over the whole genome, each --reps times (median [min, max]):
    merge     view.view_pats as `wgbstools merge` runs it (no sources): the figures to hold beside profiles/merge_mi355x.txt — its kernels
              are the ones of that profile
    mix       the same call with sources, as mix_pat.mix_once runs it, at two adjusted rates: 0.25 (one draw per count: reps 1) and 1.0
              (four draws per count at p = 0.25: reps 4)
Per run: the device time of the feed (measure + pack over all chunks: where the draws happen, twice), of the inflate, the sort, collapse
+ emit (with labels: + the order of tied lines) and the deflate, the wall time from the .pat.gz files to the last fetched byte, and what
the sampler saw.  `feed_ratio` = the feed with sampling / the feed of merge: what the draws cost."""
import argparse
import json
import os
import os.path as op
import sys
import tempfile
import time

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tools'))
sys.path.insert(0, op.join(ROOT, 'tests'))

from homog_bench import N_SITES, pat_piece, stats          # noqa: E402
from merge_bench import shifted                             # noqa: E402
from view_bench import Sink                                 # noqa: E402

KEYS = ('kernel_ms', 'inflate_ms', 'sort_ms', 'emit_ms', 'deflate_ms', 'wall_s')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e7)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--files', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--adj', type=float, nargs='+', default=[0.25, 1.0], help='the adjusted rate of every file, one run each')
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    from wgbs_tools_amd import homog, mix_pat, view
    d = args.workdir or tempfile.mkdtemp(prefix='mix_bench_')
    os.makedirs(d, exist_ok=True)
    try:
        n_reads, n_files = int(args.reads), max(args.files)
        t0 = time.perf_counter()
        step, per = N_SITES // args.pieces, n_reads // args.pieces
        text = b''.join(pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces))
        paths = []
        for k in range(n_files):
            paths.append(op.join(d, 'copy%d.pat.gz' % k))
            homog.write_bgzf(paths[-1], text if k == 0 else shifted(text, k), 16)
        say(dict(n_sites=N_SITES, n_reads_per_file=per * args.pieces, text_bytes_per_file=len(text), files=n_files,
                 pat_gz_bytes=[op.getsize(p) for p in paths], input_s=round(time.perf_counter() - t0, 1)))
        del text
        s, e = 1, N_SITES + 1
        for n in args.files:
            runs = [('merge', None)] + [('mix, adjusted rate %g' % a, a) for a in args.adj]
            merge_feed = None
            for what, adj in runs:
                sources = None
                if adj is not None:
                    T, reps, p = mix_pat.sampler_args(adj)
                    sources = ([('file%d' % k, T, reps) for k in range(n)], args.seed, 0)
                view.view_pats(paths[:n], s, e, Sink(), sort=True, inflate='device', deflate=True, sources=sources)      # warm-up
                parts, info = {k: [] for k in KEYS}, None
                for _ in range(args.reps):
                    t, sink = {}, Sink()
                    t1 = time.perf_counter()
                    lines, nbytes = view.view_pats(paths[:n], s, e, sink, sort=True, inflate='device', deflate=True, timings=t, sources=sources)
                    t['wall_s'] = time.perf_counter() - t1
                    assert sink.n == nbytes
                    for k in KEYS:
                        parts[k].append(t.get(k, 0.0))
                    info = dict(lines=lines, bgzf_bytes=nbytes, records=t['records'], merge_passes=t['merge_passes'], order=t['order'])
                    if adj is not None:
                        info.update(T=T, reps=reps, p=p, sampled_reads=t['sampled_reads'], sampled_dropped=t['sampled_dropped'], sampled_kept=t['sampled_kept'])
                rec = dict(what='%s, whole genome, %d files, --inflate device, deflated on the device' % (what, n), **info, **{k: stats(v) for k, v in parts.items()})
                if adj is None:
                    merge_feed = rec['kernel_ms']['median']
                else:
                    rec['feed_ratio'] = round(rec['kernel_ms']['median'] / merge_feed, 3)
                say(rec)
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
