#!/usr/bin/env python3
"""`wgbstools test_bimodal -L` on an hg19-shaped synthetic run (profiles/bimodal_*.txt).

Input: the run of tools/homog_bench.py — 28 M CpGs, a segmentation-like blocks table (~3.5 M rows, blocks of 1-12 CpGs), a
BGZF pat file of --reads reads (default 10^8; 1-12 CpGs over C / T / H / ., counts 1-40, sorted by start).

Reports, as median [min, max] of --reps runs:
  kernel   every launch of wgbsseg_bimodal_* (parse, order check, gather, EM, drop) over the decompressed text fed in 64 MB
           chunks (HIP events), and rows x EM iterations per second of it
  cli      test_bimodal.multiple_regions from the .pat.gz to the output file, split into inflate (host, BGZF on a thread pool),
           feed (copy + launches, and the EM of the blocks each chunk completes), finish (the last blocks' EM + the results)
           and write (chi-square, BH, text)
--ref-blocks N: also time the reference's own per-block path (read_pat_vis + calc_initial_liklihood + em_pat_matrix +
           chi-square, src/python/test_bimodal.py imported from REF_ROOT) on the first N blocks, on this host's CPU, with the
           block's reads handed over in memory (the `tabix` subprocess it starts per block is not counted).
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


def write_genome_stub(d):
    """a reference directory naming the one chromosome of the run (test_bimodal -L only lists the chromosomes)"""
    import gzip
    os.makedirs(d, exist_ok=True)
    with open(op.join(d, 'CpG.chrome.size'), 'w') as f:
        f.write('chr1\t%d\n' % N_SITES)
    with open(op.join(d, 'chrome.size'), 'w') as f:
        f.write('chr1\t%d\n' % (40 * N_SITES + 10000))
    with gzip.open(op.join(d, 'CpG.bed.gz'), 'wb') as f:
        f.write(b'')
    return d


def ref_per_block(text, s, e, n):
    """seconds per block of the reference's own code on the first n blocks (reads handed over in memory)"""
    ref = os.environ.get('REF_ROOT', '')
    sys.path.insert(0, op.join(ref, 'src', 'python'))
    sys.path.insert(0, op.join(ROOT, 'tests', 'golden'))
    import make_golden_bimodal as M
    M.install_stub()
    import test_bimodal as rt
    from scipy import stats as st
    lines = text[:min(len(text), 40 * 1000 * 1000)].decode().split('\n')
    starts = np.array([int(ln.split('\t')[1]) for ln in lines if ln], dtype=np.int64)
    t0 = time.perf_counter()
    for j in range(n):
        a, b = int(s[j]), int(e[j])
        lo, hi = np.searchsorted(starts, max(1, a - 150)), np.searchsorted(starts, b - 1, 'right')
        mat = rt.read_pat_vis('\n'.join(lines[lo:hi]), a, b, False, 1)
        if mat.shape[0]:
            ll0 = rt.calc_initial_liklihood(mat, should_print=False)
            ll = rt.em_pat_matrix(mat, should_print=False)
            1 - st.chi2.cdf(2 * np.log(2) * (ll - ll0), mat.shape[1])
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ref-blocks', type=int, default=0)
    ap.add_argument('--no-gpu', action='store_true')
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix='bimodal_bench_')
    try:
        run(args, d)
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)


def run(args, d):
    from wgbs_tools_amd import homog, test_bimodal
    n_reads = int(args.reads)
    t0 = time.perf_counter()
    s, e, btext = blocks_table(7, N_SITES)
    blocks = op.join(d, 'blocks.bed')
    with open(blocks, 'w') as f:
        f.write(btext)
    step = N_SITES // args.pieces
    per = n_reads // args.pieces
    text = b''.join(pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces))
    pat = op.join(d, 'bench.pat.gz')
    homog.write_bgzf(pat, text, 16)
    res = dict(n_sites=N_SITES, n_blocks=int(s.size), n_reads=per * args.pieces, text_bytes=len(text), pat_gz_bytes=op.getsize(pat),
               input_s=round(time.perf_counter() - t0, 1))
    print(json.dumps(res), flush=True)
    if args.ref_blocks:
        sec = ref_per_block(text, s, e, args.ref_blocks)
        print(json.dumps(dict(what='reference per-block path, CPU of this host, one process, no tabix', blocks=args.ref_blocks,
                              s_per_block=float('%.4g' % sec), whole_table_h=round(sec * s.size / 3600, 2))), flush=True)
    if args.no_gpu:
        return
    from wgbs_tools_amd import _lib
    CH = 64 << 20
    chunks = []
    pos = 0
    while pos < len(text):
        cut = text.rfind(b'\n', pos, pos + CH) + 1 if pos + CH < len(text) else len(text)
        chunks.append(text[pos:cut])
        pos = cut
    kms, walls = [], []
    for _ in range(args.reps):
        with _lib.Bimodal(s, e) as b:
            t = time.perf_counter()
            for c in chunks:
                b.feed(c)
            ll, cnt = b.finish()
            walls.append(time.perf_counter() - t)
            kms.append(b.kernel_ms())
    km = stats(kms)
    rows_iters = float((cnt[:, 1] * cnt[:, 2]).sum())
    print(json.dumps(dict(what='kernel', kernel_ms=km, rows_x_iters=rows_iters, rows_x_iters_per_s=float('%.4g' % (rows_iters / km['median'] * 1e3)),
                          blocks_with_rows=int((cnt[:, 1] > 0).sum()), max_iters=int(cnt[:, 2].max()), max_cols=int(cnt[:, 0].max()),
                          feed_finish_wall_s=stats(walls))), flush=True)
    g = write_genome_stub(op.join(d, 'genome'))
    parts = {k: [] for k in ('inflate_s', 'feed_s', 'finish_s', 'write_s', 'kernel_ms', 'wall_s')}
    for _ in range(args.reps):
        a = test_bimodal.parse_args([pat, '-L', blocks, '--genome', g, '-o', op.join(d, 'out.txt')])
        t = {}
        t0 = time.perf_counter()
        test_bimodal.multiple_regions(a, t)
        t['wall_s'] = time.perf_counter() - t0
        for k in parts:
            parts[k].append(t[k])
    out = {k: stats(v) for k, v in parts.items()}
    print(json.dumps(dict(what='cli (test_bimodal -L: .pat.gz -> output text)', **out,
                          out_lines=open(op.join(d, 'out.txt')).read().count('\n'),
                          kernel_share_of_wall=round(out['kernel_ms']['median'] / 1e3 / out['wall_s']['median'], 3))), flush=True)


if __name__ == '__main__':
    main()
