#!/usr/bin/env python3
"""`wgbstools homog` on an hg19-shaped synthetic run (profiles/homog_*.txt).

Input: 28 M CpGs, blocks from a segmentation-like partition (synthetic, ~3.5 M rows), a BGZF pat file of --reads reads
(default 10^8; reads of 1-12 CpGs, counts 1-40, sorted by start — the distribution of bench.synth_pat_text, generated in
pieces of disjoint site ranges so that the whole file stays sorted).

Reports, as median [min, max] of --reps runs:
  kernel   k_homog_count alone over the decompressed text fed in 64 MB chunks (HIP events): GB/s of text, reads/s
  cli      `wgbstools homog` from the .pat.gz to the .uxm.bed.gz, split into inflate (host, BGZF on a thread pool), feed
           (page-locked copy + launch, waiting for a staging buffer), finish (the last kernel + the counts) and write
           (merge, text, BGZF compression)
--ref EXE: also time the reference's homog binary (`gunzip -c x.pat.gz | EXE -b blocks -r ... -l 3`) on the first
           --ref-reads reads of the same text, on this host's CPU (single-threaded, as the reference runs).
"""
import argparse
import json
import os
import os.path as op
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)

from wgbs_tools_amd.synth import hash_at          # noqa: E402

N_SITES = 28_217_448


def pat_piece(seed, a, b, n_reads):
    """pat text of n_reads reads starting in CpGs [a, b), sorted; `chr1` throughout (homog ignores the chromosome)"""
    idx = np.arange(n_reads, dtype=np.int64)
    start = np.sort((hash_at(seed, 91, idx) % np.uint64(b - a)).astype(np.int64) + a)
    h1 = hash_at(seed, 92, idx)
    ln = 1 + ((h1 & np.uint64(15)).astype(np.int64) % 12)
    cnt = 1 + ((h1 >> np.uint64(8)) % np.uint64(40)).astype(np.int64)
    hp = hash_at(seed, 93, idx)
    ds = np.floor(np.log10(start)).astype(np.int64) + 1
    dc = 1 + (cnt >= 10)
    size = 5 + ds + 1 + ln + 1 + dc + 1
    off = np.concatenate([[0], np.cumsum(size)])
    buf = np.empty(int(off[-1]), dtype=np.uint8)
    o = off[:-1]
    for k, ch in enumerate(b'chr1\t'):
        buf[o + k] = ch
    for k in range(int(ds.max())):
        m = ds > k
        buf[o[m] + 5 + ds[m] - 1 - k] = 48 + (start[m] // 10 ** k) % 10
    buf[o + 5 + ds] = 9
    alphabet = np.frombuffer(b'CCCTTTH.', dtype=np.uint8)
    po = o + 6 + ds
    for k in range(12):
        m = ln > k
        buf[po[m] + k] = alphabet[((hp[m] >> np.uint64(3 * k)) & np.uint64(7)).astype(np.int64)]
    buf[po + ln] = 9
    co = po + ln + 1
    two = dc == 2
    buf[co[two]] = 48 + cnt[two] // 10
    buf[co + dc - 1] = 48 + cnt % 10
    buf[co + dc] = 10
    return buf.tobytes()


def blocks_table(seed, n_sites):
    """a partition of CpGs into blocks of 1..12 sites, every fifth dropped -> (start, end) and the table's text"""
    n = n_sites // 4 + 16
    ln = 1 + (hash_at(seed, 11, np.arange(n, dtype=np.int64)) % np.uint64(12)).astype(np.int64)
    ends = 1 + np.cumsum(ln)
    starts = ends - ln
    keep = (ends <= n_sites + 1) & ((hash_at(seed, 12, np.arange(n, dtype=np.int64)) % np.uint64(5)) != 0)
    s, e = starts[keep], ends[keep]
    lines = np.char.add(np.char.add(np.char.add('chr1\t', (s * 40).astype(str)), '\t'),
                        np.char.add(np.char.add((e * 40).astype(str), '\t'), np.char.add(np.char.add(s.astype(str), '\t'), e.astype(str))))
    return s, e, '\n'.join(lines.tolist()) + '\n'


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--ref', default=None, help='the reference homog binary (CPU timing)')
    ap.add_argument('--ref-reads', type=float, default=1e7)
    ap.add_argument('--no-gpu', action='store_true', help='only build the input (and time --ref)')
    args = ap.parse_args()
    from wgbs_tools_amd import homog
    d = args.workdir or tempfile.mkdtemp(prefix='homog_bench_')
    os.makedirs(d, exist_ok=True)
    try:
        run(args, d)
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)


def run(args, d):
    from wgbs_tools_amd import homog
    n_reads = int(args.reads)
    t0 = time.perf_counter()
    s, e, btext = blocks_table(7, N_SITES)
    blocks = op.join(d, 'blocks.bed')
    with open(blocks, 'w') as f:
        f.write(btext)
    step = N_SITES // args.pieces
    per = n_reads // args.pieces
    parts = [pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces)]
    text = b''.join(parts)
    del parts
    pat = op.join(d, 'bench.pat.gz')
    homog.write_bgzf(pat, text, 16)
    res = dict(n_sites=N_SITES, n_blocks=int(s.size), n_reads=per * args.pieces, text_bytes=len(text), pat_gz_bytes=op.getsize(pat),
               input_s=round(time.perf_counter() - t0, 1))
    print(json.dumps(res), flush=True)
    if args.ref:
        k = int(args.ref_reads) // per if per else 0
        sub = text[:text.find(b'\n', 0) + 1] if k == 0 else b''.join(pat_piece(100 + i, 1 + i * step, 1 + (i + 1) * step, per) for i in range(k))
        rng = homog.range_text(3)
        times = []
        for _ in range(max(1, min(3, args.reps))):
            t = time.perf_counter()
            p = subprocess.run([args.ref, '-b', blocks, '-r', rng, '-l', '3', '-n', 'bench'], input=sub, stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, check=True)
            times.append(time.perf_counter() - t)
        r = dict(what='reference homog binary, CPU of the build host, single thread, text on stdin (no gunzip)',
                 reads=sub.count(b'\n'), text_bytes=len(sub), s=stats(times), out_rows=p.stdout.count(b'\n'),
                 mb_per_s=round(len(sub) / stats(times)['median'] / 1e6, 1))
        print(json.dumps(r), flush=True)
    if args.no_gpu:
        return
    from wgbs_tools_amd import _lib
    from wgbs_tools_amd.beta_to_blocks import load_blocks_file
    edges = homog.parse_range(homog.range_text(3))
    CH = 64 << 20
    chunks = []
    pos = 0
    while pos < len(text):
        cut = text.rfind(b'\n', pos, pos + CH) + 1 if pos + CH < len(text) else len(text)
        chunks.append(text[pos:cut])
        pos = cut
    kms, walls = [], []
    for _ in range(args.reps):
        with _lib.Homog(s, e, edges, 3) as h:
            t = time.perf_counter()
            for c in chunks:
                h.feed(c)
            counts = h.finish()
            walls.append(time.perf_counter() - t)
            kms.append(h.kernel_ms())
    km = stats(kms)
    print(json.dumps(dict(what='kernel', kernel_ms=km, text_GB_per_s=round(len(text) / km['median'] / 1e6, 1),
                          reads_per_s=float('%.4g' % (res['n_reads'] / km['median'] * 1e3)), feed_finish_wall_s=stats(walls),
                          counted=int(counts.astype(np.int64).sum()))), flush=True)

    class A:
        rlen, inclusive, binary, nr_bits, force, threads, device = 3, False, False, 8, True, 16, 0
    b = load_blocks_file(blocks)
    parts = {k: [] for k in ('inflate_s', 'feed_s', 'finish_s', 'write_s', 'kernel_ms', 'wall_s')}
    for _ in range(args.reps):
        t = {}
        t0 = time.perf_counter()
        homog.homog_process(pat, b, edges, A, d, None, t)
        t['wall_s'] = time.perf_counter() - t0
        for k in parts:
            parts[k].append(t[k])
    out = {k: stats(v) for k, v in parts.items()}
    print(json.dumps(dict(what='cli (homog_process: .pat.gz -> .uxm.bed.gz)', **out,
                          kernel_share_of_wall=round(out['kernel_ms']['median'] / 1e3 / out['wall_s']['median'], 3),
                          text_MB_per_s=round(len(text) / out['wall_s']['median'] / 1e6, 1))), flush=True)


if __name__ == '__main__':
    main()
