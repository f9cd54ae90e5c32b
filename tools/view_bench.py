#!/usr/bin/env python3
"""`wgbstools view` on the hg19-shaped synthetic pat file of tools/homog_bench.py and tools/frag_len_bench.py (profiles/view_*.txt).

Input: the same BGZF pat file of --reads reads (default 10^8; reads of 1-12 CpGs, counts 1-40, sorted by start, `chr1` throughout),
read with --inflate device.  Three runs, each --reps times (median [min, max]):
  (a) whole genome, --strip --min_len 3, the text fetched and thrown away (no sort: the file's order is kept)
  (b) one chromosome's worth of sites, [1, --chrom-sites], --strict --strip: sorted
  (c) a region of 5,000 CpGs, --strict --strip: sorted
Per run: the device time of measure + pack over all chunks, of the sort, of collapse + emit and (with --deflate) of the deflate; the
wall time of view.view_pat from the .pat.gz to the last fetched byte; the records kept, the merge passes and whether the sort ran.

For (b) and (c) the same selected lines — the device's own unsorted output, in which only neighbours have been collapsed — go through
`LC_ALL=C sort -k2,2n -k3,3` and a one-pass collapse in Python on this box's CPU; the sha1 of that text is compared with the device's
(every count of this file is positive, so collapsing neighbours first changes no sum)."""
import argparse
import hashlib
import json
import os
import os.path as op
import subprocess
import sys
import tempfile
import time

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tools'))

from homog_bench import N_SITES, pat_piece, stats          # noqa: E402


class Sink:
    """counts and (hash=True) hashes what it is given; keep: also writes it to a file"""

    def __init__(self, hash=False, keep=None):
        self.n, self.h, self.f = 0, hashlib.sha1() if hash else None, open(keep, 'wb') if keep else None

    def __call__(self, piece):
        self.n += len(piece)
        if self.h:
            self.h.update(piece)
        if self.f:
            self.f.write(piece)

    def close(self):
        if self.f:
            self.f.close()
        return self.h.hexdigest() if self.h else None


def collapse_file(src):
    """one pass over sorted pat lines -> sha1 of the collapsed text, its lines"""
    h, lines, key, total = hashlib.sha1(), 0, None, 0
    with open(src, 'rb') as f:
        for line in f:
            k, _, c = line.rpartition(b'\t')
            if k == key:
                total += int(c)
                continue
            if key is not None and total > 0:
                h.update(b'%s\t%d\n' % (key, total))
                lines += 1
            key, total = k, int(c)
    if key is not None and total > 0:
        h.update(b'%s\t%d\n' % (key, total))
        lines += 1
    return h.hexdigest(), lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chrom-sites', type=int, default=2_300_000, help='the sites of run (b): about chr1 of hg19')
    ap.add_argument('--deflate', action='store_true', help='also time every run with the output deflated on the device')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()
    d = args.workdir or tempfile.mkdtemp(prefix='view_bench_')
    os.makedirs(d, exist_ok=True)
    try:
        run(args, d)
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)


def run(args, d):
    from wgbs_tools_amd import homog, view

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    n_reads = int(args.reads)
    t0 = time.perf_counter()
    step, per = N_SITES // args.pieces, n_reads // args.pieces
    text = b''.join(pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces))
    pat = op.join(d, 'bench.pat.gz')
    homog.write_bgzf(pat, text, 16)
    say(dict(n_sites=N_SITES, n_reads=per * args.pieces, text_bytes=len(text), pat_gz_bytes=op.getsize(pat), input_s=round(time.perf_counter() - t0, 1)))
    del text
    mid = N_SITES // 2
    runs = [('a: whole genome, --strip --min_len 3', 1, N_SITES + 1, dict(strip=True, min_len=3, sort=False), False),
            ('b: sites [1, %d), --strict --strip, sorted' % args.chrom_sites, 1, args.chrom_sites, dict(strict=True, strip=True, sort=True), True),
            ('c: 5,000 CpGs, --strict --strip, sorted', mid, mid + 5000, dict(strict=True, strip=True, sort=True), True)]
    for what, s, e, flags, compare in runs:
        device_sha = None
        for deflate in ([False, True] if args.deflate else [False]):
            keys = ('kernel_ms', 'sort_ms', 'emit_ms', 'deflate_ms', 'inflate_ms', 'wall_s')
            parts, sha, info = {k: [] for k in keys}, None, None
            for rep in range(args.reps):
                t, sink = {}, Sink(hash=rep == 0 and not deflate)
                t1 = time.perf_counter()
                lines, nbytes = view.view_pat(pat, s, e, sink, inflate='device', deflate=deflate, timings=t, **flags)
                t['wall_s'] = time.perf_counter() - t1
                assert sink.n == nbytes
                sha = sink.close() or sha
                for k in keys:
                    parts[k].append(t.get(k, 0.0))
                info = dict(lines=lines, out_bytes=nbytes, records=t['records'], arena_bytes=t['arena_bytes'], merge_passes=t['merge_passes'],
                            order=t['order'], grown_records=t['grown_records'], grown_arena=t['grown_arena'])
            device_sha = device_sha or sha
            say(dict(what=what, deflate=deflate, sha1=sha, **info, **{k: stats(v) for k, v in parts.items()}))
        if compare:
            raw, srt = op.join(d, 'selected.pat'), op.join(d, 'sorted.pat')
            sink = Sink(keep=raw)
            view.view_pat(pat, s, e, sink, inflate='device', **dict(flags, sort=False))
            sink.close()
            t1 = time.perf_counter()
            with open(srt, 'wb') as f:
                subprocess.check_call(['sort', '-k2,2n', '-k3,3', raw], stdout=f, env=dict(os.environ, LC_ALL='C'))
            t2 = time.perf_counter()
            cpu_sha, cpu_lines = collapse_file(srt)
            t3 = time.perf_counter()
            say(dict(what=what + ' — on the CPU: sort -k2,2n -k3,3, then a one-pass collapse in Python', selected_lines_bytes=op.getsize(raw),
                     sort_s=round(t2 - t1, 3), collapse_s=round(t3 - t2, 3), lines=cpu_lines, sha1=cpu_sha, equals_device=cpu_sha == device_sha))
            os.remove(raw)
            os.remove(srt)


if __name__ == '__main__':
    main()
