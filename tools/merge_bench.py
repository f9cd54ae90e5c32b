#!/usr/bin/env python3
"""`wgbstools merge` on the hg19-shaped synthetic inputs of the other profiles (profiles/merge_*.txt).

Pat merge.  Input: the BGZF pat file of tools/view_bench.py (--reads reads, default 10^8; reads of 1-12 CpGs, counts 1-40, sorted by start,
`chr1` throughout) and three copies of it whose counts are shifted (the last digit d of every count becomes 1 + (d - 1 + k) mod 9 in
copy k: the same reads, other counts, none below 1).  Two and four files; the whole genome and one chromosome's worth of sites,
[1, --chrom-sites); each --reps times (median [min, max]) through view.view_pats with --inflate device and the output deflated on the
device, as merge.merge_pats runs it.  Per run: the device time of the feed (measure + pack over all chunks), of the inflate, the sort,
collapse + emit and the deflate, and the wall time from the .pat.gz files to the last fetched byte.
With --cpu the same box's CPU does what the reference pipes: every file's selected lines (the device's own unsorted output of that file
alone) through `LC_ALL=C sort -k2,2n -k3,3`, then `sort -m -k2,2n -k3,3` over the files and a one-pass collapse restated here in
Python; the sha1 of that text is compared with the device's.

Beta merge.  Rows: --sites sites (default 28,217,448) x 2, 8 and 32 samples of uint8 pairs, filled on the device and handed over by
pointer; wgbsseg_merge_rows --reps times: the kernel's HIP-event time, its bytes (rows read + one row written) per second, beside the
8.0 TB/s peak and the 6.29 TB/s float4 copy measured on this chip (MI355X_MICROARCH.md).  numpy's restatement of merge_betas /
trim_to_uint8 is timed on the same box over the same rows and compared with the device's result."""
import argparse
import hashlib
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
sys.path.insert(0, op.join(ROOT, 'tools'))
sys.path.insert(0, op.join(ROOT, 'tests'))

from homog_bench import N_SITES, pat_piece, stats          # noqa: E402
from view_bench import Sink, collapse_file                  # noqa: E402

HBM_PEAK_TB_S, HBM_COPY_TB_S = 8.0, 6.29


def shifted(text, k):
    """copy k of the text: the last digit d of every count -> 1 + (d - 1 + k) mod 9"""
    buf = np.frombuffer(text, dtype=np.uint8).copy()
    at = np.flatnonzero(buf == 10) - 1
    d = buf[at].astype(np.int64) - 48
    buf[at] = (49 + (d - 1 + k) % 9).astype(np.uint8)
    return buf.tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--files', type=int, nargs='+', default=[2, 4])
    ap.add_argument('--chrom-sites', type=int, default=2_300_000, help='the sites of the one-chromosome run: about chr1 of hg19')
    ap.add_argument('--cpu', action='store_true', help='also time sort, sort -m and a collapse on this box\'s CPU and compare the texts')
    ap.add_argument('--sites', type=int, default=N_SITES, help='sites of the beta rows')
    ap.add_argument('--rows', type=int, nargs='+', default=[2, 8, 32])
    ap.add_argument('--skip-pat', action='store_true')
    ap.add_argument('--skip-beta', action='store_true')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    d = args.workdir or tempfile.mkdtemp(prefix='merge_bench_')
    os.makedirs(d, exist_ok=True)
    try:
        if not args.skip_pat:
            pat_runs(args, d, say)
        if not args.skip_beta:
            beta_runs(args, say)
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)


def pat_runs(args, d, say):
    from wgbs_tools_amd import homog, view
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
    keys = ('kernel_ms', 'inflate_ms', 'sort_ms', 'emit_ms', 'deflate_ms', 'wall_s')
    for what, s, e in (('whole genome', 1, N_SITES + 1), ('sites [1, %d)' % args.chrom_sites, 1, args.chrom_sites)):
        for n in args.files:
            sink = Sink(hash=True)
            view.view_pats(paths[:n], s, e, sink, sort=True, inflate='device')         # the plain text once: its sha1 (and the warm-up)
            plain_bytes, device_sha = sink.n, sink.close()
            parts, info = {k: [] for k in keys}, None
            for _ in range(args.reps):
                t, sink = {}, Sink()
                t1 = time.perf_counter()
                lines, nbytes = view.view_pats(paths[:n], s, e, sink, sort=True, inflate='device', deflate=True, timings=t)
                t['wall_s'] = time.perf_counter() - t1
                assert sink.n == nbytes
                for k in keys:
                    parts[k].append(t.get(k, 0.0))
                info = dict(lines=lines, bgzf_bytes=nbytes, text_bytes=plain_bytes, records=t['records'], merge_passes=t['merge_passes'], order=t['order'])
            say(dict(what='pat merge, %s, %d files, --inflate device, deflated on the device' % (what, n), sha1_of_text=device_sha, **info,
                     **{k: stats(v) for k, v in parts.items()}))
            if not args.cpu:
                continue
            raws, t_sort = [], 0.0
            for k in range(n):
                raw, srt = op.join(d, 'sel%d.pat' % k), op.join(d, 'sorted%d.pat' % k)
                sink = Sink(keep=raw)
                view.view_pats([paths[k]], s, e, sink, sort=False, inflate='device')
                sink.close()
                t1 = time.perf_counter()
                with open(srt, 'wb') as f:
                    subprocess.check_call(['sort', '-k2,2n', '-k3,3', raw], stdout=f, env=dict(os.environ, LC_ALL='C'))
                t_sort += time.perf_counter() - t1
                os.remove(raw)
                raws.append(srt)
            merged = op.join(d, 'merged.pat')
            t1 = time.perf_counter()
            with open(merged, 'wb') as f:
                subprocess.check_call(['sort', '-m', '-k2,2n', '-k3,3'] + raws, stdout=f, env=dict(os.environ, LC_ALL='C'))
            t2 = time.perf_counter()
            cpu_sha, cpu_lines = collapse_file(merged)
            t3 = time.perf_counter()
            say(dict(what='pat merge, %s, %d files — on the CPU: sort -k2,2n -k3,3 per file, sort -m, then a one-pass collapse in Python' % (what, n),
                     sort_per_file_s=round(t_sort, 3), sort_m_s=round(t2 - t1, 3), collapse_s=round(t3 - t2, 3), lines=cpu_lines, sha1=cpu_sha,
                     equals_device=cpu_sha == device_sha))
            for p in raws + [merged]:
                os.remove(p)


def beta_runs(args, say):
    import merge_ref as MR
    from stats_bench import device_rows
    from wgbs_tools_amd import _lib
    for n in args.rows:
        buf, pitch = device_rows(args.sites, n)
        with _lib.Segmenter(0) as seg:
            seg.set_betas_device(buf.data_ptr(), n, pitch, args.sites, keepalive=buf)
            for lbeta in (False, True):
                first = seg.merge_rows(list(range(n)), lbeta=lbeta)              # warm-up (allocations, code load)
                ms, wall = [], []
                for _ in range(args.reps):
                    t1 = time.perf_counter()
                    again = seg.merge_rows(list(range(n)), lbeta=lbeta)
                    wall.append(time.perf_counter() - t1)
                    ms.append(seg.last_merge_rows_ms())
                assert again.tobytes() == first.tobytes()
                nbytes = 2 * args.sites * n + first.nbytes
                med = stats(ms)['median']
                rows = [buf[s, :2 * args.sites].cpu().numpy().reshape(-1, 2) for s in range(n)]
                t1 = time.perf_counter()
                want = MR.merge_betas(rows, lbeta=lbeta)
                t_np = time.perf_counter() - t1
                say(dict(what='beta merge, %d rows of %d sites, %s out' % (n, args.sites, 'uint16' if lbeta else 'uint8'), kernel_ms=stats(ms),
                         bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3), of_hbm_peak=round(nbytes / med / 1e9 / HBM_PEAK_TB_S, 3),
                         of_measured_copy=round(nbytes / med / 1e9 / HBM_COPY_TB_S, 3), call_wall_s=stats(wall), saturated_sites=int((want[:, 1] == (65535 if lbeta else 255)).sum()),
                         numpy_s=round(t_np, 3), equals_numpy=bool(np.array_equal(first, want)), sha1=hashlib.sha1(first.tobytes()).hexdigest()))
        del buf


if __name__ == '__main__':
    main()
