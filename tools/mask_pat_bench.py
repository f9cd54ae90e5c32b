#!/usr/bin/env python3
"""`wgbstools mask_pat` on the hg19-shaped synthetic pat file of tools/view_bench.py (profiles/mask_pat_*.txt).

Input: the same BGZF pat file of --reads reads (default 10^8; reads of 1-12 CpGs, counts 1-40, sorted by start, `chr1` throughout),
read with --inflate device.  Runs, each --reps times (median [min, max]), all in this one process:
  (a)  view_bench's run (a): whole genome, --strip --min_len 3, no sort, no mask — the unmasked k_view_measure / k_view_pack, to be held
       against profiles/view_mi355x.txt
  (u)  whole genome with mask_pat's flags (STRIP | SORT, min_len 1, the output deflated on the device) and NO mask
  (m)  the same with a mask of 10^3, 10^6 and 5 x 10^6 blocks of 1-3 sites at hashed places of the genome
Per run: the device time of k_view_mask_fill, of measure + pack over all chunks, of the sort, of collapse + emit and of the deflate; the
wall time of view.view_pats from the .pat.gz to the last fetched byte; the records kept, the merge passes, the hidden sites.

On this box's CPU, for the sites [1, --chrom-sites) and the 10^6-block mask: the device's own selection (no mask, no strip, no sort)
goes through an awk program that hides the sites and strips the dots, `LC_ALL=C sort -k2,2n -k3,3` and a one-pass collapse in Python;
the sha1 of that text is compared with the device's masked output over the same interval."""
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

from homog_bench import N_SITES, pat_piece, stats          # noqa: E402
from view_bench import Sink, collapse_file                 # noqa: E402

# hides the sites of the blocks file (first argument: "start end" lines) in the pat lines on stdin, strips the dots at both ends
AWK = r'''
BEGIN { FS = "\t"; OFS = "\t"; while ((getline line < blocks) > 0) { split(line, b, " "); for (s = b[1]; s < b[2]; s++) H[s] = 1 } }
{
    n = length($3); out = "";
    for (i = 1; i <= n; i++) { c = substr($3, i, 1); out = out (($2 + i - 1) in H ? "." : c) }
    while (n > 0 && substr(out, n, 1) == ".") n--;
    if (n == 0) next;
    a = 1; while (substr(out, a, 1) == ".") a++;
    print $1, $2 + a - 1, substr(out, a, n - a + 1), $4
}
'''


def mask_blocks(n_blocks, seed=7):
    rng = np.random.default_rng(seed)
    s = rng.integers(1, N_SITES, n_blocks)
    return s, s + rng.integers(1, 4, n_blocks)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--blocks', type=float, nargs='+', default=[1e3, 1e6, 5e6])
    ap.add_argument('--chrom-sites', type=int, default=2_300_000, help='the sites of the comparison on the CPU: about chr1 of hg19')
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()
    d = args.workdir or tempfile.mkdtemp(prefix='mask_bench_')
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

    def timed(what, s, e, mask, deflate, hash_first=False, **flags):
        keys = ('mask_ms', 'kernel_ms', 'sort_ms', 'emit_ms', 'deflate_ms', 'inflate_ms', 'wall_s')
        parts, sha, info = {k: [] for k in keys}, None, None
        for rep in range(args.reps):
            t, sink = {}, Sink(hash=hash_first and rep == 0)
            t1 = time.perf_counter()
            lines, nbytes = view.view_pats([pat], s, e, sink, inflate='device', deflate=deflate, timings=t, mask=mask, **flags)
            t['wall_s'] = time.perf_counter() - t1
            assert sink.n == nbytes
            sha = sink.close() or sha
            for k in keys:
                parts[k].append(t.get(k, 0.0))
            info = dict(lines=lines, out_bytes=nbytes, records=t['records'], arena_bytes=t['arena_bytes'], merge_passes=t['merge_passes'], order=t['order'],
                        hidden_sites=t.get('hidden_sites', 0), mask_words=t.get('mask_words', 0))
        say(dict(what=what, deflate=deflate, sha1=sha, **info, **{k: stats(v) for k, v in parts.items()}))
        return sha

    timed('a: whole genome, --strip --min_len 3, no sort, no mask', 1, N_SITES + 1, None, False, strip=True, min_len=3, sort=False)
    timed('u: whole genome, strip + sort, min_len 1, deflated, no mask', 1, N_SITES + 1, None, True, strip=True, sort=True)
    masks = {}
    for nb in args.blocks:
        masks[int(nb)] = mask_blocks(int(nb))
        timed('m: whole genome, strip + sort, min_len 1, deflated, a mask of %d blocks' % int(nb), 1, N_SITES + 1, masks[int(nb)], True, strip=True, sort=True)

    # ---- the same masked text on the CPU, over one chromosome's worth of sites
    nb = int(args.blocks[len(args.blocks) // 2])
    starts, ends = masks[nb]
    e = args.chrom_sites
    device_sha = timed('c: sites [1, %d), strip + sort, a mask of %d blocks, plain text' % (e, nb), 1, e, (starts, ends), False, hash_first=True, strip=True, sort=True)
    raw, blocks, masked, srt = (op.join(d, n) for n in ('selected.pat', 'blocks.txt', 'masked.pat', 'sorted.pat'))
    sink = Sink(keep=raw)
    view.view_pats([pat], 1, e, sink, inflate='device', sort=False)
    sink.close()
    with open(blocks, 'w') as f:                                       # (the blocks that can reach a selected read)
        f.write(''.join('%d %d\n' % (a, b) for a, b in zip(starts.tolist(), ends.tolist()) if a < e + 64))
    env = dict(os.environ, LC_ALL='C')
    t1 = time.perf_counter()
    with open(raw, 'rb') as fin, open(masked, 'wb') as fout:
        subprocess.check_call(['awk', '-v', 'blocks=' + blocks, AWK], stdin=fin, stdout=fout, env=env)
    t2 = time.perf_counter()
    with open(srt, 'wb') as f:
        subprocess.check_call(['sort', '-k2,2n', '-k3,3', masked], stdout=f, env=env)
    t3 = time.perf_counter()
    cpu_sha, cpu_lines = collapse_file(srt)
    t4 = time.perf_counter()
    say(dict(what='c on the CPU: awk mask + strip, sort -k2,2n -k3,3, a one-pass collapse in Python', selected_bytes=op.getsize(raw), awk_s=round(t2 - t1, 3),
             sort_s=round(t3 - t2, 3), collapse_s=round(t4 - t3, 3), lines=cpu_lines, sha1=cpu_sha, equals_device=cpu_sha == device_sha))
    for p in (raw, blocks, masked, srt):
        os.remove(p)


if __name__ == '__main__':
    main()
