#!/usr/bin/env python3
"""BGZF output deflated on the GPU against the host paths (profiles/bgzf_deflate_mi355x.txt), one command on one box.

Reports, as median [min, max] of --reps runs after one warm-up run:
  kernel     k_bgzf_deflate and k_bgzf_pack (with the scan between) inside wgbsseg_beta2bed_bgzf over the 28 M-site synthetic sample of
             tools/beta2bed_bench.py (HIP events around the launches, summed over the slabs): bytes of text per second
  beta2bed   the whole call writing x.bed.gz: --deflate device (wgbsseg_beta2bed_bgzf straight to the file) and --deflate host (the text
             through a pipe into gzip.GzipFile, level 9, one thread), the latter over the first --host-fraction of the sites
  homog      homog_process() (.pat.gz -> .uxm.bed.gz) with --deflate host (zlib level 6 on -@ 16 threads) and --deflate device,
             alternating, on the block table of tools/inflate_bench.py's file and a pat file of --reads reads (the output's size depends
             on the blocks only)
  size       the device's members against zlib level 1, 6 and 9 over the same cut of the first --size-mb MB of the BED text
  resources  the compiler's report for k_bgzf_deflate and k_bgzf_pack
"""
import argparse
import gzip
import os
import os.path as op
import re
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tools'))

from beta2bed_bench import N_SITES, SEED, device_rows          # noqa: E402
from homog_bench import blocks_table, pat_piece, stats          # noqa: E402
from inflate_bench import fmt, verdict                          # noqa: E402


def resources():
    from wgbs_tools_amd import build
    with tempfile.TemporaryDirectory() as d:
        src = op.join(d, 'k.hip')
        with open(src, 'w') as f:
            f.write('#include "bed_kernels.h"\n#include "deflate_kernels.h"\n')
        r = subprocess.run([build.hipcc(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '-ffp-contract=off', '--cuda-device-only', '-c',
                            '-I', build.CSRC, '-Rpass-analysis=kernel-resource-usage', src, '-o', op.join(d, 'k.o')], capture_output=True, text=True)
    keep, on = [], False
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)', line)
        if m:
            if m.group(1) == 'Function Name':
                on = 'bgzf' in m.group(2)
            if on:
                keep.append('%s: %s' % (m.group(1), m.group(2)))
    return keep or ['(no report: hipcc said: %s)' % r.stderr.strip()[-300:]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=N_SITES)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-fraction', type=float, default=0.1)
    ap.add_argument('--size-mb', type=int, default=32)
    ap.add_argument('--reads', type=float, default=1e7)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--no-homog', action='store_true')
    ap.add_argument('--out', default=op.join(ROOT, 'profiles', 'bgzf_deflate_mi355x.txt'))
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix='deflate_bench_')
    try:
        lines = run(args, d)
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(op.dirname(op.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def run(args, d):
    from wgbs_tools_amd import _lib, beta2bed, homog, synth
    n = args.sites
    names, sizes = synth.genome_shape(n)
    loci = synth.synth_loci(SEED, sizes)
    cum = np.cumsum(sizes)
    buf, pitch = device_rows(n)
    out = ['BGZF output deflated on one MI355X against the host paths — tools/deflate_bench.py --sites %d --reps %d (median [min, max] of %d runs'
           % (n, args.reps, args.reps), 'after one warm-up run; one command, one box)', '']
    with _lib.Segmenter(0) as seg:
        seg.set_betas_device(buf.data_ptr(), 1, pitch, n, keepalive=buf)
        seg.set_loci(loci)

        def call(path, sink=None, **kw):
            fd = sink.fd if sink else os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            t0 = time.perf_counter()
            try:
                got = seg.beta2bed(fd, 0, names, cum, **kw)
            finally:
                sink.close() if sink else os.close(fd)
            return got, time.perf_counter() - t0

        # ---- the kernels and the device command ------------------------------------------------------------------------------------
        gz = op.join(d, 'x.bed.gz')
        walls, dms, pms, ems = [], [], [], []
        for rep in range(args.reps + 1):
            (n_lines, n_out, n_text), wall = call(gz, bgzf=True)
            if rep:
                walls.append(wall)
                a, b = seg.bgzf_deflate_ms()
                dms.append(a / 1e3); pms.append(b / 1e3); ems.append(sum(seg.beta2bed_pass_ms()) / 1e3)
        assert op.getsize(gz) == n_out
        dm, pm = stats(dms), stats(pms)
        members = sum(1 for _ in range(0, n_text, 65280))
        out += ['Input: the sample of tools/beta2bed_bench.py: %s sites, %s lines, %s bytes of text; %s bytes of BGZF (%.3f of the text), the default slab.'
                % (format(n, ','), format(n_lines, ','), format(n_text, ','), format(n_out, ','), n_out / n_text), '',
                'kernel    k_bgzf_deflate, one member (65280 bytes of text) per wavefront, 3 per workgroup, behind every slab\'s emit pass',
                '          %s  ->  %.2f GB/s of text (about %s members)' % (fmt(dms, 'ms', 1e3, 1), n_text / dm['median'] / 1e9, format(members, ',')),
                'pack      k_bed_scan over the sizes + k_bgzf_pack, one workgroup per member',
                '          %s  ->  %.1f GB/s of compressed bytes' % (fmt(pms, 'ms', 1e3, 2), n_out / pm['median'] / 1e9),
                '          (the length, scan and emit passes in front: %s)' % fmt(ems, 'ms', 1e3, 1), '',
                'beta2bed  the whole call (rows resident) writing x.bed.gz',
                '          --deflate device  %s  (all %s sites)' % (fmt(walls, 's', 1, 3), format(n, ','))]
        # the parent commit's path: the text through a pipe into gzip.GzipFile (level 9) on one thread
        part = max(1, int(n * args.host_fraction))
        hz = op.join(d, 'h.bed.gz')
        hwalls = []
        for rep in range(2):
            (h_lines, h_text), wall = call(hz, sink=beta2bed._GzipSink(hz), end0=part)
            hwalls.append(wall)
        (p_lines, p_out, p_text), pwall = call(gz, bgzf=True, end0=part)
        assert (p_lines, p_text) == (h_lines, h_text)
        with gzip.open(hz, 'rb') as fa, gzip.open(gz, 'rb') as fb:
            same = fa.read() == fb.read()
        out += ['          --deflate host    %.1f s, %.1f s  (two runs over the first %s sites only, %.0f %% of them: %s bytes of text -> %s bytes; %.1f MB/s of text)'
                % (hwalls[0], hwalls[1], format(part, ','), 100.0 * part / n, format(h_text, ','), format(op.getsize(hz), ','), h_text / min(hwalls) / 1e6),
                '          --deflate device  %.3f s over the same sites -> %s bytes; both files inflate to the same text: %s' % (pwall, format(p_out, ','), 'yes' if same else 'NO'),
                '          at the host path\'s rate the whole sample would take about %.0f s (an extrapolation)' % (min(hwalls) * n_text / h_text), '']

        # ---- the size ---------------------------------------------------------------------------------------------------------------------
        plain = op.join(d, 'p.bed')
        few = max(1, int(n * (args.size_mb << 20) / n_text))
        call(plain, end0=few)
        text = open(plain, 'rb').read()
    t0 = time.perf_counter()
    ours = _lib.bgzf_deflate(text, eof=False)
    t_dev = time.perf_counter() - t0
    assert _lib.bgzf_inflate(ours) == (text, len(ours))
    pieces = [text[p:p + 65280] for p in range(0, len(text), 65280)]
    out += ['size      the first %s sites: %s bytes of text in %s members; payload + 26 bytes of framing per member' % (format(few, ','), format(len(text), ','), format(len(pieces), ',')),
            '          device (wgbsseg_bgzf_deflate, %.3f s with both copies)  %s bytes  %.4f of the text' % (t_dev, format(len(ours), ','), len(ours) / len(text))]
    for level in (1, 6, 9):
        t0 = time.perf_counter()
        total = 0
        for p in pieces:
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            total += len(c.compress(p)) + len(c.flush()) + 26
        dt = time.perf_counter() - t0
        out += ['          zlib level %d, one thread, %.1f s (%.1f MB/s)  %s bytes  %.4f of the text  (device / zlib: %.3f)'
                % (level, dt, len(text) / dt / 1e6, format(total, ','), total / len(text), len(ours) / total)]
    out += ['']
    del text, pieces

    # ---- homog ------------------------------------------------------------------------------------------------------------------------
    if not args.no_homog:
        from wgbs_tools_amd.beta_to_blocks import load_blocks_file
        n_reads = int(args.reads)
        s, e, btext = blocks_table(7, N_SITES)
        blocks = op.join(d, 'blocks.bed')
        with open(blocks, 'w') as f:
            f.write(btext)
        step, per = N_SITES // args.pieces, n_reads // args.pieces
        pat = op.join(d, 'bench.pat.gz')
        homog.write_bgzf(pat, b''.join(pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces)), 16)
        edges = homog.parse_range(homog.range_text(3))

        class A:
            rlen, inclusive, binary, nr_bits, force, threads, device, inflate, deflate = 3, False, False, 8, True, 16, 0, 'device', 'host'
        b = load_blocks_file(blocks)
        hw, ws, texts = {'host': [], 'device': []}, {'host': [], 'device': []}, {}
        for rep in range(args.reps + 1):
            for mode in ('host', 'device'):
                A.deflate = mode
                t = {}
                t0 = time.perf_counter()
                path = homog.homog_process(pat, b, edges, A, d, op.join(d, mode), t)
                wall = time.perf_counter() - t0
                if rep:
                    hw[mode].append(wall); ws[mode].append(t['write_s'])
                elif mode not in texts:
                    texts[mode] = (gzip.open(path, 'rb').read(), op.getsize(path))
        out += ['homog     homog_process(): .pat.gz -> .uxm.bed.gz, %s blocks (the table of tools/inflate_bench.py\'s file), a pat file of %s reads, --inflate device;'
                % (format(int(s.size), ','), format(per * args.pieces, ',')),
                '          the output is %s bytes of text; --deflate host (zlib level 6, -@ 16) and --deflate device alternating' % format(len(texts['host'][0]), ',')]
        for mode in ('host', 'device'):
            out += ['          %-6s wall %s   (of it the table\'s text and the .gz written: %s)  %s bytes' % (mode, fmt(hw[mode], 's', 1, 2), fmt(ws[mode], 's', 1, 2), format(texts[mode][1], ','))]
        out += ['          ' + verdict(hw['host'], hw['device']), '          the two files inflate to the same text: %s' % ('yes' if texts['host'][0] == texts['device'][0] else 'NO'), '']
    out += ['resources  k_bgzf_deflate and k_bgzf_pack as the compiler reports them (-Rpass-analysis=kernel-resource-usage, gfx950)'] + ['          ' + x for x in resources()]
    return out


if __name__ == '__main__':
    main()
