#!/usr/bin/env python3
"""BGZF pat files inflated on the GPU against the host path (profiles/pat_inflate_mi355x.txt), one command on one box.

Input: the file of tools/homog_bench.py (28 M CpGs, a segmentation-like block table, a BGZF pat file of --reads sorted reads,
default 10^8).

Reports, as median [min, max] of --reps runs after one warm-up run:
  kernel     k_bgzf_inflate over the whole file fed to a homog engine with feed_bgzf (HIP events around every launch): GB/s of text;
             and the wall time of all feed_bgzf calls + finish from the file's bytes in memory
  cli        homog_process() (.pat.gz -> .uxm.bed.gz) and pat2beta's path (feed_pat + finish + the .beta written) with the host
             inflate and with the device inflate, alternating, same file, same box
  resources  the compiler's report for k_bgzf_inflate (registers, LDS, scratch, waves per SIMD)
The device path counts as faster only where its slowest run is faster than the host path's fastest one; the file says which way it fell.
"""
import argparse
import os
import os.path as op
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tools'))

from homog_bench import N_SITES, blocks_table, pat_piece, stats          # noqa: E402


def fmt(v, unit='s', scale=1.0, digits=3):
    s = stats([x * scale for x in v])
    return '%.*f %s [%.*f, %.*f]' % (digits, s['median'], unit, digits, s['min'], digits, s['max'])


def verdict(host, device):
    if max(device) < min(host):
        return 'device faster: its slowest run (%.3f s) is below the host path\'s fastest (%.3f s); medians %.2fx' % (
            max(device), min(host), stats(host)['median'] / stats(device)['median'])
    if max(host) < min(device):
        return 'host faster: its slowest run (%.3f s) is below the device path\'s fastest (%.3f s)' % (max(host), min(device))
    return 'no difference shown: the ranges overlap'


def resources():
    """the compiler's resource report for k_bgzf_inflate, from a translation unit that holds only that kernel"""
    from wgbs_tools_amd import build
    with tempfile.TemporaryDirectory() as d:
        src = op.join(d, 'k.hip')
        with open(src, 'w') as f:
            f.write('#include "inflate_kernels.h"\n')
        r = subprocess.run([build.hipcc(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '-ffp-contract=off', '--cuda-device-only', '-c',
                            '-I', build.CSRC, '-Rpass-analysis=kernel-resource-usage', src, '-o', op.join(d, 'k.o')], capture_output=True, text=True)
    keep = []
    for line in r.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)', line)
        if m:
            keep.append('%s: %s' % (m.group(1), m.group(2)))
    return keep or ['(no report: hipcc said: %s)' % r.stderr.strip()[-300:]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reads', type=float, default=1e8)
    ap.add_argument('--pieces', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=op.join(ROOT, 'profiles', 'pat_inflate_mi355x.txt'))
    args = ap.parse_args()
    d = args.workdir or tempfile.mkdtemp(prefix='inflate_bench_')
    os.makedirs(d, exist_ok=True)
    try:
        lines = run(args, d)
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)
    os.makedirs(op.dirname(op.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def run(args, d):
    from wgbs_tools_amd import _lib, homog
    from wgbs_tools_amd.beta_to_blocks import load_blocks_file
    from wgbs_tools_amd.pat2beta import feed_pat
    n_reads = int(args.reads)
    s, e, btext = blocks_table(7, N_SITES)
    blocks = op.join(d, 'blocks.bed')
    with open(blocks, 'w') as f:
        f.write(btext)
    step, per = N_SITES // args.pieces, n_reads // args.pieces
    text = b''.join(pat_piece(100 + k, 1 + k * step, 1 + (k + 1) * step, per) for k in range(args.pieces))
    pat = op.join(d, 'bench.pat.gz')
    homog.write_bgzf(pat, text, 16)
    n_text = len(text)
    del text
    data = open(pat, 'rb').read()
    out = ['BGZF pat files inflated on one MI355X against the host path — tools/inflate_bench.py --reads %g --reps %d (median [min, max] of %d runs'
           % (args.reads, args.reps, args.reps), 'after one warm-up run; one command, one box)', '',
           'Input: the file of tools/homog_bench.py: %s CpGs, %s blocks, a BGZF pat file of %s sorted reads: %s bytes of text,'
           % (format(N_SITES, ','), format(int(s.size), ','), format(per * args.pieces, ','), format(n_text, ',')),
           '%s bytes compressed (members of 65280 bytes of text, zlib level 6); -l 3.' % format(len(data), ','), '']
    edges = homog.parse_range(homog.range_text(3))

    # ---- the kernel --------------------------------------------------------------------------------------------------------------
    PIECE = 64 << 20
    ims, kms, walls = [], [], []
    for rep in range(args.reps + 1):
        with _lib.Homog(s, e, edges, 3) as h:
            t = time.perf_counter()
            tail = b''
            for pos in range(0, len(data), PIECE):
                buf = tail + data[pos:pos + PIECE]
                tail = buf[h.feed_bgzf(buf):]
            counts = h.finish()
            wall = time.perf_counter() - t
            assert tail == b''
            if rep:                                                     # (run 0 warms up: allocations, the code object)
                walls.append(wall); ims.append(h.inflate_ms() / 1e3); kms.append(h.kernel_ms() / 1e3)
    with _lib.Homog(s, e, edges, 3) as h:                               # the same counts from the host path
        feed_pat(h, pat, {})
        same = bool(np.array_equal(h.finish(), counts))
    im = stats(ims)
    out += ['kernel  k_bgzf_inflate, one member per wavefront, over the file in calls of 64 MB of compressed bytes (feed_bgzf of a homog engine),',
            '        HIP events around every launch',
            '        %s  ->  %.1f GB/s of text, %.1f GB/s of compressed bytes' % (fmt(ims, 'ms', 1e3, 1), n_text / im['median'] / 1e9, len(data) / im['median'] / 1e9),
            '        k_homog_count behind it over the same device text: %s' % fmt(kms, 'ms', 1e3, 1),
            '        all feed_bgzf calls + finish, from the file\'s bytes in memory: %s' % fmt(walls),
            '        counts equal to the host path\'s: %s' % ('yes' if same else 'NO'), '']

    # ---- the commands ------------------------------------------------------------------------------------------------------------
    class A:
        rlen, inclusive, binary, nr_bits, force, threads, device, inflate = 3, False, False, 8, True, 16, 0, 'host'
    b = load_blocks_file(blocks)
    hw = {'host': [], 'device': []}
    parts = {'host': [], 'device': []}
    for rep in range(args.reps + 1):
        for mode in ('host', 'device'):
            A.inflate = mode
            t = {}
            t0 = time.perf_counter()
            homog.homog_process(pat, b, edges, A, d, None, t)
            t['wall_s'] = time.perf_counter() - t0
            if rep:
                hw[mode].append(t['wall_s']); parts[mode].append(t)
    out += ['cli     homog_process(): the .pat.gz -> <name>.uxm.bed.gz, --inflate host and --inflate device alternating']
    for mode in ('host', 'device'):
        p = parts[mode]
        out += ['        %-6s wall %s   (%s %s, feed %s, finish %s, write %s)' % (
            mode, fmt(hw[mode], 's', 1, 2), 'inflate' if mode == 'host' else 'read', fmt([x['inflate_s'] for x in p], 's', 1, 2),
            fmt([x['feed_s'] for x in p], 's', 1, 2), fmt([x['finish_s'] for x in p], 's', 1, 3), fmt([x['write_s'] for x in p], 's', 1, 2))]
    out += ['        ' + verdict(hw['host'], hw['device']), '']
    pw = {'host': [], 'device': []}
    beta = {}
    for rep in range(args.reps + 1):
        for mode in ('host', 'device'):
            t0 = time.perf_counter()
            with _lib.PatBeta(1, N_SITES + 1) as pb:
                feed_pat(pb, pat, {}, inflate=mode)
                rows = pb.finish()
            rows.tofile(op.join(d, 'bench.%s.beta' % mode))
            if rep:
                pw[mode].append(time.perf_counter() - t0)
            beta[mode] = rows
    out += ['cli     pat2beta\'s path: feed_pat() + finish() + the .beta written (%s bytes), host and device alternating' % format(2 * N_SITES, ',')]
    for mode in ('host', 'device'):
        out += ['        %-6s wall %s' % (mode, fmt(pw[mode], 's', 1, 2))]
    out += ['        ' + verdict(pw['host'], pw['device']), '        the two .beta files are equal: %s' % ('yes' if np.array_equal(beta['host'], beta['device']) else 'NO'), '']
    out += ['resources  k_bgzf_inflate as the compiler reports it (-Rpass-analysis=kernel-resource-usage, gfx950)'] + ['        ' + x for x in resources()]
    return out


if __name__ == '__main__':
    main()
