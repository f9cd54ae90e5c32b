#!/usr/bin/env python3
"""`wgbstools init_genome` on the hg19-shaped FASTA of tools/make_fasta.py (profiles/init_genome_mi355x.txt).

Steps, every one a process of its own under its own `timeout -k 10`, chained with && (without --step: all of them):
    make        the FASTA (25 chromosomes, --sites CpGs, lines of 60 bases) and the same text as BGZF
    run plain   the whole call (init_genome.build_dictionary: the file, which is in the page cache, to the written CpG.bed.gz, size files
    run bgzf    and loci.u32) --reps times after a warm-up, median [min, max]: the wall time, the scan kernels' device time (HIP events,
                summed over the chunks) and the text bytes per second of it, the gather, emit and deflate of the finish; bgzf runs with
                --inflate device.  The loci that come out are compared with the ones the FASTA was laid out from.
    copy        the host-to-device copy of as many bytes as the text has, 64 MiB at a time from a page-locked buffer: bytes per second,
                the yardstick to hold beside the kernels' rate — below it, the call waits for the kernels
    cpu         the tests' restatement of the reference's route (strip, join, upper, re.finditer) over the first chromosome's record on
                this machine's CPU: NOT the reference's route itself (no samtools, no pandas frame, no bgzip)
Every step prints JSON lines (and appends them to --out)."""
import argparse
import json
import os
import os.path as op
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tools'))
sys.path.insert(0, op.join(ROOT, 'tests'))

LIMITS = dict(make=500, run=420, copy=120, cpu=300)                 # seconds a step may take


def spread(v, digits=4):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def step_make(args, say):
    import make_fasta
    t0 = time.time()
    r = make_fasta.make_fasta(op.join(args.workdir, 'g.fa'), args.sites, bgzf=op.join(args.workdir, 'g.fa.gz'))
    r['loci'].tofile(op.join(args.workdir, 'want.u32'))
    say(dict(step='make', chromosomes=len(r['names']), sites=int(r['loci'].size), text_bytes=r['text_bytes'], bgzf_bytes=r['bgzf_bytes'], seconds=round(time.time() - t0, 1)))


def step_run(args, say):
    from wgbs_tools_amd import init_genome
    path = op.join(args.workdir, 'g.fa' if args.form == 'plain' else 'g.fa.gz')
    text_bytes = op.getsize(op.join(args.workdir, 'g.fa'))
    want = np.fromfile(op.join(args.workdir, 'want.u32'), dtype=np.uint32)
    out = op.join(args.workdir, 'out_' + args.form)
    wall, kern, gather, emit, defl, infl = [], [], [], [], [], []
    for rep in range(args.reps + 1):
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        t = {}
        t0 = time.perf_counter()
        kept = init_genome.build_dictionary(path, out, inflate='device' if args.form == 'bgzf' else 'host', timings=t)
        dt = time.perf_counter() - t0
        if rep:                                                     # (the first run warms the device, the page cache and the allocator)
            wall.append(dt); kern.append(t['kernel_ms']); gather.append(t['gather_ms']); emit.append(t['emit_ms']); defl.append(t['deflate_ms'])
            if 'inflate_ms' in t:
                infl.append(t['inflate_ms'])
    got = np.fromfile(op.join(out, 'loci.u32'), dtype=np.uint32)
    rec = dict(step='run', form=args.form, text_bytes=text_bytes, wall_s=spread(wall), scan_kernels_ms=spread(kern, 2),
               scan_kernels_text_GBps=spread([text_bytes / (ms * 1e-3) / 1e9 for ms in kern], 2), gather_ms=spread(gather, 2), emit_ms=spread(emit, 2),
               deflate_ms=spread(defl, 2), chromosomes=len(kept), sites=int(got.size), loci_equal=bool(got.size == want.size and (got == want).all()),
               dict_bytes=op.getsize(op.join(out, 'CpG.bed.gz')), read_s=round(t.get('inflate_s', 0.0), 3), feed_s=round(t.get('feed_s', 0.0), 3))
    if infl:
        rec['inflate_ms'] = spread(infl, 2)
    say(rec)


def step_copy(args, say):
    import torch
    n = op.getsize(op.join(args.workdir, 'g.fa'))
    piece = 64 << 20
    host = torch.empty(piece, dtype=torch.uint8).pin_memory()
    dev = torch.empty(piece, dtype=torch.uint8, device='cuda')
    rates = []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range((n + piece - 1) // piece):
            dev.copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        if rep:
            rates.append(n / (time.perf_counter() - t0) / 1e9)
    say(dict(step='copy', bytes=n, host_to_device_GBps=spread(rates, 2)))


def step_cpu(args, say):
    import init_genome_ref as GR
    with open(op.join(args.workdir, 'g.fa'), 'rb') as f:
        head = f.read(300 << 20)
    text = head[:head.index(b'\n>') + 1]                            # the first chromosome's record
    t0 = time.perf_counter()
    res = GR.init_genome(text)
    dt = time.perf_counter() - t0
    say(dict(step='cpu', what='tests/init_genome_ref.py (a restatement, not the reference) on one chromosome', text_bytes=len(text), sites=int(res['loci'].size),
             seconds=round(dt, 2), text_MBps=round(len(text) / dt / 1e6, 1)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=28217448, help='CpGs of the synthetic genome [28,217,448]')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    ap.add_argument('--step', choices=('make', 'run', 'copy', 'cpu'))
    ap.add_argument('--form', choices=('plain', 'bgzf'))
    args = ap.parse_args()

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    if args.step:
        return {'make': step_make, 'run': step_run, 'copy': step_copy, 'cpu': step_cpu}[args.step](args, say)
    with tempfile.TemporaryDirectory(prefix='bench_init_genome_') as d:
        base = [sys.executable, op.abspath(__file__), '--workdir', args.workdir or d, '--sites', str(args.sites), '--reps', str(args.reps)] + (['--out', args.out] if args.out else [])
        steps = [('make', []), ('run', ['--form', 'plain']), ('run', ['--form', 'bgzf']), ('copy', []), ('cpu', [])]
        for step, more in steps:                                    # a step that fails, faults or runs out of time ends the walk
            rc = subprocess.call(['timeout', '-k', '10', str(LIMITS[step])] + base + ['--step', step] + more)
            if rc != 0:
                say(dict(step=step, failed=rc))
                return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
