#!/usr/bin/env python3
"""`wgbstools bam2pat` on a synthetic collated paired-end SAM file over an hg19-shaped dictionary (profiles/bam2pat_mi355x.txt).

Input: --sites CpGs (default 28,217,448) on 25 chromosomes (synth.genome_shape / synth_loci).  A block of --block pairs is written line
by line — mates of 100 bases, 99 / 147 and 83 / 163, placed at random CpGs, every CpG under a read made CG / TG (or CG / CA), one pair in
fifty with a soft clip and a deletion — and repeated until the file holds --lines lines (default 10 M); behind it --tail lines of
unmapped reads (FLAG 77 / 141), as an aligner leaves them.  The same text as BGZF (members of 65,280 bytes).

Steps, every one a process of its own under its own `timeout -k 10`, chained with && (without --step: all of them):
    make        the genome directory and the two files
    run plain   the whole call (bam2pat.sam2pat: arguments to the written .pat.gz, --no_beta; the file is in the page cache) --reps times
    run bgzf    after a warm-up, median [min, max]: the wall time, the SAM kernels' device time (HIP events, summed over the chunks) and
                the text bytes per second of it, and finish()'s sort, emit and deflate; bgzf runs with --inflate device
    copy        the host-to-device copy of as many bytes as the text has, 64 MiB at a time from a page-locked buffer: bytes per second,
                the yardstick to hold beside the kernels' rate — below it, the call waits for the kernels
Every step prints JSON lines (and appends them to --out)."""
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

SEED = 20261021
LIMITS = dict(make=600, run=420, copy=120)                         # seconds a step may take


def spread(v, digits=4):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def genome_dir(d):
    return op.join(d, 'references', 'bench')


def block_text(loci, names, sizes, n_pairs, rng, read_len=100):
    """n_pairs collated pairs as SAM text"""
    cum = np.concatenate([[0], np.cumsum(sizes)])
    out = []
    site = rng.integers(0, len(loci) - 64, n_pairs)
    for k in range(n_pairs):
        s = int(site[k])
        c = int(np.searchsorted(cum, s, 'right')) - 1
        if s + 40 >= cum[c + 1]:
            s = int(cum[c])
        bottom = bool(k & 1)
        flags = (83, 163) if bottom else (99, 147)
        p1 = int(loci[s]) - int(rng.integers(0, 30))
        p2 = p1 + int(rng.integers(20, 160))
        for mate, pos in enumerate((p1, p2)):
            pos = max(pos, 1)
            seq = bytearray(rng.choice(np.frombuffer(b'AGT', dtype=np.uint8), read_len).tobytes())
            a = int(np.searchsorted(loci[s:s + 64], pos)) + s
            while a < cum[c + 1] and int(loci[a]) - pos < read_len - 1:
                i = int(loci[a]) - pos
                meth = rng.random() < 0.7
                seq[i:i + 2] = (b'CG' if meth else b'CA') if bottom else (b'CG' if meth else b'TG')
                a += 1
            cigar = '%dM' % read_len
            if k % 50 == 7:
                cigar, seq = '3S40M2D%dM' % (read_len - 43), seq
            out.append('r%d\t%d\t%s\t%d\t42\t%s\t=\t%d\t%d\t%s\t%s\tNM:i:1\tXM:Z:%s\n' % (k, flags[mate], names[c], pos, cigar, p2 if mate == 0 else p1, 150,
                                                                                 seq.decode(), 'F' * read_len, '.' * read_len))
    return ''.join(out).encode()


def step_make(args, say):
    from wgbs_tools_amd import homog, synth
    names, sizes = synth.genome_shape(args.sites)
    names, sizes = [str(c) for c in names], np.asarray(sizes, dtype=np.int64)
    loci = synth.synth_loci(SEED, sizes)
    synth.write_genome(genome_dir(args.workdir), names, sizes, loci, gz=False)
    rng = np.random.default_rng(SEED)
    t0 = time.time()
    block = block_text(loci.astype(np.int64), names, sizes, args.block, rng)
    lines_per_block = 2 * args.block
    reps = (args.lines + lines_per_block - 1) // lines_per_block
    tail = b''.join(b'u%d\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tYT:Z:UP\n' % (k, 77 if k % 2 == 0 else 141, b'ACGT' * 25, b'F' * 100) for k in range(1000)) * (args.tail // 1000)
    plain = op.join(args.workdir, 'x.sam')
    with open(plain, 'wb') as f:
        f.write(b'@HD\tVN:1.6\tSO:unsorted\tGO:query\n')
        for _ in range(reps):
            f.write(block)
        f.write(tail)
    text_bytes = op.getsize(plain)
    with open(plain, 'rb') as f:
        homog.write_bgzf(op.join(args.workdir, 'x.sam.gz'), f.read(), 16)
    say(dict(step='make', sites=int(args.sites), lines=int(reps * lines_per_block + tail.count(b'\n') + 1), pairs=int(reps * args.block), unmapped_tail=int(tail.count(b'\n')),
             text_bytes=text_bytes, bgzf_bytes=op.getsize(op.join(args.workdir, 'x.sam.gz')), seconds=round(time.time() - t0, 1)))


def step_run(args, say):
    from wgbs_tools_amd import bam2pat
    from wgbs_tools_amd.genome import GenomeRefPaths
    from wgbs_tools_amd.pat2beta import feed_pat
    path = op.join(args.workdir, 'x.sam' if args.form == 'plain' else 'x.sam.gz')
    text_bytes = op.getsize(op.join(args.workdir, 'x.sam'))
    genome = GenomeRefPaths(genome_dir(args.workdir))
    genome.loci()
    cli = bam2pat.parse_args([path, '-o', args.workdir, '--no_beta', '-f', '--inflate', 'device' if args.form == 'bgzf' else 'host'])
    wall, kern, sort, emit, defl, infl = [], [], [], [], [], []
    stats = lines = None
    for rep in range(args.reps + 1):
        t = {}
        t0 = time.perf_counter()
        lines, nbytes, stats = bam2pat.sam2pat(lambda v: feed_pat(v, path, t, inflate=cli.inflate), op.join(args.workdir, 'x.pat.gz'), genome, True, cli, t)
        dt = time.perf_counter() - t0
        if rep:                                                     # (the first run warms the device, the page cache and the allocator)
            wall.append(dt); kern.append(t['kernel_ms']); sort.append(t['sort_ms']); emit.append(t['emit_ms']); defl.append(t['deflate_ms'])
            if 'inflate_ms' in t:
                infl.append(t['inflate_ms'])
    rec = dict(step='run', form=args.form, text_bytes=text_bytes, wall_s=spread(wall), sam_kernels_ms=spread(kern, 2),
               sam_kernels_text_GBps=spread([text_bytes / (ms * 1e-3) / 1e9 for ms in kern], 2), sort_ms=spread(sort, 2), emit_ms=spread(emit, 2), deflate_ms=spread(defl, 2),
               out_lines=lines, out_bytes=nbytes, records=t.get('records'), counters=stats)
    if infl:
        rec['inflate_ms'] = spread(infl, 2)
    say(rec)


def step_copy(args, say):
    import torch
    n = op.getsize(op.join(args.workdir, 'x.sam'))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=28217448, help='CpGs of the synthetic genome [28,217,448]')
    ap.add_argument('--lines', type=int, default=10_000_000, help='alignment lines of mapped pairs [10 M]')
    ap.add_argument('--tail', type=int, default=500_000, help='unmapped lines behind them [500 k]')
    ap.add_argument('--block', type=int, default=25_000, help='pairs written out before the text repeats [25 k]')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    ap.add_argument('--step', choices=('make', 'run', 'copy'))
    ap.add_argument('--form', choices=('plain', 'bgzf'))
    args = ap.parse_args()

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    if args.step:
        return {'make': step_make, 'run': step_run, 'copy': step_copy}[args.step](args, say)
    with tempfile.TemporaryDirectory(prefix='bench_bam2pat_') as d:
        base = [sys.executable, op.abspath(__file__), '--workdir', args.workdir or d, '--sites', str(args.sites), '--lines', str(args.lines), '--tail', str(args.tail),
                '--block', str(args.block), '--reps', str(args.reps)] + (['--out', args.out] if args.out else [])
        steps = [('make', []), ('run', ['--form', 'plain']), ('run', ['--form', 'bgzf']), ('copy', [])]
        for step, more in steps:                                    # a step that fails, faults or runs out of time ends the walk
            rc = subprocess.call(['timeout', '-k', '10', str(LIMITS[step])] + base + ['--step', step] + more)
            if rc != 0:
                say(dict(step=step, failed=rc))
                return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
