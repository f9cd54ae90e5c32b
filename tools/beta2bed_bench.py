#!/usr/bin/env python3
"""k_bed_len + k_bed_scan + k_bed_emit (wgbsseg_beta2bed: `wgbstools beta2bed`) on hg19-shaped synthetic data
(profiles/beta2bed_*.txt).

One sample of 28,217,448 sites of uint8 pairs, filled on the device (libwgbssynth) and handed over by pointer; synthetic loci on 25
chromosomes (synth.genome_shape / synth_loci).  Two configurations, whole genome: plain (`chr start end meth cov`, sites
without reads dropped) and --mean (`chr start end ratio`).  For either, as median [min, max] of --reps calls after a warm-up:
  length    HIP-event time of the length pass and the scan, summed over the slabs
  emit      HIP-event time of the emit pass, summed over the slabs, and the text's bytes per second of it
  /dev/null wall time of the whole call writing to /dev/null (slabs produced, brought home, written)
  file      wall time of the whole call writing to a file in a temporary directory
--awk: for scale, awk filters that do what the reference's three stages do (coverage threshold, drop sites without reads, the
  "%.3g" ratio), each alone over the same base lines (every site, written by the device to a file first) on this host's CPU,
  one process, output to /dev/null; and the sha1 of what the drop and the ratio stage print against the device's two texts.
"""
import argparse
import ctypes as C
import hashlib
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

from wgbs_tools_amd import _lib, synth          # noqa: E402

N_SITES = synth.HG19_NR_SITES
SEED = 20260926

AWK_STAGES = {
    'coverage threshold 10': r'''BEGIN { FS = OFS = "\t" } $5 < 10 { $4 = 0; $5 = 0 } { print }''',
    'drop sites without reads': r'''BEGIN { FS = "\t" } $5 + 0 > 0''',
    'ratio': r'''BEGIN { FS = "\t" } { if ($5 > 0) printf "%s\t%d\t%d\t%.3g\n", $1, $2, $3, $4 / $5; else printf "%s\t%d\t%d\t-1\n", $1, $2, $3 }''',
}


def device_rows(n_sites):
    import torch
    pitch = ((2 * n_sites + 255) // 256) * 256 + 256
    buf = torch.empty((1, pitch), dtype=torch.uint8, device=torch.device('cuda', 0))
    rc = _lib.load_synth().wgbssynth_fill_betas(C.c_void_p(buf.data_ptr()), pitch, n_sites, 0, 1, SEED, None)
    assert rc == 0
    torch.cuda.synchronize()
    return buf, pitch


def spread(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def sha1_of(path):
    h = hashlib.sha1()
    with open(path, 'rb') as f:
        for piece in iter(lambda: f.read(1 << 24), b''):
            h.update(piece)
    return h.hexdigest()


def sha1_of_awk(prog, path):
    h = hashlib.sha1()
    with subprocess.Popen(['awk', prog, path], stdout=subprocess.PIPE) as p:
        for piece in iter(lambda: p.stdout.read(1 << 24), b''):
            h.update(piece)
    assert p.returncode == 0
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=N_SITES)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--awk', action='store_true')
    args = ap.parse_args()
    n = args.sites
    names, sizes = synth.genome_shape(n)
    loci = synth.synth_loci(SEED, sizes)
    cum = np.cumsum(sizes)
    buf, pitch = device_rows(n)
    print(json.dumps(dict(sites=n, chromosomes=len(names), limits=_lib.beta2bed_limits())), flush=True)
    d = tempfile.mkdtemp(prefix='beta2bed_bench_')
    try:
        with _lib.Segmenter(0) as seg:
            seg.set_betas_device(buf.data_ptr(), 1, pitch, n, keepalive=buf)
            seg.set_loci(loci)

            def run(path, **kw):
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                try:
                    t0 = time.perf_counter()
                    lines, nbytes = seg.beta2bed(fd, 0, names, cum, **kw)
                    wall = time.perf_counter() - t0
                finally:
                    os.close(fd)
                return lines, nbytes, wall, seg.beta2bed_pass_ms()

            texts = {}
            for what, kw in (('plain', {}), ('mean', dict(mean=True))):
                lines, nbytes, _, _ = run('/dev/null', **kw)                  # warm-up (allocations, code load)
                walls, len_ms, emit_ms = [], [], []
                for _ in range(args.reps):
                    got = run('/dev/null', **kw)
                    assert got[:2] == (lines, nbytes)
                    walls.append(got[2])
                    len_ms.append(got[3][0])
                    emit_ms.append(got[3][1])
                e = spread(emit_ms)
                print(json.dumps(dict(what=what, lines=lines, bytes=nbytes, length_ms=spread(len_ms), emit_ms=e,
                                      emit_bytes_per_s=float('%.4g' % (nbytes / e['median'] * 1e3)), wall_s_dev_null=spread(walls))), flush=True)
                texts[what] = op.join(d, what + '.bed')
                walls = [run(texts[what], **kw)[2] for _ in range(max(2, args.reps // 2))]
                assert op.getsize(texts[what]) == nbytes
                print(json.dumps(dict(what=what + ' to a file', wall_s=spread(walls), bytes_per_s=float('%.4g' % (nbytes / spread(walls)['median'])))), flush=True)
            if args.awk:
                base = op.join(d, 'base.bed')
                lines, nbytes, wall, _ = run(base, keep_na=True)
                assert lines == n
                print(json.dumps(dict(what='base lines (every site) to a file', bytes=nbytes, wall_s=round(wall, 4))), flush=True)
                for what, prog in AWK_STAGES.items():
                    t0 = time.perf_counter()
                    subprocess.check_call(['awk', prog, base], stdout=subprocess.DEVNULL)
                    print(json.dumps(dict(what='awk, one process, base lines -> /dev/null: ' + what, wall_s=round(time.perf_counter() - t0, 2))), flush=True)
                plain_equal = sha1_of_awk(AWK_STAGES['drop sites without reads'], base) == sha1_of(texts['plain'])
                mean_equal = sha1_of_awk(AWK_STAGES['ratio'], texts['plain']) == sha1_of(texts['mean'])      # (the plain text IS the drop stage's, when equal)
                print(json.dumps(dict(what='sha1 of the awk stages\' text against the device\'s', plain_equal=plain_equal, mean_equal=mean_equal)), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
