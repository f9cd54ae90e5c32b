#!/usr/bin/env python3
"""`wgbstools bed2beta` on an hg19-shaped synthetic BED file (profiles/bed2beta_mi355x.txt).

Input: --sites CpGs (default 28,217,448) on 25 chromosomes (synth.genome_shape / synth_loci), one sample of uint8 pairs filled on the
device (libwgbssynth), written as BED text — one line per CpG, `chr loc-1 loc+1 meth cov`: the --add_one notation — by the device
(wgbsseg_beta2bed); behind it 1 % more lines: duplicates of lines above with other values, positions one off a CpG, chromosomes the
genome does not have.  The first line per site is the one the sample wrote, so the result must be the sample's own bytes: every run
checks that.  The same text as gzip (zlib level 1) and as BGZF (members of 65,280 bytes, zlib level 6).

Without --step this runs the steps one after another, every one a process of its own under its own `timeout -k 10`, chained with &&:
    make                 the genome directory, the sample, the three files
    run  plain|gzip|bgzf `wgbstools bed2beta --add_one -f` in one process, --reps times after a warm-up (median [min, max]): the wall time
                         of the whole call (arguments to the written .beta; the files are in the page cache), k_bedbeta_scan's device
                         time (HIP events, summed over the chunks) and the text bytes per second of it; bgzf runs with --inflate device
    copy                 the host-to-device copy of as many bytes as the text has, 64 MiB at a time from a page-locked buffer: bytes per
                         second, to hold beside the scan's
    cpu                  tests/bed2beta_ref.py's bed2beta_frames — the reference's way: pandas frames, drop_duplicates, left merge — on
                         the plain file, on this box's CPU, once; its result against the sample too
Every step prints JSON lines (and appends them to --out)."""
import argparse
import contextlib
import ctypes as C
import gzip
import io
import json
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
sys.path.insert(0, op.join(ROOT, 'tests'))

SEED = 20261021
FORMS = {'plain': ('plain', 'x.bed'), 'gzip': ('gz', 'x.bed.gz'), 'bgzf': ('bgzf', 'x.bed.gz')}
LIMITS = dict(make=420, run=300, copy=120, cpu=900)                # seconds a step may take


def spread(v, digits=4):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def shape(n):
    from wgbs_tools_amd import synth
    names, sizes = synth.genome_shape(n)
    return [str(c) for c in names], np.asarray(sizes, dtype=np.int64)


def genome_dir(d):
    return op.join(d, 'references', 'bench')


def write_genome(d, names, sizes, loci):
    """a genome directory that serves the commands here: the two size tables and the binary cache of the dictionary's second column.
    CpG.bed.gz itself is a placeholder older than the cache (28 M lines of text nobody reads)."""
    g = genome_dir(d)
    os.makedirs(g, exist_ok=True)
    with open(op.join(g, 'CpG.chrome.size'), 'w') as f:
        f.write(''.join('%s\t%d\n' % (c, s) for c, s in zip(names, sizes.tolist())))
    with open(op.join(g, 'chrome.size'), 'w') as f:
        pos = 0
        for c, s in zip(names, sizes.tolist()):
            f.write('%s\t%d\n' % (c, int(loci[pos + s - 1]) + 10000))
            pos += s
    with gzip.open(op.join(g, 'CpG.bed.gz'), 'wb') as f:
        f.write(b'')
    np.asarray(loci, dtype=np.uint32).tofile(op.join(g, 'loci.u32'))
    return g


def extra_lines(names, sizes, loci, n_extra):
    """lines behind the sample's own: a third duplicates with other values, a third one position off, a third on unknown chromosomes"""
    from wgbs_tools_amd import synth
    n = int(sizes.sum())
    site = (synth.hash_at(SEED, 801, np.arange(n_extra)) % np.uint64(n)).astype(np.int64)
    chrom = np.searchsorted(np.cumsum(sizes), site, 'right')
    out = []
    for k, (s, c) in enumerate(zip(site.tolist(), chrom.tolist())):
        p, name, kind = int(loci[s]), names[c], k % 3
        if kind == 1:
            p += 1
        elif kind == 2:
            name = 'chrUn_gl%06d' % (k % 1000)
        out.append('%s\t%d\t%d\t%d\t%d\n' % (name, p - 1, p + 1, k % 7, 7 + k % 300))
    return ''.join(out).encode()


def step_make(args, say):
    import torch
    from wgbs_tools_amd import _lib, homog, synth
    d, n = args.workdir, args.sites
    t0 = time.perf_counter()
    names, sizes = shape(n)
    loci = synth.synth_loci(SEED, sizes)
    write_genome(d, names, sizes, loci)
    pitch = ((2 * n + 255) // 256) * 256 + 256
    buf = torch.empty((1, pitch), dtype=torch.uint8, device=torch.device('cuda', 0))
    assert _lib.load_synth().wgbssynth_fill_betas(C.c_void_p(buf.data_ptr()), pitch, n, 0, 1, SEED, None) == 0
    torch.cuda.synchronize()
    buf[0, :2 * n].cpu().numpy().tofile(op.join(d, 'sample.beta'))
    for sub, _ in FORMS.values():
        os.makedirs(op.join(d, sub), exist_ok=True)
        os.makedirs(op.join(d, 'out_' + sub), exist_ok=True)
    plain = op.join(d, *FORMS['plain'])
    with _lib.Segmenter(0) as seg:
        seg.set_betas_device(buf.data_ptr(), 1, pitch, n, keepalive=buf)
        seg.set_loci(loci)
        fd = os.open(plain, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            lines, nbytes = seg.beta2bed(fd, 0, names, np.cumsum(sizes), keep_na=True)
        finally:
            os.close(fd)
    assert lines == n
    extra = extra_lines(names, sizes, loci, n // 100)
    with open(plain, 'ab') as f:
        f.write(extra)
    with open(plain, 'rb') as f:
        text = f.read()
    with gzip.open(op.join(d, *FORMS['gzip']), 'wb', compresslevel=1) as f:
        f.write(text)
    homog.write_bgzf(op.join(d, *FORMS['bgzf']), text, 16)
    say(dict(step='make', sites=n, chromosomes=len(names), lines=n + n // 100, text_bytes=len(text), gzip_bytes=op.getsize(op.join(d, *FORMS['gzip'])),
             bgzf_bytes=op.getsize(op.join(d, *FORMS['bgzf'])), made_in_s=round(time.perf_counter() - t0, 1)))


def same_as_sample(d, path):
    a, b = np.fromfile(op.join(d, 'sample.beta'), dtype=np.uint8), np.fromfile(path, dtype=np.uint8)
    return bool(a.size == b.size and np.array_equal(a, b))


def step_run(args, say):
    from wgbs_tools_amd import wgbs_tools
    d, (sub, name) = args.workdir, FORMS[args.form]
    bed, outdir = op.join(d, sub, name), op.join(d, 'out_' + sub)
    argv = ['wgbstools', 'bed2beta', bed, '--add_one', '-f', '-o', outdir, '--genome', genome_dir(d)] + (['--inflate', 'device'] if args.form == 'bgzf' else [])
    text_bytes = op.getsize(op.join(d, *FORMS['plain']))
    walls, scan, inflate, summary = [], [], [], ''
    for rep in range(args.reps + 1):                                   # the first: warm-up (the library, the page cache)
        err = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stderr(err):
            rc = wgbs_tools.main(argv)
        wall = time.perf_counter() - t0
        assert rc == 0, err.getvalue()
        summary = [ln for ln in err.getvalue().splitlines() if ' lines, ' in ln][-1]
        if rep:
            walls.append(wall)
            scan.append(float(re.search(r'scan ([0-9.]+) ms', summary).group(1)))
            m = re.search(r'inflate ([0-9.]+) ms', summary)
            if m:
                inflate.append(float(m.group(1)))
    rec = dict(step='run', form=args.form, argv=' '.join(argv[:2] + [name] + argv[3:5]) + (' --inflate device' if args.form == 'bgzf' else ''),
               file_bytes=op.getsize(bed), text_bytes=text_bytes, wall_s=spread(walls), scan_ms=spread(scan),
               scan_text_bytes_per_s=float('%.4g' % (text_bytes / spread(scan)['median'] * 1e3)), equals_sample=same_as_sample(d, op.join(outdir, 'x.beta')),
               summary=summary)
    if inflate:
        rec['inflate_ms'] = spread(inflate)
    say(rec)


def step_copy(args, say):
    import torch
    n, chunk = op.getsize(op.join(args.workdir, *FORMS['plain'])), 64 << 20
    host = torch.empty(chunk, dtype=torch.uint8).pin_memory()
    dev = torch.empty(chunk, dtype=torch.uint8, device=torch.device('cuda', 0))
    ms = []
    for rep in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for off in range(0, n, chunk):
            k = min(chunk, n - off)
            dev[:k].copy_(host[:k], non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    say(dict(step='copy', bytes=n, chunk_bytes=chunk, copy_ms=spread(ms), copy_bytes_per_s=float('%.4g' % (n / spread(ms)['median'] * 1e3))))


def step_cpu(args, say):
    import bed2beta_ref as BR
    d = args.workdir
    names, sizes = shape(args.sites)
    loci = np.fromfile(op.join(genome_dir(d), 'loci.u32'), dtype=np.uint32)
    t0 = time.perf_counter()
    frame = BR.dict_frame(loci, list(zip(names, sizes.tolist())))
    t1 = time.perf_counter()
    rows = BR.bed2beta_frames(op.join(d, *FORMS['plain']), frame, add_one=True)
    t2 = time.perf_counter()
    out = op.join(d, 'cpu.beta')
    rows.tofile(out)
    say(dict(step='cpu', what='tests/bed2beta_ref.py bed2beta_frames on the plain file, one process', dictionary_frame_s=round(t1 - t0, 2),
             file_to_rows_s=round(t2 - t1, 2), equals_sample=same_as_sample(d, out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=None, help='CpGs of the synthetic genome [28,217,448]')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    ap.add_argument('--no-cpu', action='store_true', help='leave the pandas restatement out')
    ap.add_argument('--step', choices=('make', 'run', 'copy', 'cpu'))
    ap.add_argument('--form', choices=tuple(FORMS))
    args = ap.parse_args()
    if args.sites is None:
        from wgbs_tools_amd import synth
        args.sites = synth.HG19_NR_SITES

    def say(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    if args.step:
        return {'make': step_make, 'run': step_run, 'copy': step_copy, 'cpu': step_cpu}[args.step](args, say)
    d = args.workdir or tempfile.mkdtemp(prefix='bed2beta_bench_')
    os.makedirs(d, exist_ok=True)
    common = [sys.executable, op.abspath(__file__), '--workdir', d, '--sites', str(args.sites), '--reps', str(args.reps)] + (['--out', args.out] if args.out else [])
    steps = [('make', [])] + [('run', ['--form', f]) for f in FORMS] + [('copy', [])] + ([] if args.no_cpu else [('cpu', [])])
    import shlex
    chain = ' && '.join('timeout -k 10 %d %s' % (LIMITS[s], ' '.join(shlex.quote(x) for x in common + ['--step', s] + more)) for s, more in steps)
    try:
        return subprocess.call(['bash', '-c', chain])
    finally:
        if not args.workdir:
            import shutil
            shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
