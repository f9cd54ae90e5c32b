#!/usr/bin/env python3
"""k_site_gather + k_site_len + k_bed_scan + k_site_emit (wgbsseg_site_table: `wgbstools beta_to_450k`) on hg19-shaped synthetic
data (profiles/beta_to_450k_*.txt).

32 samples of 28,217,448 sites of uint8 pairs, filled on the device (libwgbssynth) and handed over by pointer; 480,000 distinct
random sites in no order with the labels cg00000000 ...; min_cov 3.  As median [min, max] of --reps calls after a warm-up:
  gather    HIP-event time of the gather pass, summed over the slabs, and the cells per second of it
  text      HIP-event time of the length pass and the scan | of the emit pass, and the text's bytes per second of the emit pass
  /dev/null wall time of the whole call writing to /dev/null (slabs produced, brought home, written)
  file      wall time of the whole call writing to a file in a temporary directory
  counts    wgbsseg_site_counts over the same sites and samples: HIP-event time and wall time
--cpu: for scale, the same table on this host's CPU from the same rows (copied home first), one process: tests/array_ref.py's
  numpy restatement (every distinct pair formatted once), and — where pandas is installed — a frame of the ratios written by
  DataFrame.to_csv(float_format='%.3f', na_rep='NA'), the way the reference writes it; the sha1 of both against the device's text.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import os.path as op
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))

from wgbs_tools_amd import _lib, synth          # noqa: E402

N_SITES = synth.HG19_NR_SITES
SEED = 20261102
MIN_COV = 3


def device_rows(n_sites, n_samples):
    import torch
    pitch = ((2 * n_sites + 255) // 256) * 256 + 256
    buf = torch.empty((n_samples, pitch), dtype=torch.uint8, device=torch.device('cuda', 0))
    rc = _lib.load_synth().wgbssynth_fill_betas(C.c_void_p(buf.data_ptr()), pitch, n_sites, 0, n_samples, SEED, None)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=N_SITES)
    ap.add_argument('--samples', type=int, default=32)
    ap.add_argument('--probes', type=int, default=480000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', action='store_true')
    args = ap.parse_args()
    n, k, p = args.sites, args.samples, args.probes
    rng = np.random.default_rng(SEED)
    site0 = rng.choice(n, p, replace=False).astype(np.int64)
    labels = [b'cg%08d' % i for i in range(p)]
    samples = np.arange(k)
    buf, pitch = device_rows(n, k)
    print(json.dumps(dict(sites=n, samples=k, probes=p, min_cov=MIN_COV, limits=_lib.site_table_limits())), flush=True)
    d = tempfile.mkdtemp(prefix='beta450k_bench_')
    try:
        with _lib.Segmenter(0) as seg:
            seg.set_betas_device(buf.data_ptr(), k, pitch, n, keepalive=buf)

            def run(path):
                fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                try:
                    t0 = time.perf_counter()
                    lines, nbytes = seg.site_table(fd, site0, samples, labels, min_cov=MIN_COV)
                    wall = time.perf_counter() - t0
                finally:
                    os.close(fd)
                return lines, nbytes, wall, seg.site_table_pass_ms()

            lines, nbytes, _, _ = run('/dev/null')                            # warm-up (allocations, code load)
            walls, passes = [], []
            for _ in range(args.reps):
                got = run('/dev/null')
                assert got[:2] == (lines, nbytes)
                walls.append(got[2])
                passes.append(got[3])
            g, ln, e = (spread([x[i] for x in passes]) for i in range(3))
            print(json.dumps(dict(what='site_table', lines=lines, bytes=nbytes, gather_ms=g, gather_cells_per_s=float('%.4g' % (p * k / g['median'] * 1e3)),
                                  length_ms=ln, emit_ms=e, emit_bytes_per_s=float('%.4g' % (nbytes / e['median'] * 1e3)), wall_s_dev_null=spread(walls))), flush=True)
            text = op.join(d, 'table.csv')
            walls = [run(text)[2] for _ in range(max(2, args.reps // 2))]
            assert op.getsize(text) == nbytes
            print(json.dumps(dict(what='site_table to a file', wall_s=spread(walls), bytes_per_s=float('%.4g' % (nbytes / spread(walls)['median'])))), flush=True)
            counts = seg.site_counts(site0, samples)                        # warm-up
            walls, ms = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                counts = seg.site_counts(site0, samples)
                walls.append(time.perf_counter() - t0)
                ms.append(seg.last_block_sums_ms())
            print(json.dumps(dict(what='site_counts', bytes=int(counts.nbytes), gather_ms=spread(ms), wall_s=spread(walls))), flush=True)
        device_sha1 = sha1_of(text)
        print(json.dumps(dict(what='the device\'s text', sha1=device_sha1)), flush=True)
        if args.cpu:
            import array_ref as AR
            home = buf.cpu().numpy()
            rows = [home[s, :2 * n].reshape(n, 2) for s in range(k)]
            t0 = time.perf_counter()
            body = AR.table_body([x.decode() for x in labels], site0, rows, MIN_COV)
            wall = time.perf_counter() - t0
            sha1 = hashlib.sha1(body).hexdigest()
            print(json.dumps(dict(what='CPU, one process: tests/array_ref.py (numpy, every distinct pair formatted once)', wall_s=round(wall, 2), sha1=sha1,
                                  equal=sha1 == device_sha1)), flush=True)
            assert np.array_equal(counts, np.stack([r[site0] for r in rows], axis=1))
            try:
                import pandas as pd
            except ImportError:
                pd = None
            if pd is not None:
                t0 = time.perf_counter()
                frame = pd.DataFrame({'ilmn': [x.decode() for x in labels]})
                for s, r in enumerate(rows):
                    c = r[site0]
                    ok = c[:, 1] >= MIN_COV
                    v = np.divide(c[:, 0], c[:, 1], where=ok, out=np.full(p, np.nan))
                    frame['s%02d' % s] = v
                out = op.join(d, 'pandas.csv')
                frame.to_csv(out, index=None, header=False, float_format='%.3f', na_rep='NA')
                wall = time.perf_counter() - t0
                sha1 = sha1_of(out)
                print(json.dumps(dict(what='CPU, one process: numpy ratios + DataFrame.to_csv (the reference\'s way)', wall_s=round(wall, 2), sha1=sha1,
                                      equal=sha1 == device_sha1)), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
