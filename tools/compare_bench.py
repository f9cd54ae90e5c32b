#!/usr/bin/env python3
"""k_pair_ranges + k_pair_hist (wgbsseg_pair_ranges / wgbsseg_pair_hist: `wgbstools compare_betas`) on hg19-shaped synthetic
rows (profiles/compare_betas_*.txt).

Rows: 28,217,448 sites x --samples samples of uint8 pairs, filled on the device (libwgbssynth) and handed over by pointer; all
pairs (i, j) with j <= i (528 for 32 samples), --min_cov 10, --bins 101.  Reports, as median [min, max] of --reps calls after
a warm-up:
  ranges    HIP-event time of pass 1 (k_pair_ranges)
  hist      HIP-event time of pass 2 (the clearing of the counts + k_pair_hist), with the corner cells counted in registers
            (WGBSSEG_PAIR_CORNERS=1) and with every cell through LDS atomics (=0, the default), alternating; both must give
            the same bytes
  and pair-sites per second of either (pairs x sites / time), the share of the masked-in sites and of those in the two
  corner cells.
--wall: the rows are written to .beta files in a temporary directory and compare_betas.pair_histograms runs from the files
  (map, upload, both passes, edges on the host, counts home): wall time.
--numpy-pairs K: np.histogram2d on K pairs of the same rows on this host's CPU, for scale, and its counts against the
  device's.
One run measures one sample count: a job runs it per count, each under its own time limit.
"""
import argparse
import ctypes as C
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

from wgbs_tools_amd import _lib, compare_betas, synth          # noqa: E402

N_SITES = synth.HG19_NR_SITES
SEED = 20260926


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=N_SITES)
    ap.add_argument('--samples', type=int, default=32)
    ap.add_argument('--min_cov', type=int, default=10)
    ap.add_argument('--bins', type=int, default=101)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--wall', action='store_true')
    ap.add_argument('--numpy-pairs', type=int, default=0)
    args = ap.parse_args()
    n, S = args.sites, args.samples
    pairs = compare_betas.all_pairs(S)
    pair_sites = float(len(pairs)) * n
    buf, pitch = device_rows(n, S)
    print(json.dumps(dict(sites=n, samples=S, pairs=len(pairs), pair_sites=pair_sites, min_cov=args.min_cov, bins=args.bins, limits=_lib.pair_hist_limits())), flush=True)
    with _lib.Segmenter(0) as seg:
        seg.set_betas_device(buf.data_ptr(), S, pitch, n, keepalive=buf)
        got = seg.pair_ranges(pairs, args.min_cov)                      # warm-up (allocations, code load)
        ms = []
        for _ in range(args.reps):
            assert seg.pair_ranges(pairs, args.min_cov).tobytes() == got.tobytes()
            ms.append(seg.last_block_sums_ms())
        r = spread(ms)
        print(json.dumps(dict(what='ranges (pass 1)', ms=r, pair_sites_per_s=float('%.4g' % (pair_sites / r['median'] * 1e3)),
                              masked_in_share=round(float(got['n'].sum()) / pair_sites, 4))), flush=True)
        xe = np.stack([compare_betas.edges_of(g['n'], float(g['b_min']), float(g['b_max']), args.bins) for g in got])
        ye = np.stack([compare_betas.edges_of(g['n'], float(g['a_min']), float(g['a_max']), args.bins) for g in got])
        edges = np.stack([xe, ye], axis=1)
        counts = seg.pair_hist(pairs, args.min_cov, args.bins, edges)   # warm-up
        assert (counts.sum(axis=(1, 2)) == got['n']).all()
        ms = {'1': [], '0': []}
        for _ in range(args.reps):
            for form in ('1', '0'):
                os.environ['WGBSSEG_PAIR_CORNERS'] = form               # (read per call)
                assert seg.pair_hist(pairs, args.min_cov, args.bins, edges).tobytes() == counts.tobytes()
                ms[form].append(seg.last_block_sums_ms())
        del os.environ['WGBSSEG_PAIR_CORNERS']
        corner = float(counts[:, 0, 0].sum() + counts[:, -1, -1].sum()) / max(float(counts.sum()), 1.0)
        for form, name in (('1', 'hist (pass 2), corner cells in registers'), ('0', 'hist (pass 2), every cell through LDS atomics')):
            r = spread(ms[form])
            print(json.dumps(dict(what=name, ms=r, pair_sites_per_s=float('%.4g' % (pair_sites / r['median'] * 1e3)), corner_share_of_counted=round(corner, 4))), flush=True)
        if args.numpy_pairs:
            pick = [len(pairs) - 2, len(pairs) // 2, 1][:args.numpy_pairs]          # (off the diagonal)
            host = {}
            secs = []
            for k in pick:
                i, j = (int(v) for v in pairs[k])
                for s in (i, j):
                    if s not in host:
                        host[s] = buf[s, :2 * n].cpu().numpy().reshape(-1, 2)
                t0 = time.perf_counter()
                a, b = host[i], host[j]
                keep = np.min(np.c_[a[:, 1], b[:, 1]], axis=1) >= args.min_cov
                h, hx, hy = np.histogram2d(b[keep][:, 0] / b[keep][:, 1], a[keep][:, 0] / a[keep][:, 1], args.bins)
                secs.append(time.perf_counter() - t0)
                assert np.array_equal(h.astype(np.uint64), counts[k]) and hx.tobytes() == xe[k].tobytes() and hy.tobytes() == ye[k].tobytes(), (i, j)
            print(json.dumps(dict(what='np.histogram2d (mask, ratios, histogram) on this host, one process', pairs=[[int(v) for v in pairs[k]] for k in pick],
                                  s_per_pair=spread(secs), equal_to_device=True)), flush=True)
    if args.wall:
        d = tempfile.mkdtemp(prefix='compare_bench_')
        try:
            paths = []
            for s in range(S):
                paths.append(op.join(d, 'smp%02d.beta' % s))
                buf[s, :2 * n].cpu().numpy().tofile(paths[-1])
            del buf
            walls, kms = [], []
            for _ in range(max(2, args.reps // 2)):
                t = []
                t0 = time.perf_counter()
                res = compare_betas.pair_histograms(paths, args.min_cov, args.bins, timings=t)
                walls.append(time.perf_counter() - t0)
                kms.append(sum(t))
                assert res[1].tobytes() == counts.tobytes()
            print(json.dumps(dict(what='pair_histograms from %d .beta files (page cache): map, upload, two passes, counts home' % S, wall_s=spread(walls),
                                  kernels_ms=spread(kms))), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
