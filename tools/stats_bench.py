#!/usr/bin/env python3
"""k_sample_stats (wgbsseg_sample_stats: `wgbstools beta_cov` / `beta_stats`) on hg19-shaped synthetic rows resident in HBM
(profiles/stats_*.txt).

Rows: 28,217,448 sites x 32 and x 8 samples of uint8 pairs, filled on the device (libwgbssynth) and handed over by pointer.
Reports, as median [min, max] of --reps calls after a warm-up, the HIP-event time of the two kernels of one call
(k_sample_stats + k_sample_stats_fold) and the bytes of the rows it has to read once (2 * sites * samples) per second, for
  whole    the whole genome as one range
  bed      100,000 disjoint ranges of 1-400 sites at random places (what `beta_stats -L` hands over)
and, on the same rows, the scan pass the README's headline bandwidth comes from (wgbsseg_scan_only), as the ceiling to compare
with.  The results of `whole` are checked against numpy on a 2 M-site prefix of two samples copied back from the device.
"""
import argparse
import ctypes as C
import json
import os.path as op
import sys

import numpy as np

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))

from wgbs_tools_amd import _lib, synth          # noqa: E402

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


def bed_ranges(n_sites, n_ranges, rng):
    starts = np.sort(rng.choice(n_sites - 400, n_ranges, replace=False).astype(np.int64))
    ends = np.minimum(starts + rng.integers(1, 401, n_ranges), np.concatenate([starts[1:], [n_sites]]))
    return np.stack([starts, ends], axis=1)


def spread(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sites', type=int, default=N_SITES)
    ap.add_argument('--samples', type=int, nargs='+', default=[32, 8])
    ap.add_argument('--ranges', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', help='also write the numbers here')
    args = ap.parse_args()
    import stats_ref as SR
    rng = np.random.default_rng(1)
    bed = bed_ranges(args.sites, args.ranges, rng)
    out = []
    for n_samples in args.samples:
        buf, pitch = device_rows(args.sites, n_samples)
        with _lib.Segmenter(0) as seg:
            seg.set_betas_device(buf.data_ptr(), n_samples, pitch, args.sites, keepalive=buf)
            for what, ranges in (('whole', np.array([[0, args.sites]], dtype=np.int64)), ('bed', bed)):
                res = seg.sample_stats(ranges)                      # warm-up (allocations, code load)
                ms = []
                for _ in range(args.reps):
                    again = seg.sample_stats(ranges)
                    ms.append(seg.last_block_sums_ms())
                    assert again.tobytes() == res.tobytes()
                med, lo, hi = spread(ms)
                nbytes = 2 * int((ranges[:, 1] - ranges[:, 0]).sum()) * n_samples
                rec = dict(what=what, samples=n_samples, sites=int((ranges[:, 1] - ranges[:, 0]).sum()), ranges=len(ranges), ms_median=med, ms_min=lo,
                           ms_max=hi, bytes=nbytes, tb_per_s=nbytes / med / 1e9)
                out.append(rec)
                print('x%-3d %-5s %9d sites in %6d ranges: %.3f ms [%.3f, %.3f]  %.3f TB/s of row bytes' %
                      (n_samples, what, rec['sites'], len(ranges), med, lo, hi, rec['tb_per_s']), flush=True)
            # the ceiling: the scan pass over the same rows
            lens = np.full((args.sites + 59999) // 60000, 60000, dtype=np.int32)
            st = np.arange(lens.size, dtype=np.int64) * 60000
            lens[-1] = args.sites - int(st[-1])
            seg.scan_only(st, lens, repeat=2)
            sms, sbytes = seg.scan_only(st, lens, repeat=args.reps)
            out.append(dict(what='scan_only', samples=n_samples, ms_median=sms, bytes=sbytes, tb_per_s=sbytes / sms / 1e9))
            print('x%-3d scan pass over the same rows: %.3f ms  %.3f TB/s' % (n_samples, sms, sbytes / sms / 1e9), flush=True)
            # correctness on a prefix of two samples
            k = min(args.sites, 2_000_000)
            got = seg.sample_stats([(0, k)])
            for s in (0, n_samples - 1):
                rows = buf[s, :2 * k].cpu().numpy().reshape(-1, 2)
                assert SR.as_dict(got[s]) == SR.expect(rows, [(0, k)]), s
            print('x%-3d results equal numpy on the first %d sites of samples 0 and %d' % (n_samples, k, n_samples - 1), flush=True)
        del buf
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
