#!/usr/bin/env python3
"""random_world_cases.json: border lists printed by the REFERENCE `segmentor` (oracle/_ref/segmentor = the reference's
src/segment_betas/{main,segmentor}.cpp compiled where they lie), `-s start0 -n len` on the random worlds of tests/cases.py
random_world(seed), three chunks each.  Runs only in the build container.

Usage:  python tests/golden/make_golden_random_worlds.py
"""
import json
import os
import os.path as op
import sys
import tempfile

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))

import cases                                   # noqa: E402
from oracle import oracle                      # noqa: E402

SEEDS = range(24)

oracle.build(ref=True)
assert oracle.have_ref(), 'reference binary not built'
out = {}
for seed in SEEDS:
    slices, loci, pcount, max_cpg, max_bp, chunks = cases.random_world(seed)
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for i, s in enumerate(slices):
            p = os.path.join(td, 's%02d.beta' % i)
            s.tofile(p)
            paths.append(p)
        borders = [oracle.ref_segment_chunk(paths, st, ln, loci[st:st + ln], pcount, max_cpg, max_bp).tolist() for st, ln in chunks]
    out[str(seed)] = dict(input_crc32=cases.case_checksum(slices, loci), n=int(loci.size), samples=len(slices), pcount=pcount,
                          max_cpg=max_cpg, max_bp=max_bp, chunks=[list(c) for c in chunks], borders=borders)
    print('seed %-3d n=%-5d N=%d pcount=%-12g max_cpg=%-4d max_bp=%-6d borders=%s' % (seed, loci.size, len(slices), pcount, max_cpg, max_bp,
                                                                                       [len(b) for b in borders]), flush=True)
with open(op.join(HERE, 'random_world_cases.json'), 'w') as f:
    json.dump(out, f, separators=(',', ':'))
