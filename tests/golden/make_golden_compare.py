#!/usr/bin/env python3
"""Golden histograms of `wgbstools compare_betas` from the REFERENCE ITSELF: runs only in the build container, imports
/root/reference/src/python/compare_betas.py from where it lies and calls its comp2 on an Agg axes for the small seeded cases
of tests/compare_cases.py (golden_cases: <= 200 sites, <= 7 bins, uint8 and uint16 rows).  What comp2 drew is read back from
the axes: the mesh's array (counts, transposed as drawn), its coordinates (the edges) and the axis limits.

Usage:  python tests/golden/make_golden_compare.py
"""
import json
import os.path as op
import sys

import matplotlib
matplotlib.use('Agg')
import matplotlib.pyplot as plt          # noqa: E402
import numpy as np                        # noqa: E402

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference/src/python')

import compare_cases as CC                # noqa: E402
from compare_betas import comp2           # noqa: E402  (the reference's)


def main():
    out = {}
    for name, (a, b, min_cov, bins) in CC.golden_cases().items():
        fig, ax = plt.subplots()
        comp2(a, b, min_cov, bins, ax)
        mesh, = ax.collections
        arr = np.ma.filled(mesh.get_array(), np.nan).reshape(bins, bins)
        coords = np.asarray(mesh.get_coordinates())
        assert np.isfinite(arr).all() and (arr == np.rint(arr)).all()
        assert (coords[:, :, 0] == coords[0, :, 0]).all() and (coords[:, :, 1] == coords[:, :1, 1]).all()
        out[name] = dict(min_cov=min_cov, bins=bins, n_sites=int(a.shape[0]),
                         drawn=[[int(v) for v in row] for row in arr],              # [y_cell][x_cell]
                         xedges=[float(v) for v in coords[0, :, 0]], yedges=[float(v) for v in coords[:, 0, 1]],
                         xlim=[float(v) for v in ax.get_xlim()], ylim=[float(v) for v in ax.get_ylim()])
        plt.close(fig)
    path = op.join(HERE, 'compare_cases.json')
    with open(path, 'w') as f:
        json.dump(dict(note='what the reference\'s comp2 drew for tests/compare_cases.py golden_cases()', cases=out), f, indent=1)
        f.write('\n')
    print('wrote', path, len(out), 'cases')


if __name__ == '__main__':
    main()
