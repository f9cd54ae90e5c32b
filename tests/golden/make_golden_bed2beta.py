#!/usr/bin/env python3
"""Golden output of `wgbstools bed2beta` from the REFERENCE'S OWN FUNCTIONS: the cases of tests/bed2beta_cases.py.

Per case the BED text is written to a file, read with the reference's bed2beta.load_bed (the header peek, drop_duplicates, --add_one),
left-merged into the dictionary frame of the tiny genome of frag_cases.genome_dir — the frame utils_wgbs.load_dict reads from its
CpG.bed.gz: chr, start, idx — and trimmed with the reference's utils_wgbs.trim_to_uint8, as bed2beta.bed2betas does for the whole
genome (bed2beta.py:43-51).  Recorded: the text's sha1, the flags, the sha1 of the resulting bytes and the non-zero rows.

Runs only where a checkout of the reference lies: REF_ROOT=<its root> python tests/golden/make_golden_bed2beta.py.
Writes tests/golden/bed2beta_cases.json."""
import hashlib
import json
import os
import os.path as op
import shutil
import sys
import tempfile

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
REF = os.environ.get('REF_ROOT', '')
if not op.isfile(op.join(REF, 'src', 'python', 'bed2beta.py')):
    sys.exit('set REF_ROOT to the root of a wgbs_tools checkout')
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, op.join(REF, 'src', 'python'))

import numpy as np                                 # noqa: E402
import pandas as pd                                # noqa: E402

import bed2beta_cases as BC                        # noqa: E402
import frag_cases as FC                            # noqa: E402
from bed2beta import load_bed                      # noqa: E402  (the reference's)
from utils_wgbs import trim_to_uint8               # noqa: E402  (the reference's)


def main():
    tmp = tempfile.mkdtemp(prefix='bed2beta_golden_')
    out = {}
    try:
        ref, _ = FC.genome_dir(tmp)
        rf = pd.read_csv(op.join(ref, 'CpG.bed.gz'), header=None, names=['chr', 'start'], sep='\t', usecols=[0, 1])      # (what load_dict reads)
        rf['idx'] = rf.index + 1
        assert rf.shape[0] == BC.N_SITES
        for name, case in BC.CASES.items():
            text = BC.case_text(case)
            path = op.join(tmp, name + '.bed')
            with open(path, 'wb') as f:
                f.write(text)
            df = load_bed(path, None, bool(case.get('add_one')))
            res = rf.merge(df, how='left', on=['chr', 'start']).fillna(0)
            rows = trim_to_uint8(np.array(res[['meth', 'total']]))
            assert rows.shape == (BC.N_SITES, 2) and rows.dtype == np.uint8
            out[name] = dict(text_sha1=hashlib.sha1(text).hexdigest(), flags=BC.case_flags(case), n_sites=BC.N_SITES,
                             out_sha1=hashlib.sha1(np.ascontiguousarray(rows).tobytes()).hexdigest(), rows=BC.sparse(rows))
            print(name, len(out[name]['rows']), out[name]['out_sha1'], flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'bed2beta_cases.json'), 'w') as f:
        json.dump(out, f, indent=None, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main()
