#!/usr/bin/env python3
"""Golden vectors of `wgbstools homog` from the REFERENCE ITSELF: the cases of tests/homog_cases.py through the reference's own
homog.py (src/python/homog.py, imported) driving its own homog binary, compiled from src/homog/homog.cpp and
src/pipeline_wgbs/patter_utils.cpp with the reference's build line (setup.py:62-64) into a temporary directory.  Runs only
where a checkout of the reference lies: REF_ROOT=<its root> python tests/golden/make_golden_homog.py.  Every case goes through the reference's full-file branch
(`gunzip -c` into the tool: view_full=True; with more than 5,000 blocks that is its own choice, below it the cview branch
is bypassed — see the deviations in wgbs_tools_amd/homog.py).  Empty .csi files satisfy validate_file_list.

Writes tests/golden/homog_cases.json: per case the generator parameters, the arguments, the sha1 of the pat text, and the
sha1 of the DECOMPRESSED .uxm.bed.gz text (gzip headers carry timestamps) or of the --binary bytes, and the first rows."""
import gzip
import hashlib
import json
import os
import os.path as op
import shutil
import subprocess
import sys
import tempfile

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
REF = os.environ.get('REF_ROOT', '')
if not op.isdir(op.join(REF, 'src', 'homog')):
    sys.exit('set REF_ROOT to the root of a wgbs_tools checkout')
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, op.join(REF, 'src', 'python'))

import homog_cases as HC                           # noqa: E402


def build_tool(tmp):
    obj1, obj2, exe = op.join(tmp, 'homog.o'), op.join(tmp, 'patter_utils.o'), op.join(tmp, 'homog')
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj1, op.join(REF, 'src', 'homog', 'homog.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj2, op.join(REF, 'src', 'pipeline_wgbs', 'patter_utils.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-o', exe, obj1, obj2])
    return exe


def main():
    import homog as rh
    import utils_wgbs as ru
    tmp = tempfile.mkdtemp(prefix='homog_golden_')
    try:
        exe = build_tool(tmp)
        rh.homog_tool = exe
        ru.homog_tool = exe
        orig = rh.ctool_wrap
        rh.ctool_wrap = lambda pat, name, bp, rc, view_full, *a, **k: orig(pat, name, bp, rc, True, *a, **k)
        out = {}
        for name, case in HC.CASES.items():
            d = op.join(tmp, name)
            os.makedirs(d)
            pat_text = HC.case_pat(case['pat'])
            _, _, btext = HC.case_blocks(case['blocks'])
            pat = op.join(d, 'smp.pat.gz')
            with gzip.open(pat, 'wb') as f:
                f.write(pat_text)
            open(pat + '.csi', 'w').close()
            blocks = op.join(d, 'blocks.bed')
            with open(blocks, 'w') as f:
                f.write(btext)
            argv = ['homog', pat, '-b', blocks, '-o', d] + case['args']
            saved = sys.argv
            sys.argv = argv
            try:
                rh.main()
            finally:
                sys.argv = saved
            rec = dict(pat=case['pat'], blocks=case['blocks'], args=case['args'], pat_sha1=hashlib.sha1(pat_text).hexdigest())
            if '--binary' in case['args']:
                b = open(op.join(d, 'smp.uxm'), 'rb').read()
                rec['bin_sha1'] = hashlib.sha1(b).hexdigest()
                rec['bin_len'] = len(b)
            else:
                with gzip.open(op.join(d, 'smp.uxm.bed.gz'), 'rb') as f:
                    txt = f.read()
                rec['text_sha1'] = hashlib.sha1(txt).hexdigest()
                rec['rows'] = txt.count(b'\n')
                rec['head'] = txt.decode().splitlines()[:12]
            out[name] = rec
            print(name, {k: v for k, v in rec.items() if k in ('text_sha1', 'bin_sha1', 'rows', 'bin_len')}, flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'homog_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
