#!/usr/bin/env python3
"""Golden lines of `wgbstools frag_len` from the REFERENCE'S OWN TOOLS: the cases of tests/frag_cases.py through the reference's
cview, compiled from src/cview/cview.cpp and src/pipeline_wgbs/patter_utils.cpp into a temporary directory, into the awk program of
the reference's frag_len.py (imported; the program's text is read off a FragLen object at run time, nothing of it is written here),
under LC_ALL=C.  Runs only where a checkout of the reference lies: REF_ROOT=<its root> python tests/golden/make_golden_frag.py.

Per case the pat text goes on cview's standard input — the reference's `gunzip -c` branch (cview.py:88-89; the tabix branches need
an index and htslib) — with `--sites "s\\te"` for -s / -r and `--blocks_path FILE` for -L; whole-genome cases go straight into the
awk program (the reference runs it once per chromosome behind tabix and adds the results: the same sums).  For -s / -r the CpG span
is taken from this package's GenomicRegion over the tiny genome of frag_cases.genome_dir (its conversion has goldens of its own,
tests/golden/convert_cases.json).  The awk output becomes the line the reference prints with -v as frag_len.py:15-18,:82-88 do it:
empty fields are 0, an all-zero result prints nothing.

Writes tests/golden/frag_cases.json: per case m, the selecting arguments (a blocks table as its text), the sha1 of the pat text, the
line, and for block lists the order cview's own `sort -k1,1n` gave them.  Every sum stays below 2^31 (asserted)."""
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
if not op.isdir(op.join(REF, 'src', 'cview')):
    sys.exit('set REF_ROOT to the root of a wgbs_tools checkout')
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, op.join(REF, 'src', 'python'))

import frag_cases as FC                            # noqa: E402

ENV = dict(os.environ, LC_ALL='C')


def build_tool(tmp):
    obj1, obj2, exe = op.join(tmp, 'cview.o'), op.join(tmp, 'patter_utils.o'), op.join(tmp, 'cview')
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj1, op.join(REF, 'src', 'cview', 'cview.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj2, op.join(REF, 'src', 'pipeline_wgbs', 'patter_utils.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-o', exe, obj1, obj2])
    return exe


def awk_tail(m):
    """' | awk ...' of the reference for --max_frag_size m"""
    import frag_len as rf

    class Args:
        max_frag_size = m
    return rf.FragLen('unused', Args, gr=object()).awk_hist_cmd


def run(cmd, text):
    return subprocess.run(cmd, shell=True, executable='/bin/bash', input=text, stdout=subprocess.PIPE, check=True, env=ENV).stdout.decode()


def main():
    from wgbs_tools_amd.genome import GenomeRefPaths, GenomicRegion
    tmp = tempfile.mkdtemp(prefix='frag_golden_')
    out = {}
    try:
        exe = build_tool(tmp)
        ref, _ = FC.genome_dir(tmp)
        genome = GenomeRefPaths(ref)
        for name, case in FC.CASES.items():
            text = FC.case_pat(case)
            where = FC.case_where(case)
            rec = dict(m=case['m'], where=where, pat_sha1=hashlib.sha1(text).hexdigest())
            if not where:
                front = 'cat'
            elif where[0] == '-L':
                bpath = op.join(tmp, name + '.bed')
                with open(bpath, 'w') as f:
                    f.write(where[1])
                front = f'{exe} --blocks_path {bpath}'
                rec['order'] = run(f'cut -f4-5 {bpath} | sort -k1,1n', b'').splitlines()
            else:
                gr = GenomicRegion(sites=where[1], genome=genome) if where[0] == '-s' else GenomicRegion(region=where[1], genome=genome)
                s, e = gr.sites
                rec['sites'] = [int(s), int(e)]
                front = f'{exe} --sites "{s}\t{e}"'
            rec['passed'] = run(front, text).count('\n')
            vals = [int(r) if r else 0 for r in run(front + awk_tail(case['m']), text).split('\n')[:-1]]
            assert len(vals) == case['m'] and all(abs(v) < 2 ** 31 for v in vals), name
            rec['stdout'] = ' '.join(str(v) for v in vals) + '\n' if sum(vals) else ''
            out[name] = rec
            print(name, rec['passed'], rec['stdout'][:100].rstrip(), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'frag_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
