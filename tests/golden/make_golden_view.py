#!/usr/bin/env python3
"""Golden output of `wgbstools view` from the REFERENCE'S OWN TOOLS: the cases of tests/view_cases.py through the reference's cview,
compiled from src/cview/cview.cpp and src/pipeline_wgbs/patter_utils.cpp into a temporary directory, then `sort -k2,2n -k3,3` where
the reference sorts (cview.py:43-44: a region or a site range, without --no_sort), then `perl src/collapse_pat.pl -`, all under
LC_ALL=C.  Runs only where a checkout of the reference lies: REF_ROOT=<its root> python tests/golden/make_golden_view.py.

Per case the pat text goes on cview's standard input — the reference's `gunzip -c` branch (cview.py:31; the tabix branch needs an index
and htslib) — with `--sites "s\\te"`; the whole genome is [1, nr_sites + 1).  For -s / -r the CpG span is taken from this package's
GenomicRegion over the tiny genome of frag_cases.genome_dir (its conversion has goldens of its own, tests/golden/convert_cases.json).

Writes tests/golden/view_cases.json: per case the selecting arguments, the flags, the site pair, the sha1 of the pat text and the
full stdout."""
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

import view_cases as VC                            # noqa: E402

ENV = dict(os.environ, LC_ALL='C')


def build_tool(tmp):
    obj1, obj2, exe = op.join(tmp, 'cview.o'), op.join(tmp, 'patter_utils.o'), op.join(tmp, 'cview')
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj1, op.join(REF, 'src', 'cview', 'cview.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj2, op.join(REF, 'src', 'pipeline_wgbs', 'patter_utils.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-o', exe, obj1, obj2])
    return exe


def run(cmd, text):
    return subprocess.run(cmd, shell=True, executable='/bin/bash', input=text, stdout=subprocess.PIPE, check=True, env=ENV).stdout.decode()


def main():
    from wgbs_tools_amd.genome import GenomeRefPaths, GenomicRegion
    tmp = tempfile.mkdtemp(prefix='view_golden_')
    out = {}
    try:
        exe = build_tool(tmp)
        ref, _ = VC.genome_dir(tmp)
        genome = GenomeRefPaths(ref)
        collapse = 'perl ' + op.join(REF, 'src', 'collapse_pat.pl') + ' -'
        for name, case in VC.CASES.items():
            text = VC.case_pat(case)
            where, flags = VC.case_where(case), list(case['flags'])
            if not where:
                s, e = 1, genome.get_nr_sites() + 1
            else:
                gr = GenomicRegion(sites=where[1], genome=genome) if where[0] == '-s' else GenomicRegion(region=where[1], genome=genome)
                s, e = gr.sites
            tool_flags = ' '.join(f for f in flags if f != '--no_sort').replace('--min_len', '--min_cpgs')       # (cview.py:69-79)
            cmd = f'{exe} --sites "{s}\t{e}" {tool_flags}'
            sorts = bool(where) and '--no_sort' not in flags
            if sorts:
                cmd += ' | sort -k2,2n -k3,3'
            cmd += ' | ' + collapse
            stdout = run(cmd, text)
            out[name] = dict(where=where, flags=flags, sites=[int(s), int(e)], sorted=sorts, pat_sha1=hashlib.sha1(text).hexdigest(), stdout=stdout)
            print(name, s, e, stdout.count('\n'), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'view_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
