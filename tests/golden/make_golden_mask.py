#!/usr/bin/env python3
"""Golden output of `wgbstools mask_pat` from the REFERENCE'S OWN TOOLS: the cases of tests/mask_cases.py.

Per case the reference's pipe (mask_pat.py:25-36 over cview.py:25-52) under LC_ALL=C,
    cview --sites "s\te" < PAT [| sort -k2,2n -k3,3] | perl collapse_pat.pl - | mask_pat SITES.bed | sort -k2,2n -k3,3 | perl collapse_pat.pl -
with cview compiled from src/cview/cview.cpp and mask_pat from src/pat2beta/mask_pat.cpp (both with src/pipeline_wgbs/patter_utils.cpp) into
a temporary directory, the pat text on cview's standard input (the `gunzip -c` branch of cview.py) and the blocks table in a file.  The
sort inside cview.py runs for an interval only, as there.  The interval of a case comes from this build's GenomicRegion over the tiny
genome of frag_cases.genome_dir; the whole genome is [1, nr_sites + 1).

Runs only where a checkout of the reference lies: REF_ROOT=<its root> python tests/golden/make_golden_mask.py.
Writes tests/golden/mask_cases.json: per case the inputs' sha1, the interval, what mask_pat printed on stderr about its sites, and the output."""
import hashlib
import json
import os
import os.path as op
import re
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

import mask_cases as KC                            # noqa: E402

ENV = dict(os.environ, LC_ALL='C')


def build_tools(tmp):
    utils = op.join(tmp, 'patter_utils.o')
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', utils, op.join(REF, 'src', 'pipeline_wgbs', 'patter_utils.cpp')])
    exes = []
    for name, src in (('cview', op.join(REF, 'src', 'cview', 'cview.cpp')), ('mask_pat', op.join(REF, 'src', 'pat2beta', 'mask_pat.cpp'))):
        obj, exe = op.join(tmp, name + '.o'), op.join(tmp, name)
        subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj, src])
        subprocess.check_call(['g++', '-std=c++11', '-o', exe, obj, utils])
        exes.append(exe)
    return exes


def main():
    from wgbs_tools_amd.genome import GenomeRefPaths, GenomicRegion
    tmp = tempfile.mkdtemp(prefix='mask_golden_')
    out = {}
    try:
        cview, mask = build_tools(tmp)
        genome = GenomeRefPaths(KC.genome_dir(tmp)[0])
        collapse = 'perl ' + op.join(REF, 'src', 'collapse_pat.pl') + ' -'
        for name, case in KC.CASES.items():
            pat, table, where = KC.case_pat(case), KC.case_table(case).encode(), KC.case_where(case)
            pat_path, bed_path, err_path = op.join(tmp, name + '.pat'), op.join(tmp, name + '.bed'), op.join(tmp, name + '.err')
            with open(pat_path, 'wb') as f:
                f.write(pat)
            with open(bed_path, 'wb') as f:
                f.write(table)
            if not where:
                s, e, inner_sort = 1, genome.get_nr_sites() + 1, ''
            else:
                gr = GenomicRegion(sites=where[1], genome=genome) if where[0] == '-s' else GenomicRegion(region=where[1], genome=genome)
                (s, e), inner_sort = gr.sites, ' | sort -k2,2n -k3,3'
            cmd = (f'{cview} --sites "{s}\t{e}" < {pat_path}{inner_sort} | {collapse} | {mask} {bed_path} 2> {err_path}'
                   f' | sort -k2,2n -k3,3 | {collapse}')
            stdout = subprocess.run(cmd, shell=True, executable='/bin/bash', stdout=subprocess.PIPE, check=True, env=ENV).stdout.decode()
            with open(err_path) as f:
                err = f.read()
            assert 'failed' not in err, (name, err)
            loaded = int(re.search(r'loaded (\d+) sites', err).group(1))
            out[name] = dict(where=where, sites=[int(s), int(e)], pat_sha1=hashlib.sha1(pat).hexdigest(), table_sha1=hashlib.sha1(table).hexdigest(),
                             loaded=loaded, stdout=stdout)
            print(name, s, e, loaded, stdout.count('\n'), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'mask_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
