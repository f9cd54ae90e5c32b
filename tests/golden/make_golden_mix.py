#!/usr/bin/env python3
"""Golden output of `wgbstools mix_pat` from the REFERENCE'S OWN TOOLS: the cases of tests/mix_cases.py.

The reference's sampler seeds itself from the clock, so its draws cannot be recorded.  Per case every input's lines are therefore drawn
first, by tests/mix_ref.py, keyed on the byte offsets of the ORIGINAL text (sampling before the cut says the same as after it: the cut
never reads the count); the drawn text then goes through the reference's pipeline (merge.py:76-100 fast_merge_pats with labels) under
LC_ALL=C,
    sort -m -k2,2n -k3,3 <(cview --sites ... | sort -k2,2n -k3,3 | perl collapse_pat.pl - | sed 's/$/\\tLABEL/') ... | perl collapse_pat.pl -
with cview compiled from src/cview/cview.cpp and src/pipeline_wgbs/patter_utils.cpp into a temporary directory.  This pins the order of
tied lines and the label column against the real `sort` and Perl.  A whole-genome case runs chromosome by chromosome over the tiny genome
of frag_cases.genome_dir and concatenates (merge.py:105-120 merge_by_chrom).

Runs only where a checkout of the reference lies: REF_ROOT=<its root> python tests/golden/make_golden_mix.py.
Writes tests/golden/mix_cases.json: per case the inputs' sha1, the sampler's arguments and the output."""
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

import mix_cases as XC                             # noqa: E402
import mix_ref as MX                               # noqa: E402

ENV = dict(os.environ, LC_ALL='C')


def build_tool(tmp):
    obj1, obj2, exe = op.join(tmp, 'cview.o'), op.join(tmp, 'patter_utils.o'), op.join(tmp, 'cview')
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj1, op.join(REF, 'src', 'cview', 'cview.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-c', '-o', obj2, op.join(REF, 'src', 'pipeline_wgbs', 'patter_utils.cpp')])
    subprocess.check_call(['g++', '-std=c++11', '-o', exe, obj1, obj2])
    return exe


def run(cmd):
    return subprocess.run(cmd, shell=True, executable='/bin/bash', stdout=subprocess.PIPE, check=True, env=ENV).stdout.decode()


def main():
    from wgbs_tools_amd.genome import GenomeRefPaths, GenomicRegion
    tmp = tempfile.mkdtemp(prefix='mix_golden_')
    out = {}
    try:
        exe = build_tool(tmp)
        ref, _ = XC.genome_dir(tmp)
        genome = GenomeRefPaths(ref)
        collapse = 'perl ' + op.join(REF, 'src', 'collapse_pat.pl') + ' -'
        for name, case in XC.CASES.items():
            texts, per_file = XC.case_files(case), XC.per_file(case)
            paths = []
            for k, text in enumerate(texts):
                T, reps = per_file[k]
                paths.append(op.join(tmp, '%s_%d.pat' % (name, k)))
                with open(paths[-1], 'wb') as f:
                    f.write(MX.sample_text(text, T, reps, case['seed'], MX.stream_of(case['rep'], k)))
            where, flags = XC.case_where(case), list(case['flags'])
            if not where:
                spans = [tuple(GenomicRegion(region=c, genome=genome).sites) for c in genome.get_chroms()]
                s, e = 1, genome.get_nr_sites() + 1
            else:
                gr = GenomicRegion(sites=where[1], genome=genome) if where[0] == '-s' else GenomicRegion(region=where[1], genome=genome)
                spans = [tuple(gr.sites)]
                s, e = gr.sites
            tool_flags = ' '.join(flags).replace('--min_len', '--min_cpgs')                                      # (cview.py:69-79)
            stdout = ''
            for a, b in spans:
                views = ' '.join(f"<({exe} --sites \"{a}\t{b}\" {tool_flags} < {p} | sort -k2,2n -k3,3 | {collapse} | sed 's/$/\\t{lab}/')"
                                 for p, lab in zip(paths, case['labels']))
                stdout += run(f'sort -m -k2,2n -k3,3 {views} | {collapse}')
            out[name] = dict(where=where, flags=flags, sites=[int(s), int(e)], passes=[[int(a), int(b)] for a, b in spans],
                             pat_sha1=[hashlib.sha1(t).hexdigest() for t in texts], labels=case['labels'], per_file=[list(x) for x in per_file],
                             seed=case['seed'], rep=case['rep'], stdout=stdout)
            print(name, s, e, len(spans), stdout.count('\n'), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'mix_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
