#!/usr/bin/env python3
"""Golden output of `wgbstools bam2pat` from the REFERENCE'S OWN TOOLS: the cases of tests/bam2pat_cases.py through the reference's
`patter`, compiled from src/pipeline_wgbs/{main,patter,patter_utils,ont}.cpp where they lie into a temporary directory, then what
bam2pat.py:99-106 pipes behind it — `sort -k2,2n -k3,3 | uniq -c | awk` — under LC_ALL=C.  Runs only where a checkout of the reference
lies: REF_ROOT=<its root> python tests/golden/make_golden_bam2pat.py.

`patter` asks `tabix` for the dictionary rows of its chromosome; a stand-in of our own, first on PATH, prints them from a plain-text
copy of the tiny genome's CpG.bed.  What `samtools view -q -F -f` and the awk of --top_strand / --bottom_strand do (bam2pat.py:159-170)
is done here in Python, on the lines whose FLAG and MAPQ are numbers; the survivors are handed to `patter` chromosome by chromosome, as
bam2pat.py does, and the parts are joined in the dictionary's order.  No case may hold a name that continues on its chromosome right
behind lines of another one (bam2pat_cases.names_split_by_other_chromosomes): only there would neighbours in the file differ from
neighbours in the streams.

Writes tests/golden/bam2pat_cases.json: per case the arguments, the sha1 of the SAM text and the stdout."""
import hashlib
import json
import os
import os.path as op
import shutil
import stat
import subprocess
import sys
import tempfile

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
REF = os.environ.get('REF_ROOT', '')
SRC = op.join(REF, 'src', 'pipeline_wgbs')
if not op.isfile(op.join(SRC, 'patter.cpp')):
    sys.exit('set REF_ROOT to the root of a wgbs_tools checkout')
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))

import bam2pat_cases as SC                         # noqa: E402
import bam2pat_ref as BR                           # noqa: E402

TABIX = """#!/bin/sh
# stand-in for `tabix DICT CHROM`: the rows of CHROM from a plain-text dictionary
exec awk -F '\\t' -v c="$2" '$1 == c' "$1"
"""


def build(tmp):
    exe = op.join(tmp, 'patter')
    subprocess.check_call(['g++', '-std=c++11', '-O1', '-o', exe] + [op.join(SRC, f) for f in ('main.cpp', 'patter.cpp', 'patter_utils.cpp', 'ont.cpp')])
    bindir = op.join(tmp, 'bin')
    os.mkdir(bindir)
    tabix = op.join(bindir, 'tabix')
    with open(tabix, 'w') as f:
        f.write(TABIX)
    os.chmod(tabix, os.stat(tabix).st_mode | stat.S_IXUSR)
    dict_path = op.join(tmp, 'CpG.bed')
    with open(dict_path, 'w') as f:
        at = 0
        for chrom, size in SC.CHROMS:
            for k in range(size):
                f.write('%s\t%d\t%d\n' % (chrom, SC.LOCI[at + k], at + k + 1))
            at += size
    return exe, bindir, dict_path


def survivors(text, a):
    out = []
    for line in text.split(b'\n'):
        if not line or line.startswith(b'@'):
            continue
        tok = BR.tokens_of(line)
        if len(tok) >= 11:
            flag, mapq = BR.number(tok[1], 2 ** 31 - 1), BR.number(tok[4], 2 ** 31 - 1)
            if flag is not None and mapq is not None and not BR.keep(flag, mapq, a['paired'], a['exclude'], a['include'], a['mapq'], a['strand']):
                continue
        out.append((tok, line))
    return out


def main():
    tmp = tempfile.mkdtemp(prefix='bam2pat_golden_')
    out = {}
    try:
        exe, bindir, dict_path = build(tmp)
        env = dict(os.environ, LC_ALL='C', PATH=bindir + os.pathsep + os.environ.get('PATH', ''))
        tail = "LC_ALL=C sort -k2,2n -k3,3 | uniq -c | awk -v OFS='\\t' '{print $2,$3,$4,$1}'"
        for name, case in SC.CASES.items():
            text, a = SC.case_text(case), SC.case_args(case)
            alive = survivors(text, a)
            known = [c.encode() for c, _ in SC.CHROMS]                  # (a line of any other chromosome reaches no stream)
            assert not SC.names_split_by_other_chromosomes([(tok[0], tok[2]) for tok, _ in alive if len(tok) >= 3 and tok[2] in known]), name
            stdout = ''
            for chrom, _ in SC.CHROMS:
                part = b''.join(line + b'\n' for tok, line in alive if len(tok) >= 3 and tok[2] == chrom.encode())
                if not part:
                    continue
                cmd = f'{exe} {dict_path} {chrom} --min_cpg {a["min_cpg"]} --clip {a["clip"]} | {tail}'
                r = subprocess.run(cmd, shell=True, executable='/bin/bash', input=part, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, env=env)
                stdout += r.stdout.decode()
            out[name] = dict(args=a, text_sha1=hashlib.sha1(text).hexdigest(), stdout=stdout)
            print(name, len(text), stdout.count('\n'), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'bam2pat_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
