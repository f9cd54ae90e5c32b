#!/usr/bin/env python3
"""Golden output of `wgbstools init_genome` from the REFERENCE'S OWN FUNCTIONS: the cases of tests/init_genome_cases.py through
init_genome.py's load_seq_by_chrom, is_valid_chrome and chromosome_order, the frames assembled and dumped as InitGenome.load_fai() and
InitGenome.run() do it (init_genome.py:131-137, 155-179, 241-243).  Runs only where a checkout of the reference lies:
REF_ROOT=<its root> python tests/golden/make_golden_init_genome.py.

load_seq_by_chrom asks `samtools faidx FASTA CHROM | tail -n +2` for a chromosome's lines; a stand-in of our own, first on PATH, prints
the record's lines as they lie in the file.  The .fai table (names and sizes in FASTA order) is made here: a name is what follows '>'
up to the first blank, a size is the bytes of the record's sequence lines without '\\n' and '\\r'.

Writes tests/golden/init_genome_cases.json: per case the text's sha1, --no_sort, and the sha1 and the text of CpG.bed, chrome.size and
CpG.chrome.size, and the loci."""
import hashlib
import io
import json
import os
import os.path as op
import shutil
import stat
import sys
import tempfile

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
REF = os.environ.get('REF_ROOT', '')
SRC = op.join(REF, 'src', 'python')
if not op.isfile(op.join(SRC, 'init_genome.py')):
    sys.exit('set REF_ROOT to the root of a wgbs_tools checkout')
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, SRC)

import pandas as pd                                # noqa: E402
import init_genome as RG                           # noqa: E402  (the reference's)
import init_genome_cases as GC                     # noqa: E402

SAMTOOLS = """#!/bin/sh
# stand-in for `samtools faidx FASTA CHROM`: the lines of CHROM's record as they lie
exec awk -v c="$3" '/^>/ { name = substr($0, 2); sub(/[ \\t\\r].*/, "", name); on = (name == c) } on { print }' "$2"
"""


def fai(text):
    rows = []
    for line in text.split(b'\n'):
        if line.startswith(b'>'):
            name = line[1:]
            for blank in (b' ', b'\t', b'\r'):
                name = name.split(blank)[0]
            rows.append([name.decode(), 0])
        elif rows:
            rows[-1][1] += len(line.replace(b'\r', b''))
    return pd.DataFrame(rows, columns=['chr', 'size'])


def dump(df):
    """InitGenome.dump_df"""
    buf = io.StringIO()
    df.to_csv(buf, index=None, header=False, sep='\t')
    return buf.getvalue()


def one(text, no_sort, tmp):
    fa = op.join(tmp, 'x.fa')
    with open(fa, 'wb') as f:
        f.write(text)
    df = fai(text)
    df = df[df.apply(lambda x: RG.is_valid_chrome(x['chr']), axis=1)] if len(df) else df         # load_fai
    if not no_sort and len(df):
        df = pd.DataFrame(sorted(df['chr'], key=RG.chromosome_order), columns=['chr']).merge(df, how='left')
    fai_df = df
    arr = [RG.load_seq_by_chrom(fa, c) for c in fai_df['chr']]                                   # find_cpgs_loci
    cpg = pd.concat(arr).reset_index(drop=True) if arr else pd.DataFrame(columns=['chr', 'loc'])
    cpg['site'] = cpg.index + 1                                                                  # run
    ncgs = fai_df[['chr']].copy()
    t = cpg.groupby('chr')['loc'].nunique().to_frame().reset_index().rename(columns={'loc': 'size'})
    ncgs = ncgs.merge(t, on='chr', how='left').fillna(0)
    ncgs['size'] = ncgs['size'].astype(int)
    texts = dict(cpg_bed=dump(cpg), chrome_size=dump(fai_df[['chr', 'size']]), cpg_chrome_size=dump(ncgs[['chr', 'size']]))
    out = dict(text_sha1=hashlib.sha1(text).hexdigest(), no_sort=bool(no_sort), loci=[int(x) for x in cpg['loc']])
    for k, v in texts.items():
        out[k] = v
        out[k + '_sha1'] = hashlib.sha1(v.encode()).hexdigest()
    return out


def main():
    tmp = tempfile.mkdtemp(prefix='init_genome_golden_')
    out = {}
    try:
        bindir = op.join(tmp, 'bin')
        os.mkdir(bindir)
        exe = op.join(bindir, 'samtools')
        with open(exe, 'w') as f:
            f.write(SAMTOOLS)
        os.chmod(exe, os.stat(exe).st_mode | stat.S_IXUSR)
        os.environ['PATH'] = bindir + os.pathsep + os.environ.get('PATH', '')
        got = RG.load_seq_by_chrom(_write(tmp, b'>chr1\nacgtC\nGNNc\r\ng'), 'chr1')['loc'].tolist()
        assert got == [2, 5, 9], got
        for name, (text, no_sort) in GC.CASES.items():
            out[name] = one(text, no_sort, tmp)
            print(name, len(text), len(out[name]['loci']), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(op.join(HERE, 'init_genome_cases.json'), 'w') as f:
        json.dump(out, f, indent=1)


def _write(tmp, text):
    path = op.join(tmp, 'probe.fa')
    with open(path, 'wb') as f:
        f.write(text)
    return path


if __name__ == '__main__':
    main()
