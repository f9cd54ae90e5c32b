#!/usr/bin/env python3
"""Golden text of `wgbstools beta2bed` from the REFERENCE ITSELF: runs only in the build container.  Imports
/root/reference/src/python/beta2bed.py from where it lies, asks its beta2bed_build_cmd for the shell command of every case of
tests/bed_cases.py and RUNS that command with bash, awk, paste and gzip as they are installed.  Two tools of the pipeline are not
installed; stand-ins on the PATH speak exactly what the two view scripts say to them (the fixture records which were used):

    tabix     TABIX_SHIM of make_golden_convert.py
    hexdump   HEXDUMP_SHIM below: `hexdump [-s N] [-n N] -v -e '/K "%u\\t" /K "%u\\n"' FILE`, K = 1 or 2, nothing else

`-L` cases need `bedtools intersect -a stdin -b BED -wa`, which is not installed either (`bedtools_for_L: false`): their expected
text is the whole genome's base lines as the reference's view script prints them, each repeated once for every bed row on its
chromosome with start <= loc <= end (tests/bed_ref.py counts them with one plain comparison per row), piped through the
reference's REAL awk stages — the part of beta2bed_build_cmd's command behind the view command.

Every recorded text is also held against tests/bed_ref.py's restatement here, so a disagreement shows when the fixture is made.

ONE PLACE WHERE THE INSTALLED awk IS NOT THE RULE.  The awk here is mawk 1.3.4, which prints an integer-valued number above
2^31 - 1 with OFMT ("%.6g": 2158525740 comes out as 2.15853e+09) and clamps printf "%d" there; gawk and the one-true-awk print
such numbers in full, and loc - 1 / loc + 1 as plain integers is what the command is specified to print.  Only the small world's
last ~90 sites (loci from 2^31 up to 4,294,967,294) are concerned; no real chromosome is that long.  For those lines the fixture
records the plain integers; the reference's real output is still checked in full: it must equal the recorded text once
mawk's two conversions (mawk_numbers below) are applied to the recorded text's second and third column.  `awk_integers` in the
fixture says whether the installed awk needed that, and every case counts the lines concerned (`lines_beyond_int32`).
Texts of at most FULL_TEXT bytes are stored whole; longer ones as sha1, byte and line counts and their first and last three lines.

Usage:  python tests/golden/make_golden_beta2bed.py
"""
import argparse
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
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
sys.path.insert(0, '/root/reference/src/python')

import bed_cases as BC                          # noqa: E402
import bed_ref as BR                            # noqa: E402
from make_golden_convert import TABIX_SHIM      # noqa: E402

FULL_TEXT = 24 << 10

HEXDUMP_SHIM = r'''#!/usr/bin/env python3
import array, re, sys
a, skip, count, fmt, path, i = sys.argv[1:], 0, None, None, None, 0
while i < len(a):
    if a[i] == '-s': skip = int(a[i + 1]); i += 2
    elif a[i] == '-n': count = int(a[i + 1]); i += 2
    elif a[i] == '-v': i += 1
    elif a[i] == '-e': fmt = a[i + 1]; i += 2
    else: path = a[i]; i += 1
m = re.fullmatch(r'/([12]) "%u\\t" /([12]) "%u\\n"', fmt or '')
if not m or m.group(1) != m.group(2) or path is None:
    sys.exit('hexdump stand-in: unsupported call: %r' % (a,))
with open(path, 'rb') as f:
    f.seek(skip)
    data = f.read() if count is None else f.read(count)
k = int(m.group(1))
v = array.array('B' if k == 1 else 'H', data[:len(data) // (2 * k) * 2 * k])
try:
    sys.stdout.write(''.join('%d\t%d\n' % (v[j], v[j + 1]) for j in range(0, len(v), 2)))
except BrokenPipeError:
    pass
'''


def put_tool(directory, name, text):
    path = op.join(directory, name)
    with open(path, 'w') as f:
        f.write(text)
    os.chmod(path, os.stat(path).st_mode | stat.S_IEXEC)


def shell(cmd):
    return subprocess.run(cmd, shell=True, executable='/bin/bash', check=True, stdout=subprocess.PIPE).stdout


INT32_TOP = 2 ** 31 - 1


def awk_prints_large_integers():
    return shell("awk 'BEGIN { print 2147483648 }'").strip() == b'2147483648'


def mawk_numbers(text, mean):
    """`text` as mawk 1.3.4 prints it: `print $2 - 1, $2 + 1` of a value above 2^31 - 1 goes through OFMT = "%.6g"; the --mean stage
    then reads that text back and prints it with "%d", clamped to 2^31 - 1.  -> (the text, the lines it changed)"""
    out, changed = [], 0
    for line in text.split(b'\n')[:-1]:
        t = line.split(b'\t')
        new = []
        for v in (int(t[1]), int(t[2])):
            s = '%d' % v if v <= INT32_TOP else '%.6g' % v
            if mean:
                s = '%d' % min(int(float(s)), INT32_TOP)
            new.append(s.encode())
        changed += new != t[1:3]
        out.append(b'\t'.join([t[0]] + new + t[3:]) + b'\n')
    return b''.join(out), changed


def record(text):
    lines = text.split(b'\n')[:-1]
    if len(text) <= FULL_TEXT:
        return {'text': text.decode()}
    return {'sha1': hashlib.sha1(text).hexdigest(), 'bytes': len(text), 'lines': len(lines),
            'first': [ln.decode() for ln in lines[:3]], 'last': [ln.decode() for ln in lines[-3:]]}


def main():
    import pandas as pd
    import genomic_region as rg
    import beta2bed as rb
    import view as rview
    from utils_wgbs import IllegalArgumentError
    td = tempfile.mkdtemp()
    tools = op.join(td, 'bin')
    os.makedirs(tools)
    used = {'bedtools_for_L': False}
    for name, text in (('tabix', TABIX_SHIM), ('hexdump', HEXDUMP_SHIM)):
        real = shutil.which(name)
        used[name] = real or 'stand-in'
        if not real:
            put_tool(tools, name, text)
    os.environ['PATH'] = tools + os.pathsep + os.environ['PATH']
    used['awk'] = op.realpath(shutil.which('awk'))
    exact_awk = awk_prints_large_integers()
    used['awk_integers'] = 'printed in full' if exact_awk else 'above 2^31 - 1 printed with OFMT and clamped by %d: recorded as plain integers, checked through mawk_numbers'
    worlds = BC.worlds()
    where = {name: BC.write_world(td, name, w) for name, w in worlds.items()}

    class FakeGenome:
        def __init__(self, name=None):
            self.genome = name
            self.w = worlds[name]
            ref = where[name]['ref']
            self.dict_path = op.join(ref, 'CpG.bed.gz')
            self.revdict_path = op.join(ref, 'rev.CpG.bed.gz')
            self.annotations = None
            self.ilmn2cpg_dict = None

        def get_chrom_cpg_size_table(self):
            return pd.DataFrame({'chr': self.w['names'], 'size': self.w['sizes']})

        def get_chrom_size_table(self):
            return pd.read_csv(op.join(where[self.genome]['ref'], 'chrome.size'), sep='\t', header=None, names=['chr', 'size'])

        def get_chroms(self):
            return tuple(self.w['names'])

        def get_nr_sites(self):
            return int(sum(self.w['sizes']))

    rg.GenomeRefPaths = FakeGenome
    rg.get_genome_name = lambda gname: gname          # (the reference looks for its own references/default link first)
    beds = BC.small_beds(worlds['small'])
    fixture = {'seed': BC.SEED, 'stand_ins': used, 'full_text_up_to': FULL_TEXT, 'cases': {}}
    try:
        for name, case in BC.cases().items():
            w, d = worlds[case['world']], where[case['world']]['dir']
            beta = op.join(d, case['file'])
            o = case['opts']
            flag, val = case['where'] or (None, None)
            args = argparse.Namespace(genome=case['world'], sites=val if flag == '-s' else None, region=val if flag == '-r' else None, array_id=None)
            entry = {}
            try:
                gr = rg.GenomicRegion(args)
            except IllegalArgumentError as e:
                entry['error'] = ' '.join(str(a) for a in e.args)
                fixture['cases'][name] = entry
                print('==', name, 'refused:', entry['error'])
                continue
            full = rb.beta2bed_build_cmd(beta, gr, None, o['min_cov'], o['mean'], o['keep_na'])
            if flag == '-L':
                base_cmd = rview.bview_build_cmd(beta, gr, None)
                assert full.startswith(base_cmd)
                mult = BR.multiplicity_by_rows(w['names'], w['sizes'], w['loci'], beds[val])
                lines = shell(base_cmd).split(b'\n')[:-1]
                assert len(lines) == len(mult)
                rep = op.join(td, 'repeated.txt')
                with open(rep, 'wb') as f:
                    f.write(b''.join((ln + b'\n') * int(k) for ln, k in zip(lines, mult)))
                text = shell('cat ' + rep + full[len(base_cmd):])
                ours = BR.case_text(w, case, bed_text=beds[val])
            else:
                text = shell(full)
                if case['gz']:
                    assert shell(full + ' | gzip -c | gunzip -c') == text
                if gr.sites is not None:
                    entry['sites'] = [int(gr.sites[0]), int(gr.sites[1])]
                ours = BR.case_text(w, case, sites=entry.get('sites'))
            if exact_awk:
                assert ours == text, (name, 'tests/bed_ref.py disagrees with the reference')
            else:
                lossy, entry['lines_beyond_int32'] = mawk_numbers(ours, o['mean'])
                assert lossy == text, (name, 'tests/bed_ref.py disagrees with the reference')
            entry.update(record(ours))
            fixture['cases'][name] = entry
            print('==', name, len(text), 'bytes', entry.get('lines_beyond_int32', ''))
    finally:
        shutil.rmtree(td, ignore_errors=True)
    path = op.join(HERE, 'bed_cases.json')
    with open(path, 'w') as f:
        json.dump(fixture, f, indent=0)
    print('wrote bed_cases.json (%.0f KB)' % (op.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
