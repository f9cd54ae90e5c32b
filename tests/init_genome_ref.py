"""`wgbstools init_genome` restated in plain Python, the way the reference does it (init_genome.py:131-137, 155-179, 246-281): the records
of the FASTA split at their header lines, every sequence's lines stripped, joined and upper-cased, re.finditer('CG'), the chromosome filter
and the stable sort, then the three texts and the loci.  tests/golden/init_genome_cases.json holds what the reference's own functions
give for tests/init_genome_cases.py; test_init_genome_cpu.py holds this file against it."""
import re

import numpy as np


def records(text):
    """[(name, [sequence lines as they lie])] — a header is a line that begins with '>'; the name ends at the first blank"""
    out = []
    for line in text.decode('latin-1').split('\n'):
        if line.startswith('>'):
            out.append((re.split(r'[ \t\r]', line[1:], maxsplit=1)[0], []))
        elif out:
            out[-1][1].append(line)
    return out


def sequence(lines):
    """init_genome.py:254"""
    return ''.join(s.strip() for s in lines).upper()


def cpg_loci(seq):
    """init_genome.py:257"""
    return [m.start() + 1 for m in re.finditer('CG', seq)]


def is_valid_chrome(chrome):
    return bool(re.match(r'^(chr)?([\d]+|[XYM]|(MT))$', chrome))


def chromosome_order(c):
    if c.startswith('chr'):
        c = c[3:]
    if c.isdigit():
        return int(c)
    if c == 'X':
        return 10000
    if c == 'Y':
        return 10001
    if c in ('M', 'MT'):
        return 10002
    return 10003


def table(text):
    """every sequence in FASTA order: (name, bases, loci)"""
    return [(name, len(sequence(lines)), cpg_loci(sequence(lines))) for name, lines in records(text)]


def init_genome(text, no_sort=False):
    """-> dict(cpg_bed, chrome_size, cpg_chrome_size: the three texts; loci: uint32; chroms: the kept names in order)"""
    kept = [t for t in table(text) if is_valid_chrome(t[0])]
    if not no_sort:
        kept = sorted(kept, key=lambda t: chromosome_order(t[0]))
    bed, site = [], 0
    for name, _, loci in kept:
        for loc in loci:
            site += 1
            bed.append('%s\t%d\t%d\n' % (name, loc, site))
    return dict(cpg_bed=''.join(bed), chrome_size=''.join('%s\t%d\n' % (n, b) for n, b, _ in kept),
                cpg_chrome_size=''.join('%s\t%d\n' % (n, len(l)) for n, _, l in kept),
                loci=np.array([x for _, _, l in kept for x in l], dtype=np.uint32), chroms=[n for n, _, _ in kept])


def assemble(seq_table, loci, order):
    """what a walk found — the sequences in FASTA order (dicts of name, bases, sites) and the loci in FASTA order — as init_genome()
    above returns it, for the sequences `order` keeps"""
    first = np.concatenate([[0], np.cumsum([s['sites'] for s in seq_table])]).astype(np.int64)
    kept = [(seq_table[i]['name'].decode('latin-1'), seq_table[i]['bases'], [int(x) for x in loci[first[i]:first[i + 1]]]) for i in order]
    bed, site = [], 0
    for name, _, sub in kept:
        for loc in sub:
            site += 1
            bed.append('%s\t%d\t%d\n' % (name, loc, site))
    return dict(cpg_bed=''.join(bed), chrome_size=''.join('%s\t%d\n' % (n, b) for n, b, _ in kept),
                cpg_chrome_size=''.join('%s\t%d\n' % (n, len(l)) for n, _, l in kept),
                loci=np.array([x for _, _, l in kept for x in l], dtype=np.uint32), chroms=[n for n, _, _ in kept])
