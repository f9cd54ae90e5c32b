"""Plain-Python restatement of what `wgbstools beta2bed` prints (the reference's beta2bed.py:11-19 over view_beta.sh's lines), for
the tests: the base lines, the three awk filters, and this build's `-L` rule with ONE plain comparison per bed row (no
searchsorted), so that the product's multiplicity builder is held against something written differently."""
import numpy as np


def chrom_of_sites(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


def multiplicity_by_rows(names, sizes, loci, bed_text):
    """per site of the genome: the number of bed rows (chrom, start, end) on its chromosome with start <= loc <= end"""
    loci = np.asarray(loci, dtype=np.int64)
    chrom = chrom_of_sites(sizes)
    mult = np.zeros(loci.size, dtype=np.int64)
    for line in bed_text.splitlines():
        if not line.strip() or line.startswith('#'):
            continue
        c, a, b = line.split('\t')[:3]
        if c in names:
            mult += (chrom == names.index(c)) & (loci >= int(a)) & (loci <= int(b))
    return mult


def ratio_text(meth, cov):
    """awk's printf "%.3g" of meth / cov: C's conversion of the double, which Python's % operator calls too"""
    return '%.3g' % (float(meth) / float(cov))


def text_of(names, sizes, loci, rows, start0, end0, mult=None, min_cov=1, mean=False, keep_na=False):
    """the bytes of the sites [start0, end0) (0-based), mult[i] copies of site start0 + i"""
    chrom = chrom_of_sites(sizes)
    out = []
    for i in range(start0, end0):
        k = 1 if mult is None else int(mult[i - start0])
        if k == 0:
            continue
        meth, cov = int(rows[i, 0]), int(rows[i, 1])
        if min_cov > 1 and cov < min_cov:
            meth = cov = 0
        if not keep_na and cov == 0:
            continue
        loc = int(loci[i])
        head = '%s\t%d\t%d\t' % (names[chrom[i]], loc - 1, loc + 1)
        if mean:
            line = head + (ratio_text(meth, cov) if cov > 0 else '-1') + '\n'
        else:
            line = head + '%d\t%d\n' % (meth, cov)
        out.append(line * k)
    return ''.join(out).encode()


def case_text(world, case, sites=None, bed_text=None):
    """the expected bytes of a case of bed_cases.cases(): `sites` = the 1-based [s1, s2) of its -s / -r, `bed_text` its bed file"""
    rows = world['files'][case['file']]
    n = len(world['loci'])
    start0, end0, mult = 0, n, None
    if bed_text is not None:
        mult = multiplicity_by_rows(world['names'], world['sizes'], world['loci'], bed_text)
    elif sites is not None:
        start0, end0 = sites[0] - 1, sites[1] - 1
    return text_of(world['names'], world['sizes'], world['loci'], rows, start0, end0, mult, **case['opts'])
