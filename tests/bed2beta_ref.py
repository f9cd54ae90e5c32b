"""`wgbstools bed2beta` restated twice, for the tests and for tools/bench_bed2beta.py:

bed2beta()         line by line with a dict, the contract as include/wgbsseg.h states it, refusals and counters included: what the GPU
                   engine is compared with.  tests/test_bed2beta_cpu.py pins it to the goldens the reference's own functions wrote
                   (tests/golden/bed2beta_cases.json).
bed2beta_frames()  the way the reference goes about it — the file into a pandas frame, duplicates dropped, the dictionary frame
                   left-merged with it, the big totals trimmed (bed2beta.py:11-51, utils_wgbs.py:277-290) — written against that
                   description: the CPU time the benchmark sets beside the GPU's."""
import numpy as np

FEW_FIELDS, NOT_NUMBER, TOTAL_RANGE, METH_GT_TOTAL = 1, 2, 3, 4
MAX_DIGITS = 18
TOP = 2 ** 31 - 1


class Refused(Exception):
    def __init__(self, why, offset):
        super().__init__('refused (%d) at byte offset %d' % (why, offset))
        self.why, self.offset = why, offset


def is_header(text):
    """the first line's second tab-separated field is not made of ASCII decimal digits only"""
    fields = text.split(b'\n', 1)[0].split(b'\t')
    return not (len(fields) > 1 and fields[1].isdigit())


def _number(tok):
    return int(tok) if tok.isdigit() and len(tok) <= MAX_DIGITS else None


def trim(meth, total):
    """the pair as the .beta file stores it: numpy's float64 division, the product, the cast"""
    if total > 255:
        return int(float(meth) / float(total) * 255.0), 255
    return meth, total


def bed2beta(text, loci, chroms, add_one=False, header=None):
    """text: the BED file's bytes; loci: the bp position of every CpG; chroms: [(name, number of CpGs)] in the order of the loci.
    -> (uint8 rows [n_sites, 2], dict of the counters); raises Refused for the lowest refused line."""
    if header is None:
        header = is_header(text)
    index, base = {}, 0
    for name, size in chroms:
        name = name if isinstance(name, bytes) else name.encode()
        index[name] = {int(p): base + k for k, p in enumerate(np.asarray(loci[base:base + size]).tolist())}
        base += size
    rows = np.zeros((len(loci), 2), dtype=np.uint8)
    seen = set()
    st = dict(lines=0, matched=0, unknown_chrom=0, not_cpg=0, duplicates=0, sites_set=0)
    off = 0
    for ln in text.split(b'\n'):
        at, off = off, off + len(ln) + 1
        if not ln or (header and at == 0):
            continue
        st['lines'] += 1
        f = ln.split(b'\t')
        if len(f) < 5:
            raise Refused(FEW_FIELDS, at)
        start, meth, total = _number(f[1]), _number(f[3]), _number(f[4])
        if start is None or meth is None or total is None:
            raise Refused(NOT_NUMBER, at)
        if total > TOP:
            raise Refused(TOTAL_RANGE, at)
        if meth > total:
            raise Refused(METH_GT_TOTAL, at)
        sites = index.get(f[0])
        if sites is None:
            st['unknown_chrom'] += 1
            continue
        site = sites.get(start + (1 if add_one else 0))
        if site is None:
            st['not_cpg'] += 1
            continue
        st['matched'] += 1
        if site in seen:
            st['duplicates'] += 1
            continue
        seen.add(site)
        rows[site] = trim(meth, total)
    st['sites_set'] = len(seen)
    return rows, st


def dict_frame(loci, chroms):
    """the dictionary as a frame: chr, start"""
    import pandas as pd
    names = np.repeat(np.array([c for c, _ in chroms], dtype=object), [s for _, s in chroms])
    return pd.DataFrame({'chr': names, 'start': np.asarray(loci, dtype=np.int64)})


def bed2beta_frames(path, frame, add_one=False):
    """path: a BED file (plain or gzip); frame: dict_frame() -> uint8 rows"""
    import pandas as pd
    peek = pd.read_csv(path, sep='\t', nrows=1, header=None)
    head = None if str(peek.iloc[0, 1]).isdigit() else 0
    bed = pd.read_csv(path, sep='\t', header=head, names=['chr', 'start', 'meth', 'total'], usecols=[0, 1, 3, 4])
    bed = bed.drop_duplicates(subset=['chr', 'start'])
    if add_one:
        bed = bed.assign(start=bed['start'] + 1)
    pairs = np.array(frame.merge(bed, how='left', on=['chr', 'start']).fillna(0)[['meth', 'total']])
    big = pairs[:, 1] > 255
    pairs[big, 0] = pairs[big, 0] / pairs[big, 1] * 255
    pairs[big, 1] = 255
    return pairs.astype(np.uint8)
