"""Seeded inputs of the `wgbstools merge` cases (tests/golden/make_golden_merge.py records what the reference's cview, sort and collapse
script print for the pat cases, and what its trim_to_uint8 gives for the beta cases, in tests/golden/merge_cases.json;
tests/test_merge_cpu.py and tests/test_gpu_merge.py rebuild the inputs).  Pat texts over the tiny genome of frag_cases.genome_dir (chr1:
sites 1 .. 2500, chr2: 2501 .. 4000): every read lies inside the chromosome it names and every count is at least 1 — where the one
global sort of this build and the reference's pass per chromosome agree."""
import numpy as np

import frag_cases as FC
import homog_cases as HC

N_SITES = FC.N_SITES
CHR1_SITES = FC.GENOME_CHROMS[0][1]
genome_dir = FC.genome_dir
region_text = FC.region_text


def reads_text(seed, n_reads, lo, hi, max_len=3, max_count=4, alphabet=b'CCCTTTCT', newline=True):
    """n_reads reads sorted by start, starts in [lo, hi], 1 .. max_len sites of `alphabet` (8 bytes), cut at the end of their chromosome;
    short reads over few letters: many lines are equal, inside a file and between files"""
    U = HC.U
    start = np.sort((HC._rand(seed, 1, n_reads) % U(hi - lo + 1)).astype(np.int64) + lo)
    h = HC._rand(seed, 2, n_reads)
    ln = 1 + (h % U(max_len)).astype(np.int64)
    last = np.where(start <= CHR1_SITES, CHR1_SITES, N_SITES)
    ln = np.minimum(ln, last - start + 1)
    cnt = 1 + ((h >> U(8)) % U(max_count)).astype(np.int64)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    chars = letters[(HC._rand(seed, 3, int(ln.sum())) & U(7)).astype(np.int64)].tobytes()
    off = np.concatenate([[0], np.cumsum(ln)]).tolist()
    text = b''.join(b'chr%d\t%d\t%s\t%d\n' % (1 if start[i] <= CHR1_SITES else 2, start[i], chars[off[i]:off[i + 1]], cnt[i]) for i in range(n_reads))
    return text if newline else text[:-1]


_DOTS = b'CCTTH...'
# the issue's first case: about ten reads each, the second file begins below where the first ends; equal lines in both
_TINY_A = b''.join(b'chr1\t%d\t%s\t%d\n' % r for r in [(5, b'CT', 1), (5, b'CT', 2), (7, b'C', 1), (9, b'TTC', 3), (12, b'C', 1), (12, b'CC', 1),
                                                        (15, b'T', 2), (20, b'CTCT', 1), (31, b'C', 4), (40, b'TT', 1)])
_TINY_B = b''.join(b'chr1\t%d\t%s\t%d\n' % r for r in [(3, b'C', 1), (5, b'CT', 4), (9, b'TTC', 1), (9, b'TTCC', 1), (12, b'C', 2), (13, b'T', 1),
                                                        (20, b'CTCT', 5), (31, b'C', 1), (31, b'CT', 1), (44, b'T', 2)])

# name -> files: the pat texts (bytes, or a callable that makes them); where: [] | ['-s', text] | ['-r', text]; flags: the reference's view flags
PAT_CASES = {
    'tiny_overlap': dict(files=[_TINY_A, _TINY_B], where=['-s', '1-100'], flags=[]),
    'tiny_no_newline': dict(files=[_TINY_A[:-1], _TINY_B], where=['-s', '1-100'], flags=[]),
    'sites_two': dict(files=[lambda: reads_text(61, 300, 1150, 1260), lambda: reads_text(62, 280, 1150, 1260)], where=['-s', '1200-1230'], flags=[]),
    'sites_strict_strip_min3': dict(files=[lambda k=k: reads_text(63 + k, 400, 1150, 1260, max_len=9, alphabet=_DOTS) for k in range(3)],
                                    where=['-s', '1200-1230'], flags=['--strict', '--strip', '--min_len', '3']),
    'region_two': dict(files=[lambda: reads_text(66, 400, 2750, 2960, max_len=5), lambda: reads_text(67, 350, 2750, 2960, max_len=5)],
                       where=['-r', region_text], flags=['--strict']),
    'wg_two': dict(files=[lambda: reads_text(68, 300, 1, N_SITES), lambda: reads_text(69, 320, 1, N_SITES)], where=[], flags=[]),
    'wg_three': dict(files=[lambda k=k: reads_text(70 + k, 400, 2300, 2700, max_len=2) for k in range(3)], where=[], flags=[]),
}


def case_files(case):
    return [f() if callable(f) else f for f in case['files']]


def case_where(case):
    return [w() if callable(w) else w for w in case['where']]


def flag_kwargs(flags):
    """the reference's flags -> the keywords of merge_ref.merge_pats / view.view_pats"""
    kw = dict(strict='--strict' in flags, strip='--strip' in flags, min_len=1)
    if '--min_len' in flags:
        kw['min_len'] = int(flags[flags.index('--min_len') + 1])
    return kw


# ---- beta rows ----
def hashed_rows(seed, n, n_rows, wide=False, cov_max=None):
    """n_rows arrays [n, 2] of uint8 (uint16 when wide): cov below cov_max (default: the whole range), meth <= cov"""
    U = HC.U
    top = (65536 if wide else 256) if cov_max is None else cov_max
    out = []
    for r in range(n_rows):
        cov = (HC._rand(seed, 10 + 2 * r, n) % U(top)).astype(np.int64)
        meth = (HC._rand(seed, 11 + 2 * r, n) % (cov.astype(np.uint64) + U(1))).astype(np.int64)
        out.append(np.stack([meth, cov], axis=1).astype(np.uint16 if wide else np.uint8))
    return out


def saturated_domain():
    """two uint8 rows in which every (M, C) with 256 <= C <= 510 and 0 <= M <= C occurs once as the sums of a site: all a merge of two
    files can saturate"""
    C = np.repeat(np.arange(256, 511), np.arange(257, 512))
    M = np.concatenate([np.arange(c + 1) for c in range(256, 511)])
    c1 = np.minimum(C, 255)
    m1 = np.minimum(M, 255)
    rows = [np.stack([m1, c1], axis=1).astype(np.uint8), np.stack([M - m1, C - c1], axis=1).astype(np.uint8)]
    assert C.size == 97920 and (M - m1).max() <= 255 and (C - c1).min() >= 1
    return rows


def wide_corners():
    """two uint16 rows: the corners M = 0, 1, C - 1, C of C = 65536 and 131070"""
    sites = []
    for C in (65536, 131070):
        for M in (0, 1, C - 1, C):
            c1, m1 = min(C, 65535), min(M, 65535)
            sites.append(((m1, c1), (M - m1, C - c1)))
    return [np.array([s[k] for s in sites], dtype=np.uint16) for k in range(2)]


# name -> rows: a callable that makes them; lbeta: the -l flag
BETA_CASES = {
    'u8_two_4099': dict(rows=lambda: hashed_rows(81, 4099, 2), lbeta=False),
    'u8_three_4099': dict(rows=lambda: hashed_rows(82, 4099, 3), lbeta=False),
    'u8_33_rows_lbeta': dict(rows=lambda: hashed_rows(83, 1001, 33), lbeta=True),
    'u8_saturated_domain': dict(rows=saturated_domain, lbeta=False),
    'u16_two_lbeta': dict(rows=lambda: hashed_rows(84, 4099, 2, wide=True), lbeta=True),
    'u16_corners_lbeta': dict(rows=wide_corners, lbeta=True),
}


def rows_sha1(rows):
    import hashlib
    h = hashlib.sha1()
    for r in rows:
        h.update(np.ascontiguousarray(r).tobytes())
    return h.hexdigest()
