"""Hand-built `wgbstools test_bimodal` inputs, one per corner where a one-wavefront-per-block EM goes wrong, and the census that
says which corners a case really reaches (tests/test_bimodal_cpu.py asserts it; tests/test_gpu_bimodal.py compares the device with
tests/bimodal_ref.py on every case, bit for bit).  Nothing here comes from the reference: deep rows and long reads are exactly where
its BLAS order of summation is undefined, so these cases are pinned to the restatement only.  Deterministic: the pattern letters
are synth.hash_at (splitmix64)."""
import functools

import numpy as np

import bimodal_ref as BR
from wgbs_tools_amd.synth import hash_at

CTX = BR.MAX_PAT_LEN

# every corner a case may be named for (census() returns a subset)
CORNERS = (
    'lines_1', 'lines_63', 'lines_64', 'lines_65', 'lines_128', 'lines_129', 'rejected_between_accepted',
    'column_count_100k', 'rows_5k_in_each_cluster',
    'zero_count_sets_first_ind', 'zero_count_sets_ncols', 'all_counts_zero',
    'tie_without_observations', 'tie_on_symmetric_table',
    'ncols_16', 'ncols_17', 'ncols_256', 'ncols_257',
    'pattern_15', 'pattern_16', 'pattern_17', 'pattern_32', 'pattern_33',
    'strict_clip_15', 'strict_clip_16', 'strict_clip_17', 'strict_cut_inside_word',
    'lookback_150_used', 'lookback_151_unused', 'lookback_clamped', 'start_0_unused', 'start_minus_3_unused',
    'ends_at_s1_skipped', 'ends_at_s1_plus_1_used', 'starts_at_s2_minus_1_used', 'starts_at_s2_unused',
    'clipped_to_min_len_used', 'clipped_to_min_len_minus_1_unused',
    'eight_passes', 'row_sum_order_cluster_0', 'row_sum_order_cluster_1', 'blocks_descending', 'blocks_shuffled_with_duplicates',
)


def _letters(seed, n, allele=None, flip=8, gaps=True):
    """n pattern letters: allele None: C or T at random, else that letter with 1 in `flip` sites the other; '.' and 'H' here and there"""
    h = hash_at(seed, 7, np.arange(n, dtype=np.int64))
    if allele is None:
        meth = (h & np.uint64(1)) == 1
    else:
        meth = ((h % np.uint64(flip)) == 0) ^ (allele == 'C')
    ch = np.where(meth, 'C', 'T')
    if gaps:
        ch = np.where(((h >> np.uint64(16)) % np.uint64(13)) == 0, '.', ch)
        ch = np.where(((h >> np.uint64(24)) % np.uint64(29)) == 0, 'H', ch)
    return ''.join(ch.tolist())


def _observed_ends(p):
    """the pattern with an observation at its first and last site"""
    fix = lambda c, d: c if c in 'CT' else d
    return p if len(p) < 2 else fix(p[0], 'C') + p[1:-1] + fix(p[-1], 'T')


def _text(reads):
    reads = sorted(reads, key=lambda r: r[0])                      # (stable: equal starts keep their order)
    return ''.join('chr1\t%d\t%s\t%d\n' % r for r in reads).encode()


def _two_alleles(seed, s1, n, span, max_len=8, max_count=3, min_len=1):
    """n reads starting in [s1, s1 + span), alternately mostly-C and mostly-T, of min_len .. max_len sites"""
    h = hash_at(seed, 3, np.arange(n, dtype=np.int64))
    out = []
    for i in range(n):
        ln = min_len + int(h[i] % np.uint64(max_len - min_len + 1))
        p = _observed_ends(_letters(seed * 1000 + i, ln, 'CT'[i & 1]))
        out.append((s1 + i * span // n, p, 1 + int((h[i] >> np.uint64(8)) % np.uint64(max_count))))
    return out


def _lockstep():
    """blocks of exactly N table rows, all accepted (the last, partial 64-line batch of the lock-step sum), and one block in
    which rejected lines lie between accepted ones; --strict --min_len 2"""
    reads, s, e = [], [], []
    for k, n in enumerate((1, 63, 64, 65, 128, 129)):
        s1 = 1000 * (k + 1)
        reads += _two_alleles(10 + k, s1, n, 10, min_len=2)         # starts s1 .. s1 + 9, the block ends at s1 + 12
        s.append(s1)
        e.append(s1 + 12)
    s1, s2 = 8000, 8012
    mixed = [(s1 - 6, 'CTCCTCTC', 2)] + _two_alleles(30, s1 - 6, 150, 16, min_len=2)
    mixed += [(s1 - 5, 'CTCT', 2)] * 5 + [(s1 - 3, 'CTCT', 2)] * 5 + [(s1 - 1, 'TC.', 3)]      # end before s1; one site left once clipped
    reads += mixed
    s.append(s1)
    e.append(s2)
    return dict(text=_text(reads), s=s, e=e, strict=True, min_len=2,
                corners={'lines_1', 'lines_63', 'lines_64', 'lines_65', 'lines_128', 'lines_129', 'rejected_between_accepted'})


def _deep():
    """counts in the thousands: column counts past 100,000 (log2 arguments below 2^-16), tens of thousands of row copies per cluster"""
    reads = []
    for i in range(60):
        p = _observed_ends(_letters(500 + i, 6 + i % 5, 'CCT'[i % 3], flip=16, gaps=False))
        reads.append((200 + i % 3, p, 2500 + 17 * i))
    return dict(text=_text(reads), s=[200], e=[212], strict=False, min_len=1, corners={'column_count_100k', 'rows_5k_in_each_cluster'})


def _zero_counts():
    reads = [(300, 'CCTC.CT', 0)] + _two_alleles(40, 302, 30, 6) + [(307, 'TTCTCCTTCTCCTTCCTTTC', 0)]
    reads += [(600, 'CCTC', 0), (601, 'TTT', 0), (603, 'C.T', 0)]
    return dict(text=_text(reads), s=[300, 600], e=[310, 606], strict=False, min_len=1,
                corners={'zero_count_sets_first_ind', 'zero_count_sets_ncols', 'all_counts_zero'})


def _ties():
    """lines of '.' and 'H' only (l0 == l1 == -1.0) among the others, and a column whose C counts are the same in both clusters after
    the first pass (5 + 2 copies of 'C' in cluster 0, 7 of 'CTT' in cluster 1), so that the 'C' lines tie exactly in the second"""
    reads = [(400, 'C', 5), (400, 'CTT', 7), (400, '.H.', 3), (400, 'C', 2)]
    body = _two_alleles(50, 403, 40, 8, min_len=3)
    for i in range(0, 40, 5):
        body[i] = (body[i][0], '..H.'[:1 + i % 4], 1 + i % 3)
    return dict(text=_text(reads + body), s=[400], e=[420], strict=False, min_len=1,
                corners={'tie_without_observations', 'tie_on_symmetric_table'})


def _table_switch():
    """blocks of exactly 16, 17, 256 and 257 columns: either side of `nc <= lds_cols` for the default tables and for 16"""
    reads, s, e = [], [], []
    for k, nc in enumerate((16, 17, 256, 257)):
        s1 = 1000 * (k + 1)
        reads.append((s1, _observed_ends(_letters(60 + k, nc)), 2))
        reads += _two_alleles(70 + k, s1, 24, 8)
        s.append(s1)
        e.append(s1 + 10)
    return dict(text=_text(reads), s=s, e=e, strict=False, min_len=1, corners={'ncols_16', 'ncols_17', 'ncols_256', 'ncols_257'})


def _words():
    """the 2-bit pattern words: patterns ending at and next to a word's end; under --strict reads starting 15 / 16 / 17 sites before
    s1 and reads cut by s2 inside a word; clipped lengths of exactly min_len = 3 and of 2"""
    s1, s2 = 500, 540
    reads = [(s1 - k, _observed_ends(_letters(80 + k, 40)), 1 + k % 3) for k in (17, 16, 15)]
    reads += [(s1 - 5, 'TTCCTCTC', 2), (s1 - 5, 'CCTTCTC', 3)]                    # clipped to 3 and to 2 sites
    reads += _two_alleles(90, s1, 20, 30, min_len=3)
    reads += [(s2 - 21, _observed_ends(_letters(95, 40)), 2), (s2 - 5, _observed_ends(_letters(96, 30)), 1)]      # cut at 21 and at 5 sites
    reads += [(s2 - 3, 'CTCTTCCTCT', 2), (s2 - 2, 'TCTCCTTCTC', 3)]               # cut to 3 and to 2 sites
    t1 = 800
    reads += [(t1 + i, _observed_ends(_letters(100 + n, n)), 1 + i) for i, n in enumerate((15, 16, 17, 32, 33))]
    reads += _two_alleles(110, t1, 20, 30, min_len=3)
    return dict(text=_text(reads), s=[s1, t1], e=[s2, t1 + 60], strict=True, min_len=3,
                corners={'pattern_15', 'pattern_16', 'pattern_17', 'pattern_32', 'pattern_33', 'strict_clip_15', 'strict_clip_16',
                         'strict_clip_17', 'strict_cut_inside_word', 'clipped_to_min_len_used', 'clipped_to_min_len_minus_1_unused'})


def _lookback():
    """the reads a block asks for start in [max(1, s1 - 150), s2 - 1] and end after s1"""
    reads = [(-3, _observed_ends(_letters(120, 20)), 2), (0, _observed_ends(_letters(121, 15)), 3)]       # overlap [5, 12): never used
    reads += [(1, 'CCTCCCTCCC', 2)] + _two_alleles(122, 5, 16, 7)
    s1, s2 = 1000, 1010
    reads += [(s1 - CTX - 1, _observed_ends(_letters(123, 160)), 2), (s1 - CTX, _observed_ends(_letters(124, 155)), 3)]
    reads += [(s1 - 10, 'CTCCTCCTCC', 2), (s1 - 10, 'TCTTCTTTCTC', 2)]            # end at s1, at s1 + 1
    reads += _two_alleles(125, s1, 20, 9)
    reads += [(s2 - 1, 'TTCT', 3), (s2, 'CCCC', 4)]
    return dict(text=_text(reads), s=[5, s1], e=[12, s2], strict=False, min_len=1,
                corners={'lookback_150_used', 'lookback_151_unused', 'lookback_clamped', 'start_0_unused', 'start_minus_3_unused',
                         'ends_at_s1_skipped', 'ends_at_s1_plus_1_used', 'starts_at_s2_minus_1_used', 'starts_at_s2_unused'})


def _slow():
    """weakly separated populations over many columns: the EM needs at least eight passes"""
    reads = []
    for i in range(SLOW_READS):
        reads.append((700 + i % 24, _letters(SLOW_SEED + i, 6 + i % 7, 'CT'[i & 1], flip=3), 1 + i % 4))
    return dict(text=_text(reads), s=[700], e=[730], strict=False, min_len=1, corners={'eight_passes'})


def _row_sums():
    """one line of k C and m T sites per block: new_ll is a few copies of that row's likelihood alone, so the order (-1.0 + sum_C) + sum_T shows in
    the result's last bit (under thousands of rows the sum over the rows rounds such a bit away)"""
    km = [(k, m) for k in range(1, 8) for m in range(1, 8)]
    reads = [(400 * (i + 1), 'C' * k + 'T' * m, 1 + (3 * k + m) % 5) for i, (k, m) in enumerate(km)]
    s = [r[0] for r in reads]
    return dict(text=_text(reads), s=s, e=[a + 10 for a in s], strict=False, min_len=1,
                corners={'row_sum_order_cluster_0', 'row_sum_order_cluster_1'})


SLOW_SEED, SLOW_READS = 16000, 300      # (a seed on which the restatement takes 12 passes)


def _reordered(order, corner):
    base = _lockstep()
    s, e = [base['s'][i] for i in order], [base['e'][i] for i in order]
    return dict(base, s=s, e=e, corners={corner})


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(text, s, e, strict, min_len, corners: what the case is there for)"""
    return {
        'lockstep': _lockstep(), 'deep': _deep(), 'zero_counts': _zero_counts(), 'ties': _ties(), 'table_switch': _table_switch(),
        'words': _words(), 'lookback': _lookback(), 'slow': _slow(), 'row_sums': _row_sums(),
        'blocks_descending': _reordered([6, 5, 4, 3, 2, 1, 0], 'blocks_descending'),
        'blocks_shuffled': _reordered([3, 6, 0, 3, 5, 1, 6, 2, 4, 0], 'blocks_shuffled_with_duplicates'),
    }


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's (ll0, ll_em, sum_n, columns, rows, iterations) per block of the case, in the order given"""
    c = cases()[name]
    starts, reads = BR.parse_pat(c['text'])
    memo = {}
    for a, b in zip(c['s'], c['e']):
        if (a, b) not in memo:
            memo[(a, b)] = BR.block_result(starts, reads, a, b, c['strict'], c['min_len'])
    return [memo[(a, b)] for a, b in zip(c['s'], c['e'])]


def census(name):
    """the corners the case reaches, worked out through bimodal_ref (and the plain rules of read_pat_vis for the reads left out)"""
    c = cases()[name]
    strict, min_len = c['strict'], c['min_len']
    starts, reads = BR.parse_pat(c['text'])
    assert starts == sorted(starts)
    got = set()
    s, e = c['s'], c['e']
    if len(s) > 2 and all(a > b for a, b in zip(s, s[1:])):
        got.add('blocks_descending')
    if len(set(zip(s, e))) < len(s) and s != sorted(s) and s != sorted(s, reverse=True):
        got.add('blocks_shuffled_with_duplicates')
    for s1, s2 in sorted(set(zip(s, e))):
        lines, first, ncols = BR.block_reads(starts, reads, s1, s2, strict, min_len)
        lo, hi = np.searchsorted(starts, max(1, s1 - CTX), 'left'), np.searchsorted(starts, s2 - 1, 'right')
        window = reads[lo:hi]
        # which rows of the window are accepted (block_reads keeps their order)
        acc = []
        for st, pat, cnt in window:
            cl = len(pat)
            if strict:
                cl = min(st + len(pat), s2) - max(st, s1)
            acc.append(st + len(pat) > s1 and cl >= min_len)
        assert sum(acc) == len(lines)
        if all(acc) and len(lines) in (1, 63, 64, 65, 128, 129):
            got.add('lines_%d' % len(lines))
        if acc:
            i0, i1 = acc.index(True) if True in acc else 0, len(acc) - 1 - acc[::-1].index(True) if True in acc else 0
            inner = [(r, a) for r, a in zip(window[i0:i1 + 1], acc[i0:i1 + 1]) if not a]
            if any(r[0] + len(r[1]) <= s1 for r, _ in inner) and any(r[0] + len(r[1]) > s1 for r, _ in inner) and len(window) > 64:
                got.add('rejected_between_accepted')
        if ncols in (16, 17, 256, 257):
            got.add('ncols_%d' % ncols)
        rows = sum(cnt for _, _, cnt in lines)
        if lines and rows == 0 and ncols > 0:
            got.add('all_counts_zero')
        if rows:
            pos = [(cs, pat, cnt) for cs, pat, cnt in lines if cnt > 0]
            if lines[0][2] == 0 and lines[0][0] < min(cs for cs, _, _ in pos):
                got.add('zero_count_sets_first_ind')
            ends = [(st + len(pat), cnt) for (st, pat, cnt), a in zip(window, acc) if a]
            if max([en for en, cnt in ends if cnt == 0], default=0) > max(en for en, cnt in ends if cnt > 0):
                got.add('zero_count_sets_ncols')
            col = {}
            for cs, pat, cnt in lines:
                for k, ch in enumerate(pat):
                    if ch in 'CT':
                        col[(cs + k, ch)] = col.get((cs + k, ch), 0) + cnt
            if max(col.values()) >= 100000 and min(cnt for _, _, cnt in pos) >= 1000:
                got.add('column_count_100k')
            trace = []
            iters = BR.em_block(lines, first, ncols, trace)[4]
            if min(trace[-1]['rows']) >= 5000:
                got.add('rows_5k_in_each_cluster')
            if any(0 in t['ties'] for t in trace):
                got.add('tie_without_observations')
            if any(n > 0 for t in trace[1:] for n in t['ties']):
                got.add('tie_on_symmetric_table')
            if iters >= 8:
                got.add('eight_passes')
            for z in (0, 1):                                      # (a single line: its likelihood is the block's ll_em)
                if len(lines) == 1 and trace[-1]['order'][z]:
                    got.add('row_sum_order_cluster_%d' % z)
        used = [r for r, a in zip(window, acc) if a and r[2] > 0]
        for st, pat, cnt in used:
            last_observed = pat[-1] in 'CT'
            if len(pat) in (15, 16, 17, 32, 33) and last_observed and s1 <= st and st + len(pat) <= s2:
                got.add('pattern_%d' % len(pat))
            if strict and s1 - st in (15, 16, 17) and any(ch in 'CT' for ch in pat[s1 - st:]):
                got.add('strict_clip_%d' % (s1 - st))
            if strict and st + len(pat) > s2 and (s2 - st) % 16 and any(ch in 'CT' for ch in pat[s2 - st:]):
                got.add('strict_cut_inside_word')
            if strict and min(st + len(pat), s2) - max(st, s1) == min_len and min_len > 1 and len(pat) > min_len:
                got.add('clipped_to_min_len_used')
            if st == s1 - CTX:
                got.add('lookback_150_used')
            if st + len(pat) == s1 + 1:
                got.add('ends_at_s1_plus_1_used')
            if st == s2 - 1:
                got.add('starts_at_s2_minus_1_used')
        overlapping = lambda r: r[2] > 0 and r[0] + len(r[1]) > s1 and r[0] < s2 and any(
            ch in 'CT' for ch in r[1][max(0, s1 - r[0]):s2 - r[0]])
        for r, a in zip(window, acc):
            if not a and r[2] > 0 and strict and min(r[0] + len(r[1]), s2) - max(r[0], s1) == min_len - 1 and len(r[1]) >= min_len:
                got.add('clipped_to_min_len_minus_1_unused')
            if not a and r[2] > 0 and r[0] + len(r[1]) == s1:
                got.add('ends_at_s1_skipped')
        outside = reads[:lo] + reads[hi:]
        if s1 <= CTX and rows:
            got.add('lookback_clamped')
            if any(r[0] == 0 and overlapping(r) for r in outside):
                got.add('start_0_unused')
            if any(r[0] == -3 and overlapping(r) for r in outside):
                got.add('start_minus_3_unused')
        if s1 > CTX + 1 and any(r[0] == s1 - CTX - 1 and overlapping(r) for r in outside):
            got.add('lookback_151_unused')
        if any(r[0] == s2 and r[2] > 0 for r in outside):
            got.add('starts_at_s2_unused')
    return got
