"""A plain-Python restatement of `wgbstools test_bimodal` (the reference's src/python/test_bimodal.py), for tests only: the
product never imports it.  It fixes what the reference leaves to its host: log2 is libm's (math.log2, what wg_log2 restates),
a row's likelihood sums its columns left to right from 0.0 with the C and T sums kept apart and combined as (-1.0 + sum_C) + sum_T
(the reference uses BLAS dgemv, whose order is not defined), a tie goes to cluster 0, and ll0 / new_ll are added in the
reference's sequential Python order, one addition per row copy.  The device must give the same bits (tests/test_gpu_bimodal.py);
the reference's own output pins this restatement (tests/golden/bimodal_cases.json).

The contract has two halves of different strength.  Device == this restatement, bit for bit: both take log2 from libm (math.log2
here, its restatement wg_log2 on the device; tests/test_bimodal_arith_cpu.py ties the two on the EM's own arguments).  This
restatement == the reference only at print precision (rel 1e-12 and a near-tie allowance, tests/test_bimodal_cpu.py): the
reference's EM calls np.log2, which is not libm's log2 to the last bit (numpy 2.2.6 against glibc 2.35: 3,337 of 2,000,000 lattice
arguments differ in the last place), and sums its rows in BLAS's order."""
import bisect
import math

import numpy as np

MAX_PAT_LEN = 150


def parse_pat(text):
    """-> ascending starts, [(start, pattern, count)] of the pat text (bytes)"""
    reads = []
    for ln in text.decode().split('\n'):
        if not ln:
            continue
        t = ln.split('\t')
        reads.append((int(t[1]), t[2], int(t[3])))
    return [r[0] for r in reads], reads


def block_reads(starts, reads, s1, s2, strict, min_len):
    """read_pat_vis (:25-69): the accepted lines [(clipped start, clipped pattern, count)], first_ind, number of columns"""
    lo = bisect.bisect_left(starts, max(1, s1 - MAX_PAT_LEN))
    hi = bisect.bisect_right(starts, s2 - 1)
    out, first, max_ind = [], None, 0
    for st, pat, cnt in reads[lo:hi]:
        cur_end = st + len(pat)
        if cur_end <= s1:
            continue
        cs = st
        if strict:
            if cs < s1:
                pat = pat[s1 - cs:]
                cs = s1
            if cs + len(pat) > s2:
                pat = pat[:s2 - cs]
        if len(pat) < min_len:
            continue
        if first is None:
            first = cs
        out.append((cs, pat, cnt))
        if cur_end > max_ind:
            max_ind = cur_end
    if first is None:
        return out, 0, 0
    return out, first, max_ind - first


def em_block(lines, first, ncols, trace=None):
    """-> (ll0, ll_em, sum of n_per_col, rows, iterations); rows == 0: (0, 0, 0, 0, 0).  trace (a list): one dict per pass is
    appended, rows = the row copies of each cluster, ties = per exact tie l0 == l1 of a line with count > 0 its number of observations,
    order = per cluster the lines with count > 0 whose likelihood would differ as -1.0 + (sum_C + sum_T)"""
    rows = sum(c for _, _, c in lines)
    if rows == 0:
        return 0.0, 0.0, 0.0, 0, 0
    obs = []                                                     # per line: [(column, is_C)] left to right
    for cs, pat, _ in lines:
        obs.append([(cs - first + k, ch == 'C') for k, ch in enumerate(pat) if ch in 'CT'])
    C = [0] * ncols
    T = [0] * ncols
    for o, (_, _, cnt) in zip(obs, lines):
        for col, is_c in o:
            if is_c:
                C[col] += cnt
            else:
                T[col] += cnt
    ll0 = 0.0
    sum_n = 0.0
    for j in range(ncols):
        c = 1e-3 + C[j]
        t = 1e-3 + T[j]
        n = c + t
        ll0 = ll0 + (float(C[j]) * math.log2(c / n) + float(T[j]) * math.log2(t / n))
        sum_n = sum_n + n
    lpc = [[math.log2(0.9)] * ncols, [math.log2(0.1)] * ncols]
    lpt = [[math.log2(1 - 0.9)] * ncols, [math.log2(1 - 0.1)] * ncols]
    ll = -math.inf
    iters = 0
    while True:
        iters += 1
        cc = [[0] * ncols, [0] * ncols]
        ct = [[0] * ncols, [0] * ncols]
        S = [0.0, 0.0]
        seen = dict(rows=[0, 0], ties=[], order=[0, 0])
        for o, (_, _, cnt) in zip(obs, lines):
            sc = [0.0, 0.0]
            stt = [0.0, 0.0]
            for col, is_c in o:
                for z in (0, 1):
                    if is_c:
                        sc[z] = sc[z] + lpc[z][col]
                    else:
                        stt[z] = stt[z] + lpt[z][col]
            l0 = (-1.0 + sc[0]) + stt[0]
            l1 = (-1.0 + sc[1]) + stt[1]
            z = 1 if l1 > l0 else 0
            v = l1 if z else l0
            seen['rows'][z] += cnt
            if l1 == l0 and cnt:
                seen['ties'].append(len(o))
            if cnt and -1.0 + (sc[z] + stt[z]) != v:
                seen['order'][z] += 1
            s = S[z]
            for _ in range(cnt):
                s = s + v
            S[z] = s
            for col, is_c in o:
                if is_c:
                    cc[z][col] += cnt
                else:
                    ct[z][col] += cnt
        if trace is not None:
            trace.append(seen)
        new_ll = S[0] + S[1]
        more = new_ll - ll > 0
        ll = new_ll
        if not more:
            break
        for z in (0, 1):
            for j in range(ncols):
                pc = 1e-3 + cc[z][j]
                pt = 1e-3 + ct[z][j]
                tot = pc + pt
                lpc[z][j] = math.log2(pc / tot)
                lpt[z][j] = math.log2(pt / tot)
    return ll0, ll, sum_n, rows, iters


def block_result(starts, reads, s1, s2, strict=False, min_len=1):
    """-> (ll0, ll_em, sum_n, ncols, rows, iterations) of block [s1, s2)"""
    lines, first, ncols = block_reads(starts, reads, s1, s2, strict, min_len)
    ll0, ll, sum_n, rows, iters = em_block(lines, first, ncols)
    return ll0, ll, sum_n, ncols, rows, iters


def pvalue(ll0, ll_em, ncols, rows):
    """test_single_region's p (float64; 1.0 without rows)"""
    from scipy import stats
    if rows == 0:
        return np.float64(np.float32(1.0))
    return 1 - stats.chi2.cdf(2 * np.log(2) * (np.float64(ll_em) - np.float64(ll0)), ncols)


def single_text(res):
    """the lines test_single_region prints"""
    ll0, ll, sum_n, ncols, rows, _ = res
    if rows == 0:
        return ''
    ll0, ll, sum_n = np.float64(ll0), np.float64(ll), np.float64(sum_n)
    out = f'LL: {ll0} | {rows} reads | {int(round(sum_n))} observed | BPI: {2 ** (ll0 / sum_n)}\n'
    out += f'LL: {ll} | {rows} reads | {int(round(sum_n))} observed | BPI: {2 ** (ll / sum_n)}\n'
    out += f'pvalue: {pvalue(ll0, ll, ncols, rows):,.3e}\n'
    return out


def fdr_bh(p32, alpha=0.05):
    """statsmodels' multipletests(method='fdr_bh') on ascending float32 p -> (reject, corrected) as float64"""
    p = np.asarray(p32).astype(np.float64)
    n = p.size
    ecdf = np.arange(1, n + 1) / float(n)
    reject = p <= ecdf * alpha
    if reject.any():
        reject[:int(np.nonzero(reject)[0].max()) + 1] = True
    corr = np.minimum.accumulate((p / ecdf)[::-1])[::-1]
    corr[corr > 1] = 1
    return reject, corr


def multi_text(lines, p32, print_all=False):
    """test_multiple_regions' output for the block lines (in chromosome order) and their float32 p"""
    if not lines:
        return ''
    order = np.argsort(np.asarray(p32, dtype=np.float32), kind='stable')
    ls = [lines[i] for i in order]
    ps = np.asarray(p32, dtype=np.float32)[order]
    reject, corr = fdr_bh(ps)
    if not reject[0]:
        return ''
    if not print_all:
        k = int(np.argmax(1 - reject))
        ls, corr = ls[:k], corr[:k]
    return ''.join(f'{a}\t{c:,.1e}\n' for a, c in zip(ls, corr))
