"""A plain-Python restatement of the contract of `wgbstools mix_pat` (wgbs_tools_amd/mix_pat.py's docstring), built on tests/view_ref.py
and written from the contract, not from the code under test: Philox4x32-10, the sample rule, the rate arithmetic, and the whole pipeline
over text — cut, sample, collapse per label, the order of tied lines, the label column.  tests/test_mix_pat_cpu.py holds it against the
goldens that the reference's cview, sort and collapse script wrote (tests/golden/mix_cases.json) and holds csrc/view_core.h against it;
the GPU tests hold the device against it."""
import struct

import merge_ref as MR
import view_ref as VR

M32 = 0xffffffff
MAX_DRAWS = 1 << 20


class Refused(Exception):
    def __init__(self, kind, file, offset):
        super().__init__('file %d: %s at %s' % (file, kind, offset))
        self.kind, self.file, self.offset = kind, file, offset


def philox4x32_10(counter, key):
    """Salmon et al. 2011: ten rounds of (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped after each"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_blocks(off, stream, seed, n_blocks):
    """the same generator over the counters {off lo, off hi, b, stream} for b in range(n_blocks), numpy-wide: [n_blocks, 4] words"""
    import numpy as np
    u = np.uint64
    c0, c1 = np.full(n_blocks, off & M32, dtype=u), np.full(n_blocks, off >> 32, dtype=u)
    c2, c3 = np.arange(n_blocks, dtype=u), np.full(n_blocks, stream, dtype=u)
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ u(k0), p1 & u(M32), (p0 >> u(32)) ^ c3 ^ u(k1), p0 & u(M32)
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], axis=1)


def sample(count, reps, T, seed, stream, off):
    """the successes among count * reps draws: draw j is word j & 3 of the block with counter {off lo, off hi, j >> 2, stream}, key seed"""
    n, got = count * reps, 0
    if n >= 1024:                                                    # many draws: the numpy form (test_mix_pat_cpu.py holds the two together)
        return int((philox_blocks(off, stream, seed, (n + 3) // 4).reshape(-1)[:n] < T).sum())
    for b in range((n + 3) // 4):
        words = philox4x32_10((off & M32, off >> 32, b, stream), (seed & M32, seed >> 32))
        got += sum(1 for w in words[:min(4, n - 4 * b)] if w < T)
    return got


def stream_of(rep, file):
    return (rep << 16) | file


# ---- the rate arithmetic ----
def rates_of(given, k):
    """K or K - 1 rates -> K rates, or ValueError"""
    rates = list(given)
    if len(rates) == k - 1:
        rates.append(1.0 - sum(rates))
    if len(rates) != k:
        raise ValueError('count')
    if abs(sum(rates) - 1) > 1e-8:
        raise ValueError('sum')
    if min(rates) < 0 or max(rates) > 1:
        raise ValueError('range')
    return rates


def adjusted(rates, covs, cov=None):
    if not cov:
        cov = covs[max(range(len(rates)), key=lambda i: (rates[i], -i))]       # (argmax: the first of equal rates)
    return cov, [r * cov / c for r, c in zip(rates, covs)]


def float32_of_text(text):
    """the float32 nearest to a decimal text, as a Python float (std::stof, then the widening to double)"""
    return struct.unpack('f', struct.pack('f', float(text)))[0]


def sampler_args(adj):
    """-> (T, reps, p)"""
    ss, reps = adj, 1
    while ss > 0.25:
        reps, ss = reps * 2, ss / 2
    p = float32_of_text('%.6f' % ss)
    T = int(p * 2 ** 32)
    assert T == p * 2 ** 32 or T < p * 2 ** 32 < T + 1                   # (p has 24 bits: the product is exact)
    return T, reps, p


# ---- the pipeline over text ----
def lines_with_offsets(text):
    """[(offset, chrom, rs, pattern, count)] of the non-empty, well-formed lines"""
    out, pos = [], 0
    for line in text.split(b'\n'):
        off, pos = pos, pos + len(line) + 1
        if not line:
            continue
        tok = line.split(b'\t')
        out.append((off, tok[0], VR._number(tok[1], False), tok[2], VR._number(tok[3], True)))
    return out


def sample_text(text, T, reps, seed, stream):
    """the lines of a pat text with their counts drawn — keyed on the ORIGINAL byte offsets —, the lines drawn to 0 gone: what goes into the
    reference's own pipeline when the goldens are made (sampling before the cut says the same: the cut never reads the count)"""
    return b''.join(b'%s\t%d\t%s\t%d\n' % (chrom, rs, pat, new) for off, chrom, rs, pat, count in lines_with_offsets(text)
                    for new in [sample(count, reps, T, seed, stream, off)] if new > 0)


def tie_key(line):
    """a collapsed, labelled line (chrom, rs, pattern, sum, label) under `LC_ALL=C sort -m -k2,2n -k3,3`: the two keys, then the whole line —
    the chromosome, (start and pattern again,) the decimal text of the count, the label"""
    chrom, rs, pat, total, label = line
    return rs, pat, chrom, b'%d' % total, label


def mix(texts, labels, per_file, seed, rep, s, e, stats=None, **flags):
    """the output text (bytes) of one repetition; per_file: (T, reps) of every file; labels: bytes.  Refused(kind, file, offset) as the
    device refuses: merge's refusals first, then the first line with count * reps above 2^20 among the reads the cut lets through.
    stats: a dict that receives reached / dropped / kept and the kept sum per label."""
    try:
        MR.merge_pats(texts, s, e, **flags)
    except MR.Refused as r:
        raise Refused(r.kind, r.file, r.offset)
    runs, over = {}, None
    reached = dropped = kept = 0
    by_label = {lab: 0 for lab in labels}
    for k, text in enumerate(texts):
        T, reps = per_file[k]
        for off, chrom, rs, pat, count in lines_with_offsets(text):
            c = VR.cut(rs, pat, s, e, **flags)
            if c is None:
                continue
            reached += 1
            if count * reps > MAX_DRAWS:
                over = over if over is not None else (k, off)
                dropped += 1
                continue
            new = sample(count, reps, T, seed, stream_of(rep, k), off)
            if new == 0:
                dropped += 1
                continue
            kept += new
            by_label[labels[k]] += new
            key = (chrom, c[0], c[1], labels[k])
            runs[key] = runs.get(key, 0) + new
    if over is not None:
        raise Refused('over', *over)
    if stats is not None:
        stats.update(reached=reached, dropped=dropped, kept=kept, by_label=by_label)
    lines = sorted(((chrom, rs, pat, total, label) for (chrom, rs, pat, label), total in runs.items()), key=tie_key)
    return b''.join(b'%s\t%d\t%s\t%d\t%s\n' % ln for ln in lines)
