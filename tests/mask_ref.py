"""A plain-Python restatement of the contract of `wgbstools mask_pat` (wgbs_tools_amd/mask_pat.py's docstring), built on
tests/view_ref.py: select whole reads by the interval, hide the sites of the blocks, strip, sort, collapse.
tests/test_mask_pat_cpu.py holds it against the goldens the reference's own tools wrote, the GPU tests hold the device against it."""
import bisect

import merge_ref as MR
import view_ref as VR

Refused = VR.Refused


def union(blocks):
    """the blocks [(start, end)] in any order -> disjoint ascending intervals (touching ones joined)"""
    out = []
    for a, b in sorted((int(a), int(b)) for a, b in blocks):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(x) for x in out]


class Hidden:
    """the hidden sites of the blocks: `site in h`, len(h)"""

    def __init__(self, blocks):
        self.intervals = union(blocks)
        self.starts = [a for a, _ in self.intervals]

    def __contains__(self, site):
        k = bisect.bisect_right(self.starts, site) - 1
        return k >= 0 and site < self.intervals[k][1]

    def __len__(self):
        return sum(b - a for a, b in self.intervals)

    def words(self):
        """(lo, hi, the bitmap of view_core.h as a list of 32-bit words)"""
        lo, hi = self.intervals[0][0], self.intervals[-1][1]
        out = [0] * ((hi - lo + 31) // 32)
        for a, b in self.intervals:
            for site in range(a, b):
                out[(site - lo) >> 5] |= 1 << ((site - lo) & 31)
        return lo, hi, out


def mask_pattern(rs, pat, hidden):
    """mask_pat.cpp:89-95: every byte that is not '.' and whose site is hidden becomes '.'"""
    return bytes(0x2e if (rs + i) in hidden else c for i, c in enumerate(pat))


def cut(rs, pat, hidden, s, e, strict=False, strip=True, no_gaps=False, min_len=1):
    """the masked cut on one read -> (rs', pattern) or None: selection and --strict on the read as it is, the mask, then strip /
    min_len / no_gaps (view_ref.cut's steps 3-5) on what the mask leaves"""
    if rs >= e or rs + len(pat) - 1 < s:
        return None
    if strict:
        pat = pat[max(0, s - rs):]
        rs = max(rs, s)
        pat = pat[:e - rs]
    return VR.cut(rs, mask_pattern(rs, pat, hidden), rs, rs + len(pat), strip=strip, no_gaps=no_gaps, min_len=min_len)


def mask_pat(text, blocks, s, e, **flags):
    """the output text (bytes) of mask_pat over [s, e); Refused(kind, offset) as the device refuses: the first malformed line, else the
    first descending read, else the first count below 1"""
    reads = VR.reads_of(text)
    low = MR.low_count(text)
    if low is not None:
        raise Refused('low', low)
    hidden = Hidden(blocks)
    lines = []
    for chrom, rs, pat, count in reads:
        c = cut(rs, pat, hidden, s, e, **flags)
        if c is not None:
            lines.append((chrom, c[0], c[1], count))
    runs = VR.collapse(sorted(lines, key=VR.sort_key))
    if any(r[3] >= VR.MAX_SUM for r in runs):
        raise Refused('sum')
    return b''.join(b'%s\t%d\t%s\t%d\n' % r for r in runs)
