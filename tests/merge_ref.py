"""A plain-Python restatement of the contract of `wgbstools merge` (wgbs_tools_amd/merge.py's docstring), built on tests/view_ref.py.

pat:   per file view(text, s, e, sort=True, **flags) — the reference views, sorts and collapses every file by itself —, then the union
       of the files' lines in file order is sorted with view_ref.sort_key (stable: `sort -m` of sorted inputs) and collapsed again.
beta:  the numpy lines of the reference's merge_betas / trim_to_uint8 (merge.py:123-140, utils_wgbs.py:277-290), verbatim in meaning: an
       int64 sum, float64 m / c * max, assignment into the int array, astype.
tests/test_merge_cpu.py holds both against the goldens, the GPU tests hold the device against them."""
import numpy as np

import view_ref as VR


class Refused(Exception):
    def __init__(self, kind, file, offset):
        super().__init__('file %d: %s at %s' % (file, kind, offset))
        self.kind, self.file, self.offset = kind, file, offset


def parse_lines(text):
    out = []
    for ln in text.splitlines():
        chrom, rs, pat, count = ln.split(b'\t')
        out.append((chrom, int(rs), pat, int(count)))
    return out


def low_count(text):
    """the byte offset of the first well-formed line whose count is below 1, or None"""
    pos = 0
    for line in text.split(b'\n'):
        off, pos = pos, pos + len(line) + 1
        tok = line.split(b'\t')
        if len(tok) == 4 and VR._number(tok[3], True) is not None and VR._number(tok[3], True) < 1:
            return off
    return None


def merge_pats(texts, s, e, **flags):
    """the output text (bytes) of the merge of the pat texts over [s, e); Refused(kind, file, offset) as the device refuses: over all
    files the first malformed line, else the first descending read, else the first count below 1"""
    found = {}
    for k, text in enumerate(texts):
        try:
            VR.reads_of(text)
        except VR.Refused as r:
            found.setdefault(r.kind, (k, r.offset))             # (reads_of names a file's malformed line before its descending read)
    for kind in ('bad', 'desc'):
        if kind in found:
            raise Refused(kind, *found[kind])
    for k, text in enumerate(texts):
        off = low_count(text)
        if off is not None:
            raise Refused('low', k, off)
    lines = []
    for text in texts:
        lines += parse_lines(VR.view(text, s, e, sort=True, **flags))
    runs = VR.collapse(sorted(lines, key=VR.sort_key))
    if any(r[3] >= VR.MAX_SUM for r in runs):
        raise VR.Refused('sum')
    return b''.join(b'%s\t%d\t%s\t%d\n' % r for r in runs)


def trim_to_uint8(data, lbeta=False):
    max_val = 2 ** (16 if lbeta else 8) - 1
    big = np.argwhere(data[:, 1] > max_val).flatten()
    data[:, 0][big] = data[big][:, 0] / data[big][:, 1] * max_val
    data[:, 1][big] = max_val
    return data.astype(np.uint16 if lbeta else np.uint8)


def merge_betas(rows, lbeta=False):
    """rows: arrays [n, 2] of uint8 / uint16 -> the merged array"""
    data = np.asarray(rows[0]).astype(np.int64)
    for r in rows[1:]:
        data += np.asarray(r)
    return trim_to_uint8(data, lbeta=lbeta)
