"""numpy restatement of `wgbstools beta_to_450k` (reference: src/python/beta_to_450k.py, utils_wgbs.py:270-274), the yardstick of
the beta_to_450k tests: the map and ref files read with the csv module, the right merge by hand, every value as Python's own
'%.3f' of one double division.  No pandas, no GPU.  tests/golden/make_golden_450k.py holds it against the reference's text."""
import csv
import gzip
import io
import os.path as op

import numpy as np

TAG = '[wt beta_450K] '
EPIC_IGNORED = TAG + ('WARNING: current setup does not support translationto EPIC array.\n'
                      'Try re-installing wgbstools and re-initializing current genome.\n--EPIC flag is ignored')
REF_AND_EPIC = TAG + 'WARNING: --ref is provided, therefore EPIC flag is ignored'
MAP = '{MAP}'                                   # stands for the map file's path in a recorded warning


def read_map(path):
    """rows [ilmn, cpg or None, array or None] and the number of columns"""
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rt', newline='') as f:
        rows = [r for r in csv.reader(f, delimiter='\t') if r]
    width = max(len(r) for r in rows)
    out = [[r[0], int(float(r[1])) if len(r) > 1 and r[1] != '' else None, int(r[2]) if width > 2 else None] for r in rows]
    return out, width


def read_ref(path):
    """the first field of every row (None when empty), the header row dropped"""
    with open(path, newline='') as f:
        ids = [(r[0] if r[0] != '' else None) for r in csv.reader(f) if r]
    if ids and (ids[0] is None or not ids[0].startswith('cg')):
        ids = ids[1:]
    return ids


def select(map_rows, width, ref_ids=None, epic=False):
    """-> (IDs, 1-based cpg as int64, warnings): the output's rows and what the reference says on stderr on the way"""
    warnings = []
    if width < 3 and epic:
        warnings.append(EPIC_IGNORED)
    if width >= 3 and not epic and ref_ids is None:
        map_rows = [r for r in map_rows if r[2] == 450]
    map_rows = [r for r in map_rows if r[1] is not None]
    if ref_ids is None:
        return [r[0] for r in map_rows], np.array([r[1] for r in map_rows], dtype=np.int64), warnings
    ids, cpg, missing = [], [], []
    for i in ref_ids:
        hits = [r for r in map_rows if r[0] == i] if i is not None else []
        if not hits:
            missing.append('nan' if i is None else i)
        ids += [r[0] for r in hits]
        cpg += [r[1] for r in hits]
    if missing:
        msg = 'WARNING: Skipping %d unrecognized Illumina IDs (not found in the map table %s)\n' % (len(missing), MAP)
        msg += 'Example for missing sites: ' + ','.join(missing[:5])
        if not epic:
            msg += '\nconsider using --EPIC flag'
        warnings.append(TAG + msg)
    return ids, np.array(cpg, dtype=np.int64), warnings


def quoted(text):
    buf = io.StringIO()
    csv.writer(buf, lineterminator='\n').writerow([text, ''])
    return buf.getvalue()[:-2]


def value_texts(cells, min_cov):
    """[...] of (meth, cov) pairs in the last axis -> object array of their texts: every distinct pair is formatted once"""
    cells = np.asarray(cells)
    key = cells[..., 0].astype(np.int64) << 16 | cells[..., 1].astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    texts = np.empty(uniq.size, dtype=object)
    for at, k in enumerate(uniq.tolist()):
        m, c = k >> 16, k & 0xffff
        if c < min_cov or (c == 0 and m == 0):
            texts[at] = 'NA'
        elif c == 0:
            texts[at] = 'inf'
        else:
            texts[at] = '%.3f' % (m / c)
    return texts[inv.reshape(key.shape)]


def table_body(labels, site0, rows, min_cov):
    """the lines below the header: `labels` as they are printed, site0 0-based, rows: list of [n, 2] arrays, a column each"""
    site0 = np.asarray(site0, dtype=np.int64)
    if not site0.size:
        return b''
    cells = np.stack([np.asarray(r).reshape(-1, 2)[site0] for r in rows], axis=1)       # [rows][cols][2]
    texts = value_texts(cells, min_cov)
    return ''.join('%s,%s\n' % (lab, ','.join(t)) for lab, t in zip(labels, texts.tolist())).encode()


def columns_of(names):
    """header names and per name the index of the file it shows: the first file's place, the last file's values"""
    last = {}
    for at, n in enumerate(names):
        last[n] = at
    return list(last), [last[n] for n in last]


def table_text(ids, cpg, names, rows, cov_thresh):
    names, files = columns_of(names)
    header = ','.join(quoted(n) for n in ['ilmn'] + names) + '\n'
    return header.encode() + table_body([quoted(i) for i in ids], cpg - 1, [rows[f] for f in files], max(0, cov_thresh))


def case_text(w, case, map_path, ref_path, paths, rows):
    """-> (text, warnings) of a case of tests/array_cases.py over a written world"""
    warnings = [REF_AND_EPIC] if case['epic'] and case['ref'] else []
    map_rows, width = read_map(map_path)
    ids, cpg, more = select(map_rows, width, read_ref(ref_path) if ref_path else None, case['epic'])
    names = [op.splitext(op.basename(p))[0] for p in paths]
    return table_text(ids, cpg, names, rows, case['c']), warnings + more
