#!/usr/bin/env python3
"""Golden vectors of `wgbstools test_bimodal` from the REFERENCE ITSELF: the cases of tests/bimodal_cases.py through the
reference's own src/python/test_bimodal.py (imported, its test_multiple_regions / test_single_region / read_pat_vis /
calc_initial_liklihood / em_pat_matrix run unchanged).  Runs only where a checkout of the reference lies:
REF_ROOT=<its root> python tests/golden/make_golden_bimodal.py.  What is replaced, and only that:
  * statsmodels (not installed where the goldens are made): a stub `statsmodels.stats.multitest.multipletests` goes into
    sys.modules before the import.  It computes method='fdr_bh' as statsmodels does: p as a float array, sorted; reject =
    p_sorted <= (i / n) * alpha, every index up to the last rejection rejected too; corrected = minimum.accumulate of
    (p_sorted / (i / n)) reversed, clipped to 1; both put back in the input order.
  * subprocess.check_output inside the imported module: an in-memory `tabix` (no htslib here) over the case's pat text
    (`tabix x.pat.gz chrom:a-b`: the lines of chrom with a <= start <= b, i.e. an index built with -b 2 -e 2) and blocks
    text (`tabix blocks chrom`: the lines of chrom, file order, '#' lines skipped).
  * GenomeRefPaths: the cases' synthetic genome (its chromosome list), as in make_golden_convert.py; Pool: in-process.
The reference's output depends on its host (numpy's SIMD log2, BLAS's order of summation); the test restatement
tests/bimodal_ref.py fixes both.  A case is stored only when the restatement prints exactly what the reference printed; the
number of cases dropped, and why, is recorded (`dropped`).

Writes tests/golden/bimodal_cases.json: per case the generator parameters, the arguments, the sha1 of the pat text, the
reference's printed output, and per block (genome order) [ll0, ll_em, columns, rows, p] as the reference computes them."""
import contextlib
import hashlib
import io
import json
import os
import os.path as op
import sys
import tempfile
import types

import numpy as np

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(op.dirname(HERE))
REF = os.environ.get('REF_ROOT', '')
if not op.isfile(op.join(REF, 'src', 'python', 'test_bimodal.py')):
    sys.exit('set REF_ROOT to the root of a wgbs_tools checkout')
sys.path.insert(0, ROOT)
sys.path.insert(0, op.join(ROOT, 'tests'))
sys.path.insert(0, op.join(REF, 'src', 'python'))

import bimodal_cases as BC                          # noqa: E402
import bimodal_ref as BR                            # noqa: E402


def multipletests(pvals, alpha=0.05, method='hs', is_sorted=False, returnsorted=False):
    assert method == 'fdr_bh'
    p = np.asarray(pvals)
    order = np.argsort(p)
    ps = np.take(p, order)
    n = len(ps)
    ecdf = np.arange(1, n + 1) / float(n)
    reject = ps <= ecdf * alpha
    if reject.any():
        reject[:int(np.nonzero(reject)[0].max()) + 1] = True
    corr = np.minimum.accumulate((ps / ecdf)[::-1])[::-1]
    corr[corr > 1] = 1
    r_out = np.empty_like(reject)
    r_out[order] = reject
    c_out = np.empty_like(corr)
    c_out[order] = corr
    return r_out, c_out, None, None


def install_stub():
    sm = types.ModuleType('statsmodels')
    st = types.ModuleType('statsmodels.stats')
    mt = types.ModuleType('statsmodels.stats.multitest')
    mt.multipletests = multipletests
    sm.stats, st.multitest = st, mt
    sys.modules.update({'statsmodels': sm, 'statsmodels.stats': st, 'statsmodels.stats.multitest': mt})


class Tabix:
    """check_output('tabix FILE REGION', shell=True) over registered texts"""

    def __init__(self):
        self.texts = {}

    def check_output(self, cmd, shell=True):
        _, path, region = cmd.split()
        text = self.texts[path]
        chrom, lo, hi = region, None, None
        if ':' in region:
            chrom, rng = region.split(':')
            lo, hi = (int(x) for x in rng.split('-'))
        out = []
        for ln in text.splitlines(keepends=True):
            if ln.startswith('#') or not ln.strip():
                continue
            t = ln.split('\t')
            if t[0] != chrom:
                continue
            if lo is None or lo <= int(t[1]) <= hi:
                out.append(ln)
        return ''.join(out).encode()


def main():
    install_stub()
    import test_bimodal as rt
    tabix = Tabix()
    rt.subprocess = types.SimpleNamespace(check_output=tabix.check_output)
    chroms = tuple(c for c, _ in BC.CHROMS)
    rt.GenomeRefPaths = lambda *a, **k: types.SimpleNamespace(get_chroms=lambda: chroms)

    class FakePool:
        def __init__(self, n):
            pass

        def starmap(self, f, ps):
            return [f(*p) for p in ps]

        def close(self):
            pass

        def join(self):
            pass
    rt.Pool = FakePool
    tmp = tempfile.mkdtemp(prefix='bimodal_golden_')
    out, dropped = {}, []
    for name, case in BC.CASES.items():
        pat_text, bed_text, args = BC.case_inputs(case)
        pat = op.join(tmp, name + '.pat.gz')
        tabix.texts[pat] = pat_text.decode()
        strict = '--strict' in args
        min_len = int(args[args.index('--min_len') + 1]) if '--min_len' in args else 1
        starts, reads = BR.parse_pat(pat_text)
        rec = dict(pat=case['pat'], args=args, pat_sha1=hashlib.sha1(pat_text).hexdigest())
        if bed_text is None:
            s1, s2 = case['sites']
            chrom = BC.chrom_of([s1])[0]
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rt.test_single_region(pat, chrom, (s1, s2), strict, min_len)
            text = buf.getvalue()
            blocks = [(s1, s2, chrom)]
            rec['sites'] = [s1, s2]
            mine = BR.single_text(BR.block_result(starts, reads, s1, s2, strict, min_len))
        else:
            bed = op.join(tmp, name + '.bed')
            with open(bed, 'w') as f:
                f.write(bed_text)
            tabix.texts[bed] = bed_text
            o = op.join(tmp, name + '.out')
            rt.test_multiple_regions(bed, pat, 1, o, strict, min_len, False, '--print_all_regions' in args)
            text = open(o).read() if op.isfile(o) else ''
            rec['blocks'] = case['blocks']
            rec['bed'] = case['bed']
            rec['bed_sha1'] = hashlib.sha1(bed_text.encode()).hexdigest()
            lines = [ln for c in chroms for ln in bed_text.splitlines() if not ln.startswith('#') and ln.split('\t')[0] == c]
            blocks = [(int(ln.split('\t')[3]), int(ln.split('\t')[4]), ln.split('\t')[0]) for ln in lines]
            res = [BR.block_result(starts, reads, a, b, strict, min_len) for a, b, _ in blocks]
            p32 = np.array([BR.pvalue(r[0], r[1], r[3], r[4]) for r in res]).astype(np.float32)
            mine = BR.multi_text(lines, p32, '--print_all_regions' in args)
        per_block = []
        for s1, s2, chrom in blocks:
            mat = rt.read_pat_vis(rt.pull_pat_file(f'{chrom}:{max(1, s1 - 150)}-{s2 - 1}', pat), s1, s2, strict, min_len)
            if mat.shape[0] == 0:
                per_block.append([0.0, 0.0, int(mat.shape[1]), 0, 1.0])
                continue
            ll0 = float(rt.calc_initial_liklihood(mat, should_print=False))
            ll = float(rt.em_pat_matrix(mat, should_print=False))
            p = float(rt.test_single_region(pat, chrom, (s1, s2), strict, min_len, should_print=False))
            per_block.append([ll0, ll, int(mat.shape[1]), int(mat.shape[0]), p])
        rec['text'] = text
        rec['per_block'] = per_block
        if mine != text:
            dropped.append(dict(case=name, why='the restatement prints other text (near-ties of the host-dependent arithmetic)'))
            print(name, 'DROPPED', flush=True)
            continue
        out[name] = rec
        print(name, len(per_block), 'blocks,', text.count('\n'), 'output lines', flush=True)
    with open(op.join(HERE, 'bimodal_cases.json'), 'w') as f:
        json.dump(dict(cases=out, dropped=dropped, n_cases=len(BC.CASES)), f, indent=0)


if __name__ == '__main__':
    main()
