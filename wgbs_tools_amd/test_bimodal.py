"""`wgbstools test_bimodal` on MI355X: per block, is there evidence that the reads come from two methylation states (alleles)
rather than one?  Imprinted regions and allele-specific methylation are found this way.

Drop-in for the reference's src/python/test_bimodal.py (same flags, messages and output text), written against its contract:

    reads     for block [s1, s2) the pat lines starting in [max(1, s1 - 150), s2 - 1] (the reference's tabix query), minus those
              ending at or before s1; --strict clips them to [s1, s2); shorter than --min_len: dropped.  Each line stands for
              `count` identical rows; the columns run from the first accepted read's (clipped) start to the largest unclipped end.
    test      ll0: one allele per column; ll_em: the reference's hard-assignment EM over two alleles (priors fixed at 0.5, started
              from p_C = {0.9, 0.1}); p = 1 - chi2.cdf(2 ln 2 (ll_em - ll0), columns), and 1 for a block without rows.  The EM
              runs on the GPU as the pat text streams past (k_bim_em, csrc/bimodal_kernels.h, which gives the arithmetic).
    -L BED    blocks of the genome's chromosomes in its order, file order within each; a stable sort by float32 p; Benjamini-
              Hochberg at 0.05 as statsmodels' fdr_bh computes it; printed are the line of each block and its corrected p
              (`,.1e`) up to the first block not rejected — nothing when the first is not rejected, and nothing when every block is
              (the reference's argmax quirk); --print_all_regions prints every block.
    -s/-r     the three lines "LL: ... | BPI: ..." (ll0), the same for ll_em, "pvalue: ..." — nothing for a block without rows.

Deliberate deviations from the reference:
  1. No `.csi` / tabix index is needed on the pat file or on the blocks file: the whole pat file is read once, the blocks file
     is read as text (gzip or plain; '#' lines and a header line skipped).
  2. The pat file's chromosome column is not consulted: CpG indexes are genome-wide, so a block's reads are found by index.
  3. -L honours --genome for the list of chromosomes (the reference lists those of the default genome whatever --genome says).
  4. Refused with a message where the reference crashes or computes on garbage: malformed pat lines, reads that start before
     the read before them and negative counts (each naming its byte offset), blocks whose CpG columns are NA or not integers,
     blocks with endCpG <= startCpG or startCpG < 1, --min_len below 1.

No CPU fallback: the EM runs on the GPU (wgbsseg_bimodal_*, include/wgbsseg.h); the host keeps scipy's chi-square, the
Benjamini-Hochberg step and the text.
"""
import argparse
import gzip
import os.path as op
import sys
import time

import numpy as np

from .cliutil import add_threads_option, add_where_options, require_file
from .genome import GenomeRefPaths, GenomicRegion, IllegalArgumentError, eprint
from .pat2beta import feed_pat


def _stats():
    try:
        from scipy import stats
    except ImportError:
        raise IllegalArgumentError('Please install scipy in order to use this feature (its chi-square distribution). i.e. "pip install scipy"')
    return stats


def run_blocks(pat, starts, ends, strict, min_len, device=0, timings=None, max_lds_cols=-1):
    """the device's raw numbers per block: (float64 [n][3] ll0, ll_em, sum of n_per_col; int64 [n][3] columns, rows, iterations)"""
    from . import _lib
    t = timings if timings is not None else {}
    with _lib.Bimodal(starts, ends, strict, min_len, device=device, max_lds_cols=max_lds_cols) as b:
        feed_pat(b, pat, t)
        t0 = time.perf_counter()
        try:
            ll, cnt = b.finish()
        except _lib.SegmentorError as e:
            raise IllegalArgumentError(f'{pat}: {e.msg}')
        t['finish_s'] = time.perf_counter() - t0
        t['kernel_ms'] = b.kernel_ms()
    return ll, cnt


def pvalues(ll, cnt):
    """test_single_region's p per block (float64): 1 - chi2.cdf(2 ln 2 (ll_em - ll0), columns); 1 for a block without rows"""
    stats = _stats()
    rows = cnt[:, 1]
    p = np.ones(len(rows), dtype=np.float64)
    has = rows > 0
    if has.any():
        p[has] = 1 - stats.chi2.cdf(2 * np.log(2) * (ll[has, 1] - ll[has, 0]), cnt[has, 0])
    return p


def fdr_bh(p_sorted, alpha=0.05):
    """statsmodels.stats.multitest.multipletests(p, alpha, method='fdr_bh') on ascending p: (reject, corrected)"""
    p = np.asarray(p_sorted).astype(np.float64)
    n = p.size
    ecdf = np.arange(1, n + 1) / float(n)
    reject = p <= ecdf * alpha
    if reject.any():
        reject[:int(np.nonzero(reject)[0].max()) + 1] = True
    corrected = np.minimum.accumulate((p / ecdf)[::-1])[::-1]
    corrected[corrected > 1] = 1
    return reject, corrected


def choose_by_fdr(lines, p32, print_all=False):
    """the stable sort by float32 p, then choose_blocks_by_fdr_bh (:100-110) -> [(line, corrected p)]"""
    if not lines:
        return []
    p32 = np.asarray(p32, dtype=np.float32)
    order = np.argsort(p32, kind='stable')
    reject, corrected = fdr_bh(p32[order])
    if not reject[0]:
        return []
    k = len(order) if print_all else int(np.argmax(1 - reject))
    return [(lines[i], corrected[r]) for r, i in enumerate(order[:k].tolist())]


def _open_text(path):
    if path.endswith('.gz'):
        return gzip.open(path, 'rt')
    return open(path, 'r')


def read_bed(path):
    """the data lines of a blocks file: [(line text, tokens)] ('#' lines, empty lines and a header line skipped); fewer than five
    columns in the first line: the reference's message"""
    require_file(path)
    rows = []
    with _open_text(path) as f:
        for raw in f:
            line = raw.rstrip('\n')
            if not line.strip() or line.startswith('#'):
                continue
            tok = line.split('\t')
            if not rows:
                if len(line.split('#', 1)[0].split('\t')) < 5:
                    msg = f'Invalid blocks file: {path}. less than 5 columns.\n'
                    msg += f'Run wgbstools convert -L {path} -o OUTPUT_REGION_FILE to add the CpG columns'
                    raise IllegalArgumentError(msg)
                if not tok[1].strip().isdigit():                   # a header line
                    rows.append(None)
                    continue
            rows.append((line, tok))
    return [r for r in rows if r is not None]


def _cpg(tok, k, path, row):
    try:
        return int(tok[k])
    except (ValueError, IndexError):
        raise IllegalArgumentError(f'Invalid blocks file: {path}: row {row} has no integer CpG index in column {k + 1}: {tok[k] if k < len(tok) else ""!r}')


def select_blocks(rows, chroms, path):
    """the reference's order: chromosome by chromosome as the genome lists them, file order within; other chromosomes dropped"""
    by_chrom = {}
    for n, (line, tok) in enumerate(rows):
        by_chrom.setdefault(tok[0], []).append((n, line, tok))
    out = []
    for c in chroms:
        for n, line, tok in by_chrom.get(c, []):
            s1, s2 = _cpg(tok, 3, path, n + 1), _cpg(tok, 4, path, n + 1)
            if s1 < 1 or s2 <= s1:
                raise IllegalArgumentError(f'Invalid blocks file: {path}: row {n + 1} has startCpG {s1}, endCpG {s2} (1 <= startCpG < endCpG)')
            out.append((line, s1, s2))
    return out


def multiple_regions(args, timings=None):
    """test_multiple_regions (:178-235)"""
    rows = read_bed(args.bed_file)
    chroms = GenomeRefPaths(args.genome).get_chroms()
    blocks = select_blocks(rows, chroms, args.bed_file)
    if args.verbose:
        for c in chroms:
            eprint(f'[wt bimodal] finished processesing {c}')
    if not blocks:
        if args.verbose:
            eprint('[wt bimodal] empty list')
        return
    lines = [b[0] for b in blocks]
    ll, cnt = run_blocks(args.pat, [b[1] for b in blocks], [b[2] for b in blocks], args.strict, args.min_len, args.device, timings)
    t0 = time.perf_counter()
    p32 = pvalues(ll, cnt).astype(np.float32)
    chosen = choose_by_fdr(lines, p32, args.print_all_regions)
    text = ''.join(f'{a}\t{c:,.1e}\n' for a, c in chosen)
    if args.out_file == '-':
        sys.stdout.write(text)
        sys.stdout.flush()
    else:
        with open(args.out_file, 'w') as f:
            f.write(text)
    if timings is not None:
        timings['write_s'] = time.perf_counter() - t0


def single_region(args):
    """test_single_region (:153-176) with its printouts"""
    gr = GenomicRegion(args)
    s1, s2 = gr.sites
    ll, cnt = run_blocks(args.pat, [s1], [s2], args.strict, args.min_len, args.device)
    ncols, rows = int(cnt[0, 0]), int(cnt[0, 1])
    if rows == 0:
        return
    ll0, ll_em, sum_n = np.float64(ll[0, 0]), np.float64(ll[0, 1]), np.float64(ll[0, 2])
    print(f'LL: {ll0} | {rows} reads | {int(round(sum_n))} observed | BPI: {2 ** (ll0 / sum_n)}')
    print(f'LL: {ll_em} | {rows} reads | {int(round(sum_n))} observed | BPI: {2 ** (ll_em / sum_n)}')
    pv = 1 - _stats().chi2.cdf(2 * np.log(2) * (ll_em - ll0), ncols)
    print(f'pvalue: {pv:,.3e}')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('pat', help='The input pat file')
    add_where_options(parser, required=True, bed_file=True)
    add_threads_option(parser)
    parser.add_argument('--strict', action='store_true', help='Truncate reads that start/end outside the given region.')
    parser.add_argument('--min_len', type=int, default=1, help='Only use reads covering at least MIN_LEN CpG sites [1]')
    parser.add_argument('--out_file', '-o', default='-', help='Output file name in which to write results')
    parser.add_argument('--verbose', '-v', action='store_true')
    parser.add_argument('--print_all_regions', action='store_true', help='Print all regions and not only the significant ones.')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    return parser.parse_args(argv)


def check_args(args):
    if args.min_len < 1:
        raise IllegalArgumentError(f'--min_len must be at least 1 (got {args.min_len})')
    require_file(args.pat)
    _stats()


def main(argv=None):
    """
    Test whether region is bimodal
    """
    args = parse_args(argv)
    check_args(args)
    if args.bed_file is not None:
        multiple_regions(args)
    else:
        single_region(args)


if __name__ == '__main__':
    main()
