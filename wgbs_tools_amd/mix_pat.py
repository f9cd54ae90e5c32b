"""`wgbstools mix_pat` on MI355X: in-silico mixtures of pat files — the reads of K files thinned to the rates that give the requested
proportions at the requested coverage, tagged with their source and pooled into one sorted, collapsed `.pat.gz` per repetition: ground
truth for deconvolution and marker work.

Drop-in for the reference's src/python/mix_pat.py (same flags; same output names), written against its contract (mix_pat.py:18-181,
merge.py:17-100, cview.py:25-67, src/pat_sampler/sampler.cpp, src/collapse_pat.pl):

    rates     --rates holds K or K - 1 values (the last one is then 1 - their sum); their sum is 1 within 1e-8, each lies in [0, 1]
    coverage  per file beta_cov of `<pat minus .pat.gz>.beta` (`.lbeta` with -l) over the interval of -s / -r, or over the whole genome;
              a missing file is made with pat2beta next to the pat file first.  --cov defaults to the coverage of the file with the
              highest rate.
    adjusted  adj[i] = rate[i] * cov / covs[i]; above 1 it warns (`... has low coverage. Reads will be duplicated`) and goes on
    sampler   ss = adj; rep = 1; while ss > 0.25: rep *= 2; ss /= 2.  ss is printed as %.6f and read back as a float32: p is that
              float32, T = floor(p * 2^32)
    per line  of a read that survives the cut of --strict / --strip / --min_len over the interval: new = Binomial(count * rep, p); the
              line goes on with the count `new` when new > 0 and is dropped otherwise
    per file  sorted, collapsed, a fifth column `\\t<label>` appended; labels default to the files' names without directory and
              .pat.gz, one per file, distinct
    together  `LC_ALL=C sort -m -k2,2n -k3,3`, collapsed again (lines of two labels never merge), BGZF: by start as a number, the
              pattern's bytes (a prefix first), then sort's whole-line last resort — the chromosome, the decimal TEXT of the count
              ("1" < "10" < "9"), the label's bytes
    output    `<prefix>_<rep + 1>.pat.gz` for every repetition of --reps; without -p the prefix is
              `<out_dir>/<name1>_<rate1>_<name2>_<rate2>..._cov_<%.2f>[_<region>]`; an existing output is skipped unless -f

One repetition is one `view` engine (view.view_pats with sources=): every file is fed to it with wgbsseg_patview_set_source in front, the
draws, the sort, the collapse, the order of tied lines, the label column and the BGZF deflate happen on the device
(csrc/view_kernels.h).  Coverages come through this build's pat2beta and beta_cov.  No CPU fallback.

Deliberate deviations from the reference:
  1. The generator.  The reference seeds a fresh std::default_random_engine from the clock for every line, so no run can be repeated,
     not even by itself.  Here draw j of a line is word j & 3 of Philox4x32-10 with counter {byte offset of the line in its file's
     text (64 bits), j >> 2, rep << 16 | file} and key --seed (csrc/view_core.h wg_view_sample): the law is the same Binomial(count *
     rep, p), the bits are this build's own.  --seed N is new; without it the seed comes from os.urandom and is printed on stderr, so
     the run can be repeated.  The same seed gives the same bytes, whatever --inflate says and however the file is cut into chunks.
  2. No `.csi` index is written (this build never reads one); one line on stderr says so.
  3. -L / --bed_file is refused as not part of this build.
  4. The whole genome is one pass and one sort by (start, pattern, chromosome) like `merge` here, not the reference's branch that
     leaves whole-genome views unsorted before `sort -m`.
  5. A line with count * rep above 2^20 is refused (`failed in view: [file K: ]count * reps above 2^20 at byte N`), not looped over: pat
     files written by wgbstools hold small counts.  A count below 1 is refused as in `merge`.
  6. Labels: printable ASCII without white space, '/', '&' and '\\' (what goes through the reference's `sed 's/$/\\tLABEL/'` untouched).
     --no_gaps, --no_sort, --shuffle and -np are accepted and change nothing, as in the reference; -T and -@ are accepted and unused:
     nothing is sorted on disk, and the repetitions run one after another on the device.
"""
import argparse
import os
import os.path as op

import numpy as np

from .beta_cov import beta_cov
from .cliutil import add_threads_option, add_where_options, require_file
from .genome import GenomicRegion, IllegalArgumentError, eprint
from .merge import IGNORED_VIEW_FLAGS, merge_interval
from .pat2beta import add_inflate_option, pat2beta
from .view import _write_all, view_pats

MAX_LABELS = 255
SS_TH = 0.25


def pretty_name(path):
    """utils_wgbs.py pretty_name: the basename without .pat.gz"""
    name = op.basename(path)
    return name[:-7] if name.endswith('.pat.gz') else op.splitext(name)[0]


def validate_rates(rates, nr_pats):
    """mix_pat.py:72-86 -> the K rates"""
    rates = [float(r) for r in rates]
    if len(rates) == nr_pats - 1:
        rates.append(1.0 - float(np.sum(rates)))
    if len(rates) != nr_pats:
        raise IllegalArgumentError('len(rates) must be in {len(files), len(files) - 1}')
    if abs(float(np.sum(rates)) - 1) > 1e-8:
        raise IllegalArgumentError(f'Sum(rates) == {np.sum(rates)} != 1')
    if min(rates) < 0 or max(rates) > 1:
        raise IllegalArgumentError('rates must be in range [0, 1)')
    return rates


def adjust_rates(rates, covs, cov=None, pats=None):
    """mix_pat.py:101-114 -> (the coverage aimed at, the adjusted rates)"""
    if not cov:
        cov = covs[int(np.argmax(rates))]
    adj = []
    for i, (r, c) in enumerate(zip(rates, covs)):
        if not c > 0:
            raise IllegalArgumentError(f'mix_pat: {pats[i] if pats else "file %d" % i} has coverage {c} over the interval: nothing to sample from')
        a = r * cov / c
        if a > 1:
            eprint(f'[wt mix] WARNING: {pats[i] if pats else "file %d" % i} has low coverage. Reads will be duplicated')
        adj.append(a)
    return cov, adj


def sampler_args(adj):
    """cview.py:55-67 and sampler.cpp:62: an adjusted rate -> (T, reps, p): ss halves until it is at most 0.25 while reps doubles; the
    sampler reads `%.6f` of it with std::stof, so p is the float32 nearest to that text and T = floor(p * 2^32), exact in double"""
    ss, reps = float(adj), 1
    if not (ss >= 0) or ss == float('inf'):
        raise IllegalArgumentError(f'mix_pat: adjusted rate {adj}')
    while ss > SS_TH:
        reps *= 2
        ss /= 2
    p = float(np.float32('%.6f' % ss))
    return int(p * 4294967296.0), reps, p


def validate_labels(labels, pats):
    """merge.py validate_labels(required=True) and deviation 6 -> one label per file"""
    if not labels:
        labels = [pretty_name(p) for p in pats]
    if len(labels) != len(pats):
        raise IllegalArgumentError('[wt mix] ERROR: the number of labels must be the number of pat files')
    if len(set(labels)) != len(labels):
        raise IllegalArgumentError('[wt mix] ERROR: labels must be distinct')
    if len(labels) > MAX_LABELS:
        raise IllegalArgumentError(f'mix_pat: {len(labels)} files (at most {MAX_LABELS})')
    for lab in labels:
        if not lab or any(c <= ' ' or c > '~' or c in '/&\\' for c in lab):
            raise IllegalArgumentError(f'mix_pat: the label {lab!r} is not part of this build: printable ASCII without white space, "/", "&" and "\\"')
    return list(labels)


def generate_prefix(out_dir, prefix, pats, rates, cov, gr):
    """mix_pat.py:35-49"""
    if prefix:
        d = op.dirname(prefix)
        if d and not op.isdir(d):
            raise IllegalArgumentError(f'Invalid dir: {d}')
        return prefix
    if not op.isdir(out_dir):
        raise IllegalArgumentError(f'Invalid dir: {out_dir}')
    res = '_'.join(str(x) for t in zip([pretty_name(f) for f in pats], rates) for x in t)
    res += '_cov_{:.2f}{}'.format(cov, '' if gr.sites is None else f'_{gr.region_str}')
    return op.join(out_dir, res)


def read_covs(pats, args, gr):
    """mix_pat.py:88-99: the coverage of every file's beta over the interval; a missing beta is made next to its pat first"""
    suff = '.lbeta' if args.lbeta else '.beta'
    betas = []
    for pat in pats:
        beta = pat[:-7] + suff
        if not op.isfile(beta):
            eprint(f'[wt mix] No {suff} file compatible to {pat} was found. Generating it...')
            pat2beta(pat, op.dirname(pat) or '.', args=args, force=True)
        betas.append(beta)
    sites = None if gr.sites is None else tuple(int(x) for x in gr.sites)
    return [float(c) for c in beta_cov(betas, sites=sites, device=args.device)]


def rates_table(names, rates, covs, adj):
    """the reference prints a DataFrame; here plain aligned text with its three columns"""
    w = max([len(n) for n in names] + [1])
    cols = ('ReqstRates', 'OrigCov', 'AdjRates')
    lines = [' ' * w + ''.join('%12s' % c for c in cols)]
    for n, r, c, a in zip(names, rates, covs, adj):
        lines.append(n.ljust(w) + '%12.6f%12.6f%12.6f' % (r, c, a))
    return '\n'.join(lines)


def mix_once(pats, out_path, s, e, per_file, seed, rep, strict=False, strip=False, min_len=1, device=0, inflate='host', timings=None):
    """repetition `rep` of the mixture of `pats` over [s, e), as BGZF members to out_path -> (lines, bytes written).
    per_file: (label, T, reps) of every file."""
    tmp = out_path + '.tmp%d' % os.getpid()                         # (a refused input leaves no half-written output behind)
    try:
        with open(tmp, 'wb') as f:
            got = view_pats(pats, s, e, lambda piece: _write_all(f.fileno(), piece), strict=strict, strip=strip, min_len=min_len, sort=True,
                            device=device, inflate=inflate, deflate=True, timings=timings, sources=(per_file, seed, rep))
        os.replace(tmp, out_path)
    finally:
        if op.isfile(tmp):
            os.remove(tmp)
    return got


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('pat_files', nargs='+', help='Two or more pat files')
    parser.add_argument('-c', '--cov', type=float,
                        help='Coverage of the output pat. Default the coverage of the file with the highest rate. The beta files beside '
                             'the pat files are read for it; a missing one is created.')
    parser.add_argument('-f', '--force', action='store_true', help='Overwrite existing files if existed')
    parser.add_argument('--reps', type=int, default=1, help='nr or repetitions [1]')
    parser.add_argument('--rates', type=float, metavar='[0.0, 1.0]', nargs='+', required=True,
                        help='Rates for each of the pat files. Note: the order matters! Rate of for the last file may be omitted. '
                             'The rates will be adjusted s.t the output will be of the requested coverage.')
    parser.add_argument('--labels', nargs='+', help='labels for the mixed reads. Default is the basenames of the pat files')
    out_or_pref = parser.add_mutually_exclusive_group()
    out_or_pref.add_argument('-p', '--prefix', help='Prefix of output file.')
    out_or_pref.add_argument('-o', '--out_dir', help='Output directory [.]', default='.')
    parser.add_argument('-T', '--temp_dir', help='accepted and unused: nothing is sorted on disk')
    parser.add_argument('-l', '--lbeta', action='store_true', help='Use lbeta file (uint16) instead of beta (uint8)')
    parser.add_argument('-v', '--verbose', action='store_true')
    add_where_options(parser, bed_file=True)
    parser.add_argument('--strict', action='store_true', help='cut every read to the interval of -s / -r')
    parser.add_argument('--strip', action='store_true', help='remove the dots at both ends of a read (its start moves with them)')
    parser.add_argument('--min_len', type=int, default=1, help='drop reads left with fewer than MIN_LEN sites [1]')
    parser.add_argument('--no_gaps', action='store_true', help='accepted; changes nothing (as in the reference)')
    parser.add_argument('--shuffle', action='store_true', help='accepted; changes nothing (as in the reference)')
    parser.add_argument('--no_sort', action='store_true', help='accepted; changes nothing (as in the reference)')
    parser.add_argument('-np', '--nanopore', action='store_true', help='accepted; the whole of every file is read in any case')
    add_threads_option(parser)
    parser.add_argument('--seed', type=int, help='seed of the sampler, 0 <= N < 2^64 [from os.urandom; printed on stderr]')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    add_inflate_option(parser)
    return parser.parse_args(argv)


def check_args(args):
    """everything that can be refused before a file is read -> (rates, labels)"""
    if args.bed_file:
        raise IllegalArgumentError('mix_pat -L / --bed_file is not part of this build')
    if len(args.pat_files) < 2:
        raise IllegalArgumentError('Input error: at least 2 input files must be given')
    for p in args.pat_files:
        require_file(p, '.pat.gz')
    if args.min_len < 1:
        raise IllegalArgumentError(f'--min_len must be at least 1 (got {args.min_len})')
    if args.reps < 0 or args.reps > 65536:
        raise IllegalArgumentError(f'--reps must lie in [0, 65536] (got {args.reps})')
    if args.seed is not None and not 0 <= args.seed < 2 ** 64:
        raise IllegalArgumentError(f'--seed must lie in [0, 2^64) (got {args.seed})')
    if args.cov is not None and not args.cov >= 0:
        raise IllegalArgumentError(f'--cov must not be negative (got {args.cov})')
    return validate_rates(args.rates, len(args.pat_files)), validate_labels(args.labels, args.pat_files)


def main(argv=None):
    """
    Mix samples from K different pat files.
    Output a single mixed pat.gz file per repetition - sorted and bgzipped -
    with an informative name; every read carries the label of its source.
    """
    args = parse_args(argv)
    rates, labels = check_args(args)
    pats = args.pat_files
    gr = GenomicRegion(args)
    covs = read_covs(pats, args, gr)
    cov, adj = adjust_rates(rates, covs, args.cov, pats)
    prefix = generate_prefix(args.out_dir, args.prefix, pats, rates, cov, gr)
    outs = [prefix + f'_{rep + 1}.pat.gz' for rep in range(args.reps)]
    real = [op.realpath(p) for p in pats]
    for o in outs:
        if op.realpath(o) in real:
            raise IllegalArgumentError(f'mix_pat: the output path is identical to one of the input files: {o}')
    eprint('Requested Coverage: {:.2f}'.format(cov))
    eprint(rates_table([pretty_name(p) for p in pats], rates, covs, adj))
    given = [flag for name, flag in IGNORED_VIEW_FLAGS if getattr(args, name)]
    if given:
        eprint(f'[wt mix] {", ".join(given)}: accepted and without effect on mix_pat, as in the reference')
    seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(8), 'little')
    if args.seed is None:
        eprint(f'[wt mix] --seed {seed}')
    per_file = [(lab,) + sampler_args(a)[:2] for lab, a in zip(labels, adj)]
    s, e = merge_interval(gr)
    for rep, mix_i in enumerate(outs):
        if op.isfile(mix_i) and not args.force:
            eprint(f'File {mix_i} already exists. Skipping it. Use [-f] flag to force overwrite.')
            continue
        eprint(f'[wt mix] mix: {mix_i}')
        t = {}
        lines, nbytes = mix_once(pats, mix_i, s, e, per_file, seed, rep, strict=args.strict, strip=args.strip, min_len=args.min_len,
                                 device=args.device, inflate=args.inflate, timings=t)
        if args.verbose:
            eprint(f'[wt mix] {t.get("sampled_reads", 0)} reads drawn, {t.get("sampled_dropped", 0)} dropped, counts kept {t.get("sampled_kept", 0)} '
                   f'-> {lines} lines, {nbytes} bytes in {mix_i}')
        eprint(f'[wt mix] no .csi index is written for {mix_i}: this build reads pat files without one')


if __name__ == '__main__':
    main()
