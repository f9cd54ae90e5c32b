"""`wgbstools beta_to_450k` on MI355X: beta / lbeta files as one table over the sites of the Illumina 450K (or EPIC) array — a row
per probe, a column per file, `%.3f` of meth / cov or NA — the bridge from WGBS samples to array-based atlases and deconvolution.

Drop-in for the reference's src/python/beta_to_450k.py (same flags, same text, same warnings), written against its contract
(beta_to_450k.py:16-110, utils_wgbs.py:270-274):

    map       <genome>/ilmn2CpG.tsv.gz, tab-separated, no header: ilmn, cpg (1-based CpG index, may be empty), optionally array
              (450 / 850).  Two columns: every row counts as 450 and --EPIC is ignored with the reference's warning.  Without --ref
              and without --EPIC only the rows with array == 450 are kept.
    --ref     a CSV whose first column holds Illumina IDs; its first row is dropped when that field is empty or does not start
              with `cg` (a header).  The output follows the ref file's order (a right merge on the ID): an ID that repeats there
              repeats in the output, an ID with several map rows gives several rows in map order, IDs the map lacks are skipped
              with the reference's warning (count, up to five examples, the --EPIC hint).  No array filter; --EPIC with --ref warns.
    -c N      a value is NA where cov < N [3].  N <= 0 lets cov = 0 through as numpy's division does: 0 / 0 is NA, m / 0 is inf.
    text      header `ilmn,<file base names>`; two files with one base name share the first one's column, which holds the last
              one's values.  Fields are quoted as csv.QUOTE_MINIMAL does.  The header and the quoting of the labels are the host's;
              every other byte is made on the device by ONE library call over all files (wgbsseg_site_table: csrc/array_kernels.h):
              a gather of the probes' counts from the resident rows, a length pass and a scan, an emit pass that formats in LDS;
              the host hands finished slabs of text to the output while the next slab is computed.
    -o PATH   default: standard output.  A reader that goes away ends the command quietly.

Deliberate deviations from the reference: map rows with an empty cpg are dropped for every genome (the reference drops them only
for a genome NAMED hg38; elsewhere it fails or, with --ref, reports them as unrecognized); a cpg outside 1 .. the genome's sites is
refused with the probe's name (the reference reads the LAST site for 0 and raises IndexError above); EVERY file, not only the
first, must have the genome's length; no process pool: -@ is accepted and ignored; --device N is added.  No CPU fallback.
"""
import argparse
import csv
import gzip
import io
import os
import os.path as op
import sys

import numpy as np

from .beta_cov import beta_width, load_rows, pretty_name
from .cliutil import add_threads_option, require_file, require_files
from .genome import GenomeRefPaths, IllegalArgumentError, beta_sanity_check, eprint

TAG = '[wt beta_450K] '


def csv_field(text):
    """one field as csv.QUOTE_MINIMAL writes it (what pandas' to_csv does)"""
    buf = io.StringIO()
    csv.writer(buf, lineterminator='\n').writerow([text, ''])
    return buf.getvalue()[:-2]


def load_map(path, epic, has_ref):
    """beta_to_450k.py:22-48 -> (list of IDs, float array of their cpg with NaN for the empty ones), filtered to the array"""
    import pandas as pd
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        df = pd.read_csv(f, sep='\t', header=None)
    if df.shape[1] < 3:
        if epic:
            eprint(TAG + 'WARNING: current setup does not support translation'
                         'to EPIC array.\n'
                         'Try re-installing wgbstools and re-initializing current genome.'
                         '\n--EPIC flag is ignored')
        keep = np.ones(len(df), dtype=bool)
    else:
        keep = np.ones(len(df), dtype=bool) if (epic or has_ref) else (df.iloc[:, 2] == 450).values
    ids = df.iloc[:, 0].values[keep]
    cpg = pd.to_numeric(df.iloc[:, 1], errors='coerce').values.astype(np.float64)[keep]
    return list(ids), cpg


def load_ref(path):
    """beta_to_450k.py:63-69 -> the IDs of the first column, header row dropped (a missing field is None)"""
    import pandas as pd
    rf = pd.read_csv(path, header=None, usecols=[0], names=['ilmn'])
    ids = [None if pd.isna(x) else x for x in rf['ilmn'].values]
    if ids and (ids[0] is None or not str(ids[0]).startswith('cg')):
        ids = ids[1:]
    return ids


def select_probes(map_ids, map_cpg, ref_ids, epic, map_path):
    """The output's rows -> (IDs, 1-based cpg as int64).  Without a ref: the map's rows in order; with one: beta_to_450k.py:72-90."""
    known = ~np.isnan(map_cpg)                                  # (deviation: empty cpg dropped for every genome)
    ids = [i for i, k in zip(map_ids, known) if k]
    cpg = map_cpg[known].astype(np.int64)
    if ref_ids is None:
        return ids, cpg
    rows_of = {}
    for at, i in enumerate(ids):
        rows_of.setdefault(i, []).append(at)
    take, out_ids, missing = [], [], []
    for i in ref_ids:
        rows = rows_of.get(i) if i is not None else None
        if not rows:
            missing.append(i)
            continue
        take += rows
        out_ids += [i] * len(rows)
    if missing:
        msg = f'WARNING: Skipping {len(missing)} unrecognized Illumina IDs ' \
              f'(not found in the map table {map_path})\n'
        msg += 'Example for missing sites: {}'.format(','.join('nan' if m is None else str(m) for m in missing[:5]))
        if not epic:
            msg += '\nconsider using --EPIC flag'
        eprint(TAG + msg)
    return out_ids, cpg[np.asarray(take, dtype=np.int64)]


def columns_of(paths):
    """header names and, per name, the index of the file whose values it shows: the first file's place, the last file's values"""
    last = {}
    for at, p in enumerate(paths):
        last[pretty_name(p)] = at
    return list(last), [last[n] for n in last]


def betas_to_csv(paths, genome, opath, cov_thresh=3, ref=None, epic=False, device=0, slab_rows=0):
    """beta_to_450k.py:93-110"""
    from . import _lib
    if not beta_sanity_check(paths[0], genome):
        raise IllegalArgumentError('beta incompatible with genome')
    n_sites = genome.get_nr_sites()
    elem = beta_width(paths[0])
    for p in paths[1:]:
        if beta_width(p) != elem or op.getsize(p) != 2 * elem * n_sites:
            raise IllegalArgumentError(f'{p}: the file and the genome {genome.genome} differ in their number of sites')
    map_path = require_file(genome.ilmn2cpg_dict)
    map_ids, map_cpg = load_map(map_path, epic, ref is not None)
    ref_ids = load_ref(require_file(ref)) if ref is not None else None
    ids, cpg = select_probes(map_ids, map_cpg, ref_ids, epic, map_path)
    bad = np.flatnonzero((cpg < 1) | (cpg > n_sites))
    if bad.size:
        raise IllegalArgumentError(f'{map_path}: probe {ids[bad[0]]} maps to CpG {int(cpg[bad[0]])}, outside 1 .. {n_sites:,}')
    names, files = columns_of(paths)
    labels = [csv_field(str(i)).encode() for i in ids]
    lim = _lib.site_table_limits()
    for lab in labels:
        if len(lab) > lim['max_label']:
            raise IllegalArgumentError(f'Illumina ID {lab[:40].decode(errors="replace")}... has {len(lab)} bytes, at most {lim["max_label"]} are supported')
    if len(files) > lim['max_cols']:
        raise IllegalArgumentError(f'{len(files)} columns, at most {lim["max_cols"]} are supported')
    header = (','.join(csv_field(n) for n in ['ilmn'] + names) + '\n').encode()
    rows = [load_rows(paths[f]) for f in files]
    with _lib.Segmenter(device) as seg:
        (seg.set_lbetas if elem == 2 else seg.set_betas)(rows)
        out = None
        if opath is None or opath == '/dev/stdout':
            sys.stdout.flush()
            fd = 1
        else:
            out = open(opath, 'wb')
            fd = out.fileno()
        try:
            os.write(fd, header)
            try:
                seg.site_table(fd, cpg - 1, np.arange(len(files)), labels, min_cov=min(max(0, cov_thresh), 2 ** 31 - 1), slab_rows=slab_rows)
            except _lib.SegmentorError as e:
                raise IllegalArgumentError(e.msg)
        finally:
            if out:
                out.close()


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=main.__doc__)
    parser.add_argument('input_files', nargs='+', help='one or more beta files')
    parser.add_argument('-o', '--out_path', default='/dev/stdout', help='Output path. [stdout]')
    parser.add_argument('-c', '--cov_thresh', type=int, default=3,
                        help='minimal coverage to include. sites with coverage < '
                             'cov_thresh are ignored [3]')
    parser.add_argument('--ref', help='a reference file with one column, '
                                      'of Illumina IDs, optionally with a header line.')
    parser.add_argument('--EPIC', action='store_true',
                        help='If no --ref is provided, output all 850K EPIC sites, instead of only 450K')
    add_threads_option(parser)
    parser.add_argument('--genome', help='Genome reference name. Default is "default".', default='default')
    parser.add_argument('--device', type=int, default=0, help='HIP device index [0]')
    return parser.parse_args(argv)


def main(argv=None):
    """
    Convert beta (or lbeta) file[s] to Illumina-450K (or EPIC) format.
    Output: a csv file with up to ~480K (or 850K) rows, for the Illumina array sites,
            and with columns corresponding to the beta files.
            all values are in range [0, 1], or NA.
            Only works for hg19 and hg38.
    """
    args = parse_args(argv)
    if args.EPIC and args.ref:
        eprint(TAG + 'WARNING: --ref is provided, therefore EPIC flag is ignored')
    require_files(args.input_files)
    genome = GenomeRefPaths(args.genome)
    try:
        betas_to_csv(args.input_files, genome, args.out_path, args.cov_thresh, args.ref, args.EPIC, args.device)
    except BrokenPipeError:                                        # e.g. the output is piped to head
        os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())


if __name__ == '__main__':
    main()
