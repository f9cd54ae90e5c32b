#!/usr/bin/python3 -u
"""`wgbstools <command>` dispatcher (reference: src/python/wgbs_tools.py:50-79).  This build carries `segment` — the
MI355X-native hot path — and the steps either side of it that work on the same resident data: `convert` (loci <-> CpG
indexes, what feeds `segment -L`), `pat2beta` (the producer of the beta files), `beta_to_blocks`, `beta_to_table` and `find_markers` (the reductions over the blocks it writes) `homog` (the
reads' U / X / M counts over those blocks), `test_bimodal` (the per-block two-allele test over the same reads),
`beta_cov` / `beta_stats` (the per-sample coverage and methylation summary read before choosing what goes into `segment`),
`compare_betas` (the 2-D histogram of every pair of those files: which samples agree), `beta2bed` (a file's sites as BED
text, formatted on the device), `beta_to_450k` (the files' values at the Illumina 450K / EPIC probes as one CSV table, gathered
and formatted on the device), `frag_len` (the histogram of a pat file's read lengths in CpGs: what `homog -l` is chosen from) and
`view` / `cview` (a pat file's reads as pat text: filtered by an interval, cut, sorted and collapsed on the device; both names run
view.main) and `merge` (the pat files or the beta files of replicates pooled into one: the reads of all files through the one view engine,
the beta rows summed and saturated by one kernel) and `mask_pat` (a pat file with the sites of a blocks table hidden from every read: the same
view engine with a bitmap of hidden sites inside its cut) and `mix_pat` (in-silico mixtures of pat files: the same view engine thins every
file's reads by a counter-based binomial draw, tags them with their source and orders tied lines as the reference's `sort -m` does) and
`bed2beta` (BED methylation calls of any pipeline joined to the CpG dictionary on the device, the first of duplicated lines kept: the door
into the `.beta` files everything above reads) and `bam2pat` (SAM text — what `samtools view` prints — called against the CpG dictionary, mates
merged and equal reads counted on the device, the same view engine behind it: the head of the pipeline, `.pat.gz` and `.beta` from alignments) and
`init_genome` / `set_default_ref` (the genome directory all of them start from: every CpG of a FASTA file found on the device, the dictionary's text
formatted and deflated there; which directory is the default); every
other reference subcommand is out of scope and says so."""
import sys

from .genome import IllegalArgumentError, eprint

VERSION = '0.2.0-mi355x'
COMMANDS = ['segment', 'convert', 'pat2beta', 'beta_to_blocks', 'beta_to_table', 'find_markers', 'homog', 'test_bimodal',
            'beta_cov', 'beta_stats', 'compare_betas', 'beta2bed', 'beta_to_450k', 'frag_len', 'view', 'cview', 'merge', 'mask_pat', 'mix_pat',
            'bed2beta', 'bam2pat', 'init_genome', 'set_default_ref']
MODULES = {'cview': 'view'}            # commands that run another command's module
# reference command list (wgbs_tools.py:11-48), for the "not in this build" message.  `view` is in both lists: COMMANDS is looked at first and
# carries its pat side; of a .beta / .lbeta input view.py itself says that it is not part of this build (and names `beta2bed`).  `merge` likewise:
# merge.py says what of it (--labels, -L, .bin) is not part of this build; `mix_pat`: mix_pat.py says it of -L; `bed2beta`: bed2beta.py says it of -d;
# `bam2pat`: bam2pat.py says it of .bam / .cram inputs, of coordinate-sorted paired-end input and of -r / -s / -L, --blacklist, --mbias, --blueprint, --nanopore, --long, -rg, -d;
# `init_genome`: init_genome.py says it of a missing --fasta_path (no download) and of -d
REFERENCE_ONLY = ['view', 'merge', 'index',
                  'beta2bw', 'bam2pat', 'mbias', 'init_genome', 'set_default_ref', 'vis', 'pat_fig',
                  'dmb', 'mix_pat', 'bed2beta',
                  'split_by_allele', 'split_by_meth', 'add_cpg_counts']


def print_help():
    msg = '\nUsage: wgbstools <command> [<args>]'
    msg += '\nrun wgbstools <command> -h for more information'
    msg += '\nOptional commands:\n'
    for key in COMMANDS:
        msg += '\t' + key + '\n'
    print(msg)
    return 1


def _take_inflate(args):
    """`--inflate {host,device}` taken out of a command's arguments -> (the other arguments, the choice or None).  For test_bimodal,
    whose module hands no such choice to the feed: main() below runs it inside pat2beta.default_inflate(choice)."""
    rest, choice, k = [], None, 0
    while k < len(args):
        a = args[k]
        if a == '--inflate':
            if k + 1 >= len(args):
                raise IllegalArgumentError('--inflate: expected host or device')
            choice, k = args[k + 1], k + 2
            continue
        if a.startswith('--inflate='):
            choice = a[len('--inflate='):]
        else:
            rest.append(a)
        k += 1
    if choice is not None and choice not in ('host', 'device'):
        raise IllegalArgumentError(f"--inflate: invalid choice {choice!r} (choose from 'host', 'device')")
    return rest, choice


def main(argv=None):
    argv = list(sys.argv if argv is None else argv)
    if len(argv) < 2 or argv[1] in ('-h', '--help'):
        return print_help()
    if argv[1] in ('--version', '-v'):
        print('wgbstools (MI355X segment) version', VERSION)
        return 0
    cmd = argv[1]
    if cmd in REFERENCE_ONLY and cmd not in COMMANDS:
        eprint(f'wgbstools {cmd}: not part of this build (it carries the MI355X-native `segment`, `convert`, `beta_to_blocks`, `beta_to_table`)')
        return 1
    if cmd not in COMMANDS:
        eprint('Invalid command:', f'\033[01;31m{cmd}\033[00m')
        return print_help()
    try:
        import importlib
        args, inflate = _take_inflate(argv[2:]) if cmd == 'test_bimodal' else (argv[2:], None)
        if inflate is not None:                # where the BGZF pat.gz is inflated: the other pat commands have the option themselves
            from .pat2beta import default_inflate
            with default_inflate(inflate):
                importlib.import_module('.' + MODULES.get(cmd, cmd), __package__).main(args)
            return 0
        importlib.import_module('.' + MODULES.get(cmd, cmd), __package__).main(args)
        return 0
    except IllegalArgumentError as e:          # wgbs_tools.py:77-79
        eprint(f'Invalid input argument\n{e}')
        return 1


if __name__ == '__main__':
    sys.exit(main())
