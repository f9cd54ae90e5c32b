"""Seeded inputs of the `wgbstools mix_pat` cases (tests/golden/make_golden_mix.py records in tests/golden/mix_cases.json what the
reference's cview, sort, collapse script and sed print for them once tests/mix_ref.py has drawn the counts; tests/test_mix_pat_cpu.py
and tests/test_gpu_mix_pat.py rebuild the inputs).  Pat texts over the tiny genome of frag_cases.genome_dir, as in merge_cases.py: every
read lies inside the chromosome it names and every count is at least 1.  Whole-genome cases come without --strip (mix_pat.py's
deviation 4)."""
import merge_cases as MC
import mix_ref as MX

genome_dir = MC.genome_dir
region_text = MC.region_text
N_SITES = MC.N_SITES


def tie_files():
    """three files whose lines tie in start, pattern and chromosome at 80 starts; the counts put the drawn sums (p = 0.25) around 9 - 10,
    2 and 19: texts that order unlike their values (TIE_SEED is chosen so that a 9 meets a 10 and a 2 meets a 19: test_mix_pat_cpu.py
    checks it).  Every seventh line of the third file names chr2 — a name only, in a view over sites: it keeps the chromosome in the key."""
    a = b''.join(b'chr1\t%d\tCT\t%d\n' % (pos, 38 if pos <= 40 else 8) for pos in range(1, 81))
    b = b''.join(b'chr1\t%d\tCT\t%d\n' % (pos, 40 if pos <= 40 else 6 + pos % 5) for pos in range(1, 81))
    c = b''.join(b'chr%d\t%d\tCT\t%d\n' % (1 + (pos % 7 == 0), pos, 76) for pos in range(1, 81))
    return [a, b, c]


_DOTS = b'CCTTH...'
TIE_SEED = 1
QUARTER = 0.25
# name -> files: the pat texts (callables); labels (argument order); adj: the adjusted rate of every file (mix_ref.sampler_args turns it
# into T and reps); seed, rep; where / flags as in merge_cases.py
CASES = {
    'tie_three': dict(files=tie_files, labels=['b', 'ab', 'a'], adj=[QUARTER, QUARTER, QUARTER], seed=TIE_SEED, rep=0, where=['-s', '1-200'], flags=[]),
    'tie_three_rep1': dict(files=tie_files, labels=['b', 'ab', 'a'], adj=[QUARTER, QUARTER, QUARTER], seed=TIE_SEED, rep=1, where=['-s', '1-200'], flags=[]),
    'sites_strict_strip_min3': dict(files=lambda: [MC.reads_text(63 + k, 400, 1150, 1260, max_len=9, alphabet=_DOTS) for k in range(3)],
                                    labels=['liver', 'blood', 'liver2'], adj=[0.6, 1.7, 0.1], seed=2 ** 63 + 11, rep=0,
                                    where=['-s', '1200-1230'], flags=['--strict', '--strip', '--min_len', '3']),
    'region_two': dict(files=lambda: [MC.reads_text(66, 400, 2750, 2960, max_len=5), MC.reads_text(67, 350, 2750, 2960, max_len=5)],
                       labels=['x.1', 'x'], adj=[0.31, 0.07], seed=123456789, rep=3, where=['-r', region_text], flags=['--strict']),
    'wg_two': dict(files=lambda: [MC.reads_text(68, 300, 1, N_SITES), MC.reads_text(69, 320, 1, N_SITES)],
                   labels=['T-cells', 'B_cells'], adj=[0.5, 0.2], seed=99, rep=0, where=[], flags=[]),
}


def case_files(case):
    return case['files']()


def case_where(case):
    return [w() if callable(w) else w for w in case['where']]


def per_file(case):
    """(T, reps) of every file"""
    return [MX.sampler_args(a)[:2] for a in case['adj']]


flag_kwargs = MC.flag_kwargs


def expected(case, s, e, stats=None):
    """mix_ref's output for the case over [s, e)"""
    return MX.mix(case_files(case), [x.encode() for x in case['labels']], per_file(case), case['seed'], case['rep'], s, e, stats=stats,
                  **flag_kwargs(case['flags']))
