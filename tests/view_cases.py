"""Seeded inputs of the `wgbstools view` cases (tests/golden/make_golden_view.py records what the reference's cview, sort and
collapse script print for them in tests/golden/view_cases.json; tests/test_view_cpu.py and tests/test_gpu_view.py rebuild the
inputs): pat texts from homog_cases.pat_text or written out line by line, over the tiny genome of frag_cases.genome_dir; and the
random worlds of the comparison with tests/view_ref.py."""
import numpy as np

import frag_cases as FC
import homog_cases as HC

N_SITES = FC.N_SITES
region_text = FC.region_text
genome_dir = FC.genome_dir

_WG = dict(seed=51, n_sites=N_SITES, n_reads=260, n_chroms=2, max_len=9)
_DENSE = dict(seed=52, n_sites=N_SITES, n_reads=9000, n_chroms=2, max_len=10, max_count=9)
_DENSE_LONG = dict(seed=53, n_sites=N_SITES, n_reads=5000, n_chroms=2, max_len=8, long_every=250, long_len=1500)


def signed_lines(seed=54, n_sites=200, n_reads=1500):
    """short reads over few sites with counts -3 .. 3, written without a plus sign (a count the file spells "+3" comes out of the
    reference's collapse script as "+3" when its run has one line and as 3 when it has more; this build prints 3): many equal
    lines, many runs whose sum is <= 0"""
    start = np.sort((HC._rand(seed, 1, n_reads) % HC.U(n_sites)).astype(np.int64) + 1)
    h = HC._rand(seed, 2, n_reads)
    ln = 1 + (h % HC.U(3)).astype(np.int64)
    cnt = ((h >> HC.U(8)) % HC.U(7)).astype(np.int64) - 3
    chars = np.frombuffer(b'CCCTTTH.', dtype=np.uint8)[(HC._rand(seed, 3, int(ln.sum())) & HC.U(7)).astype(np.int64)].tobytes().decode()
    off = np.concatenate([[0], np.cumsum(ln)]).tolist()
    return ''.join('chr1\t%d\t%s\t%d\n' % (start[i], chars[off[i]:off[i + 1]], cnt[i]) for i in range(n_reads)).encode()


_SETTINGS = {'plain': [], 'strict': ['--strict'], 'strict_strip': ['--strict', '--strip'],
             'strict_strip_min3': ['--strict', '--strip', '--min_len', '3'], 'no_gaps': ['--no_gaps'], 'no_sort': ['--no_sort']}

# name -> pat: generator parameters of homog_cases.pat_text, or lines: the text itself or what makes it; where: [] | ['-s', text] | ['-r', text];
# flags: the reference's view flags
CASES = {
    'wg_plain': dict(pat=_WG, where=[], flags=[]),
    'wg_strip': dict(pat=_WG, where=[], flags=['--strip']),
    'empty_region': dict(lines=b'chr1\t5\tCCT\t2\nchr1\t900\tTTTT\t1\n', where=['-s', '100-200'], flags=[]),
    'signed_strict': dict(lines=signed_lines, where=['-s', '20-60'], flags=['--strict']),
    'long_reach_strict': dict(pat=_DENSE_LONG, where=['-s', '2000-2012'], flags=['--strict', '--strip']),
}
for _name, _flags in _SETTINGS.items():
    CASES['sites_' + _name] = dict(pat=_DENSE, where=['-s', '1200-1230'], flags=_flags)
    CASES['region_' + _name] = dict(pat=_DENSE, where=['-r', region_text], flags=_flags)


def case_pat(case):
    if 'pat' in case:
        return HC.pat_text(**case['pat'])
    return case['lines']() if callable(case['lines']) else case['lines']


def case_where(case):
    return [w() if callable(w) else w for w in case['where']]


def flag_kwargs(flags):
    """the reference's flags -> the keywords of view_ref.view / view.view_pat (without sort)"""
    kw = dict(strict='--strict' in flags, strip='--strip' in flags, no_gaps='--no_gaps' in flags, min_len=1)
    if '--min_len' in flags:
        kw['min_len'] = int(flags[flags.index('--min_len') + 1])
    return kw


def random_pattern(rng, n, dots=0.25):
    return ''.join(rng.choice(list('CTH.'), n, p=[(1 - dots) / 3] * 3 + [dots]))


def random_world(rng):
    """-> (pat text, s, e, flags dict with sort): reads sorted by start, some long, dots, signed counts, repeats, empty lines"""
    n_sites = int(rng.integers(30, 1200))
    nr = int(rng.integers(1, 2500))
    st = np.sort(rng.integers(-3, n_sites + 5, nr))
    ln = rng.integers(1, int(rng.choice([3, 6, 30])), nr)
    if rng.random() < 0.3:
        ln[rng.integers(0, nr)] = int(rng.integers(1100, 1700))
    cnt = rng.integers(-3, int(rng.choice([5, 50, 2 ** 31])), nr)
    dots = float(rng.choice([0.0, 0.2, 0.6]))
    lines = ['chr%d\t%d\t%s\t%d\n' % (1 + (st[i] > n_sites // 2), st[i], random_pattern(rng, ln[i], dots), cnt[i]) for i in range(nr)]
    for _ in range(int(rng.integers(0, 4))):
        lines.insert(int(rng.integers(0, len(lines) + 1)), '\n')
    text = ''.join(lines)
    if rng.random() < 0.3:
        text = text.rstrip('\n')                                    # a last line without its newline: BGZF feeds only
    if rng.random() < 0.25:
        s, e = 1, n_sites + 1
    else:
        s = int(rng.integers(1, n_sites))
        e = s + int(rng.integers(1, int(rng.choice([4, 60, n_sites]))))
    flags = dict(strict=bool(rng.random() < 0.5), strip=bool(rng.random() < 0.5), no_gaps=bool(rng.random() < 0.3),
                 min_len=int(rng.choice([1, 1, 2, 3, 7])), sort=bool(rng.random() < 0.6))
    return text.encode(), s, e, flags
