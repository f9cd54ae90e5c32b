"""`wgbstools mix_pat` on the GPU.  The view engine with labels and sources (wgbsseg_patview_set_labels / _set_source): the draws of
k_view_measure_sampled / k_view_pack_sampled, the label as the last sort key, k_view_tie_order and the labelled emit — byte for byte
against tests/mix_ref.py and, where they exist, the goldens of the reference's sort and collapse script; the same bytes however the text
is cut into calls and wherever it is inflated; the corners of T, reps and the 2^20 cap; the state rules of the new calls; an engine
without them against a `merge` golden; one statistical case; the command end to end."""
import gzip
import json
import os.path as op

import numpy as np
import pytest

import merge_cases as MC
import mix_cases as XC
import mix_ref as MX
from wgbs_tools_amd import _lib, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
QUARTER = 2 ** 30


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'mix_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return XC.genome_dir(str(tmp_path_factory.mktemp('mix_genome')))[0]


def bgzf_bytes(text, member):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def line_pieces(text, n_lines):
    """the text in pieces of n_lines whole lines"""
    lines = text.splitlines(keepends=True)
    return [b''.join(lines[k:k + n_lines]) for k in range(0, len(lines), n_lines)]


def run_mix(files, labels, per_file, seed, rep, s, e, how='text', initial_records=0, deflate=False, info=None, **flags):
    """the device's output: every file fed to ONE engine with its source.  how: 'text' (one feed per file), ('lines', n) (feeds of n lines),
    ('bgzf', member, piece) (BGZF members of `member` bytes of text, handed over in pieces of `piece` bytes that end anywhere)"""
    with _lib.PatView(s, e, sort=True, initial_records=initial_records, **flags) as v:
        ranks = v.set_labels(labels)
        assert sorted(ranks) == list(range(len(labels))) and [labels[i] for i in np.argsort(ranks)] == sorted(labels)
        for k, text in enumerate(files):
            if k:
                v.next_file()
            v.set_source(ranks[k], per_file[k][0], per_file[k][1], seed, MX.stream_of(rep, k))
            if how == 'text':
                v.feed(text if text.endswith(b'\n') or not text else text + b'\n')
            elif how[0] == 'lines':
                for piece in line_pieces(text, how[1]):
                    v.feed(piece)
            else:
                data, buf = bgzf_bytes(text, how[1]), b''
                for p in range(0, len(data), how[2]):
                    buf += data[p:p + how[2]]
                    buf = buf[v.feed_bgzf(buf):]
                assert not buf
        lines, nbytes = v.finish(deflate=deflate)
        out = v.read()
        assert len(out) == nbytes and (deflate or out.count(b'\n') == lines)
        if info is not None:
            info.update(v.info(), lines=lines, **v.sample_info())
        return out


def run_case(name, golden=None, **kw):
    case = XC.CASES[name]
    s, e = golden[name]['sites']
    return run_mix(XC.case_files(case), [x.encode() for x in case['labels']], XC.per_file(case), case['seed'], case['rep'], s, e,
                   **dict(XC.flag_kwargs(case['flags']), **kw))


# ---- against the goldens and the restatement ----
@pytest.mark.parametrize('name', sorted(XC.CASES))
def test_goldens_through_the_engine(name, golden):
    """ties in start, pattern and chromosome over three files; sums whose texts order unlike their values; a label that is a prefix of
    another and labels whose byte order is not the argument order (tie_three); reps 4 and 8; the cut flags; the whole genome"""
    want = golden[name]['stdout'].encode()
    stats, info = {}, {}
    assert XC.expected(XC.CASES[name], *golden[name]['sites'], stats=stats) == want
    assert run_case(name, golden, info=info) == want
    assert (info['sampled_reads'], info['sampled_dropped'], info['sampled_kept']) == (stats['reached'], stats['dropped'], stats['kept'])
    assert info['records'] == stats['reached'] - stats['dropped']
    assert run_case(name, golden, how=('bgzf', 300, 1000), initial_records=4) == want


def test_repetitions_differ_and_each_repeats(golden):
    a, b = run_case('tie_three', golden), run_case('tie_three_rep1', golden)
    assert a != b and a == run_case('tie_three', golden) and b == run_case('tie_three_rep1', golden)
    packed = run_case('tie_three', golden, deflate=True)
    assert packed.endswith(BGZF_EOF) and gzip.decompress(packed) == a


# ---- the same bytes however the text arrives ----
def short_lines(n, count=1, first=1):
    """n lines of 8 to 11 bytes: a 4 KB tile holds more lines than a workgroup has threads"""
    return b''.join(b'c\t%d\tC\t%d\n' % (first + i // 3, count) for i in range(n))


def test_chunking_and_inflate_do_not_show():
    files = [short_lines(3000, count=2), short_lines(2500, count=1, first=400)]
    assert files[0][:4096].count(b'\n') > 256                          # one tile, several rounds of WG_BLOCK lines
    labels, per_file = [b'ab', b'a'], [(QUARTER, 1), (3 * 2 ** 28, 2)]
    stats, info = {}, {}
    want = MX.mix(files, labels, per_file, 5, 2, 1, 5000, stats=stats)
    assert want.count(b"\n") > 1000 and want.count(b'\tab\n') and want.count(b'\ta\n')
    assert run_mix(files, labels, per_file, 5, 2, 1, 5000, info=info) == want
    assert (info['sampled_reads'], info['sampled_dropped'], info['sampled_kept']) == (stats['reached'], stats['dropped'], stats['kept'])
    grown = {}
    assert run_mix(files, labels, per_file, 5, 2, 1, 5000, how=('lines', 301), initial_records=4, info=grown) == want      # pieces that end inside a tile's round
    assert grown['grown_records'] >= 2 and grown['grown_arena'] >= 2
    assert run_mix(files, labels, per_file, 5, 2, 1, 5000, how=('lines', 257)) == want
    assert run_mix(files, labels, per_file, 5, 2, 1, 5000, how=('bgzf', 333, 4000)) == want        # members and pieces cut lines in the middle
    assert run_mix(files, labels, per_file, 5, 2, 1, 5000, how=('bgzf', 60000, 1 << 20)) == want
    assert run_mix([f[:-1] for f in files], labels, per_file, 5, 2, 1, 5000, how=('bgzf', 500, 777)) == want       # the last line without its newline
    assert run_mix(files, labels, per_file, 6, 2, 1, 5000) != want and run_mix(files, labels, per_file, 5, 3, 1, 5000) != want


# ---- the corners of the draw ----
def test_threshold_corners():
    files = [short_lines(700, count=3), short_lines(10, count=1000, first=9000)]
    labels = [b'x', b'y']
    out = run_mix(files, labels, [(0, 1), (0, 8)], 1, 0, 1, 10000, deflate=True)
    assert out == BGZF_EOF                                            # T = 0: nothing is kept; a valid, empty BGZF file
    assert run_mix(files, labels, [(0, 1), (0, 8)], 1, 0, 1, 10000) == b''
    for per_file in ([(QUARTER, 4), (QUARTER, 8)], [(1, 4), (2 ** 29 + 12345, 8)]):       # p = 0.25 with reps 4; count 1000 with reps 8
        stats, info = {}, {}
        want = MX.mix(files, labels, per_file, 77, 1, 1, 10000, stats=stats)
        assert run_mix(files, labels, per_file, 77, 1, 1, 10000, info=info) == want
        assert info['sampled_kept'] == stats['kept']
    assert stats['by_label'][b'y'] > 5 * 1000                          # 8,000 draws a line at about 0.125: about 10,000 in all


def test_the_cap_on_count_times_reps():
    at = b'chr1\t5\tCT\t3\nchr1\t9\tC\t%d\n' % 2 ** 18                   # 2^18 * 4 = 2^20: allowed
    labels, per_file = [b'a', b'b'], [(2 ** 22, 4), (QUARTER, 1)]
    good = b'chr1\t5\tCT\t3\nchr1\t9\tC\t1\n'
    assert run_mix([at, good], labels, per_file, 3, 0, 1, 100) == MX.mix([at, good], labels, per_file, 3, 0, 1, 100) != b''
    over = b'chr1\t5\tCT\t3\nchr1\t9\tC\t%d\n' % (2 ** 18 + 1)
    for files, msg in (([over, good], 'failed in view: file 0: count * reps above 2^20 at byte 12'),
                       ([good, over], None)):
        if msg is None:                                               # reps = 1 for the second file: far below the cap
            assert run_mix(files, labels, per_file, 3, 0, 1, 100) == MX.mix(files, labels, per_file, 3, 0, 1, 100)
            continue
        for how in ('text', ('bgzf', 7, 50)):
            with pytest.raises(_lib.SegmentorError) as err:
                run_mix(files, labels, per_file, 3, 0, 1, 100, how=how)
            assert err.value.code == _lib.E_ARG and err.value.msg == msg
        with pytest.raises(MX.Refused):
            MX.mix(files, labels, per_file, 3, 0, 1, 100)
    assert run_mix([over, good], labels, per_file, 3, 0, 1, 9) == MX.mix([over, good], labels, per_file, 3, 0, 1, 9)     # the cut drops the line: never drawn
    with pytest.raises(_lib.SegmentorError) as err:                  # one file: no file in the message
        run_mix([over], [b'a'], per_file[:1], 3, 0, 1, 100)
    assert err.value.msg == 'failed in view: count * reps above 2^20 at byte 12'
    with pytest.raises(_lib.SegmentorError) as err:                  # a count below 1 is refused as merge refuses it, in one file too
        run_mix([b'chr1\t5\tCT\t0\n'], [b'a'], per_file[:1], 3, 0, 1, 100)
    assert err.value.msg == 'failed in view: count < 1 at byte 0'
    with pytest.raises(_lib.SegmentorError) as err:
        run_mix([good, good + b'chr1\t12\tC\t-2\n'], labels, per_file, 3, 0, 1, 100)
    assert err.value.msg == 'failed in view: file 1: count < 1 at byte %d' % len(good)


# ---- the state rules ----
def test_state_and_argument_rules():
    good = b'chr1\t5\tCT\t3\n'
    with _lib.PatView(1, 100, sort=True) as v:
        ranks = v.set_labels(['b', 'a'])
        assert ranks == [1, 0]
        with pytest.raises(_lib.SegmentorError, match='called twice') as err:
            v.set_labels(['c'])
        assert err.value.code == _lib.E_STATE
        with pytest.raises(_lib.SegmentorError, match='has no source') as err:       # with labels every file needs a source
            v.feed(good)
        assert err.value.code == _lib.E_STATE
        for args, what in (((2, 0, 1, 0, 0), 'label rank 2 of 2'), ((0, QUARTER + 1, 1, 0, 0), 'at most 2\\^30'), ((0, 0, 0, 0, 0), 'reps = 0')):
            with pytest.raises(_lib.SegmentorError, match=what) as err:
                v.set_source(*args)
            assert err.value.code == _lib.E_ARG
        with pytest.raises(_lib.SegmentorError, match='mask and sources') as err:
            v.set_mask([5], [9])
        v.set_source(1, QUARTER, 4, 9, 0)
        v.set_source(0, QUARTER, 4, 9, 0)                              # before the first feed it may still change
        v.feed(good)
        with pytest.raises(_lib.SegmentorError, match='has been fed already') as err:
            v.set_source(1, QUARTER, 4, 9, 0)
        assert err.value.code == _lib.E_STATE
        v.next_file()
        with pytest.raises(_lib.SegmentorError, match='file 1 has no source'):
            v.feed(good)
        v.set_source(1, QUARTER, 4, 9, 1)
        v.feed(good)
        v.finish()
        assert set(v.read().split(b'\n')[:-1]) <= {b'chr1\t5\tCT\t%d\t%s' % (n, lab) for n in range(1, 13) for lab in (b'a', b'b')}
        with pytest.raises(_lib.SegmentorError) as err:
            v.set_source(1, QUARTER, 4, 9, 1)
        assert err.value.code == _lib.E_STATE
    with _lib.PatView(1, 100, sort=True) as v:
        v.feed(good)
        with pytest.raises(_lib.SegmentorError, match='after the first feed') as err:
            v.set_labels(['a'])
        assert err.value.code == _lib.E_STATE
    with _lib.PatView(1, 100, sort=True) as v:                         # no labels: no rank is valid
        with pytest.raises(_lib.SegmentorError, match='label rank 0 of 0') as err:
            v.set_source(0, QUARTER, 1, 9, 0)
        assert err.value.code == _lib.E_ARG
    with _lib.PatView(1, 100, sort=True, mask=([5], [9])) as v:        # a mask together with a source is refused
        with pytest.raises(_lib.SegmentorError, match='mask and sources'):
            v.set_labels(['a'])
        with pytest.raises(_lib.SegmentorError, match='mask and sources'):
            v.set_source(0, QUARTER, 1, 9, 0)
    with _lib.PatView(1, 100, sort=False) as v:
        with pytest.raises(_lib.SegmentorError, match='sorted view') as err:
            v.set_labels(['a'])
        assert err.value.code == _lib.E_ARG
    for bad, what in ((['a', 'a'], 'given twice'), (['a/b'], '0x2f'), ([''], 'is empty'), (['a b'], '0x20'), ([], '0 labels'), (['l%d' % k for k in range(256)], '256 labels')):
        with _lib.PatView(1, 100, sort=True) as v:
            with pytest.raises(_lib.SegmentorError, match=what) as err:
                v.set_labels(bad)
            assert err.value.code == _lib.E_ARG
    with _lib.PatView(1, 100, sort=True) as v:
        assert sorted(v.set_labels(['l%d' % k for k in range(255)])) == list(range(255))


def test_an_engine_without_the_new_calls_is_merge():
    with open(op.join(ROOT, 'tests', 'golden', 'merge_cases.json')) as f:
        rec = json.load(f)['sites_strict_strip_min3']
    files = MC.case_files(MC.PAT_CASES['sites_strict_strip_min3'])
    with _lib.PatView(*rec['sites'], sort=True, **MC.flag_kwargs(rec['flags'])) as v:
        for k, text in enumerate(files):
            if k:
                v.next_file()
            v.feed(text)
        v.finish()
        assert v.read() == rec['stdout'].encode()
        assert v.sample_info() == dict(sampled_reads=0, sampled_dropped=0, sampled_kept=0)


# ---- the law ----
STAT_SEED = 20261021


def test_the_binomial_law_on_twenty_thousand_lines():
    """20,000 lines of count 1, p = 0.2: the kept total lies within 6 standard deviations of n p = 4,000 (sigma = sqrt(n p (1 - p)) = 56.6).  The
    seed is fixed; the bound is the law's, not the kernel's: it guards against the kernel and the restatement sharing one wrong comparison."""
    n, (T, reps, p) = 20000, MX.sampler_args(0.2)
    assert reps == 1 and abs(p - 0.2) < 1e-7
    text = b''.join(b'chr1\t%d\tC\t1\n' % (1 + i) for i in range(n))
    lo, hi = n * p - 6 * np.sqrt(n * p * (1 - p)), n * p + 6 * np.sqrt(n * p * (1 - p))
    stats, info = {}, {}
    want = MX.mix([text], [b'only'], [(T, reps)], STAT_SEED, 0, 1, n + 1, stats=stats)
    assert lo <= stats['kept'] <= hi                                   # the restatement alone, on the CPU
    got = run_mix([text], [b'only'], [(T, reps)], STAT_SEED, 0, 1, n + 1, info=info)
    kept = sum(int(ln.split(b'\t')[3]) for ln in got.splitlines())
    print('kept', kept, 'of', n, 'bounds', lo, hi)
    assert lo <= kept <= hi and kept == info['sampled_kept'] == got.count(b'\n')
    assert got == want


# ---- the command end to end ----
def test_cli_end_to_end(genome, tmp_path, capfd):
    files = [MC.reads_text(81, 900, 1, XC.N_SITES, max_len=6), MC.reads_text(82, 500, 1, XC.N_SITES, max_len=6)]
    a, b = str(tmp_path / 'liver.pat.gz'), str(tmp_path / 'blood.pat.gz')
    homog.write_bgzf(a, files[0], 1)
    homog.write_bgzf(b, files[1], 1)
    pre = str(tmp_path / 'mix')
    argv = ['wgbstools', 'mix_pat', a, b, '--rates', '.3', '-p', pre, '--reps', '2', '--seed', '7', '--genome', genome, '-v']
    assert wgbs_tools.main(argv) == 0
    err = capfd.readouterr().err
    assert 'Generating it' in err and 'ReqstRates' in err and 'no .csi index is written' in err and '--seed' not in err
    covs = []
    for p in (a, b):                                                  # the missing .beta files have appeared next to the pat files
        rows = np.fromfile(p[:-7] + '.beta', dtype=np.uint8).reshape(-1, 2)
        assert rows.shape[0] == XC.N_SITES
        covs.append(float(rows[:, 1].astype(np.int64).sum()) / XC.N_SITES)
    cov, adj = MX.adjusted(MX.rates_of([0.3], 2), covs)
    assert cov == covs[1]
    per_file = [MX.sampler_args(x)[:2] for x in adj]
    outs = []
    for rep in range(2):
        stats = {}
        want = MX.mix(files, [b'liver', b'blood'], per_file, 7, rep, 1, XC.N_SITES + 1, stats=stats)
        with open('%s_%d.pat.gz' % (pre, rep + 1), 'rb') as f:
            data = f.read()
        assert data.endswith(BGZF_EOF) and gzip.decompress(data) == want
        by_label = {}
        for ln in want.splitlines():
            f5 = ln.split(b'\t')
            assert len(f5) == 5
            by_label[f5[4]] = by_label.get(f5[4], 0) + int(f5[3])
        assert by_label == stats['by_label'] and sum(by_label.values()) == stats['kept']
        assert ('%d reads drawn, %d dropped, counts kept %d ' % (stats['reached'], stats['dropped'], stats['kept'])) in err
        starts = [int(ln.split(b'\t')[1]) for ln in want.splitlines()]
        assert starts == sorted(starts)
        outs.append(data)
    assert outs[0] != outs[1]
    assert wgbs_tools.main(argv) == 0 and capfd.readouterr().err.count('already exists. Skipping it.') == 2
    assert wgbs_tools.main(argv + ['-f', '--inflate', 'device']) == 0
    capfd.readouterr()
    for rep in range(2):
        with open('%s_%d.pat.gz' % (pre, rep + 1), 'rb') as f:
            assert f.read() == outs[rep]                              # the same bytes on every run with that seed
    assert wgbs_tools.main(['wgbstools', 'mix_pat', a, b, '--rates', '.5', '.5', '-o', str(tmp_path), '--genome', genome, '-s', '100-900', '--strict']) == 0
    err = capfd.readouterr().err
    seed = int(err.split('[wt mix] --seed ')[1].split()[0])             # no --seed: drawn, and printed so that the run can be repeated
    name = [ln for ln in err.splitlines() if ln.startswith('[wt mix] mix: ')][0][len('[wt mix] mix: '):]
    assert op.basename(name).startswith('liver_0.5_blood_0.5_cov_') and name.endswith('_1.pat.gz') and op.isfile(name)
    covs = [float(np.fromfile(p[:-7] + '.beta', dtype=np.uint8).reshape(-1, 2)[99:899, 1].astype(np.int64).sum()) / 800 for p in (a, b)]
    cov, adj = MX.adjusted([0.5, 0.5], covs)
    with open(name, 'rb') as f:
        assert gzip.decompress(f.read()) == MX.mix(files, [b'liver', b'blood'], [MX.sampler_args(x)[:2] for x in adj], seed, 0, 100, 900, strict=True)
