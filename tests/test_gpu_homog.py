"""`wgbstools homog` on the GPU (k_homog_count behind wgbsseg_homog_*): every golden case of the reference through the command
line, byte for byte after decompression; chunking; the exhaustive bin check; the refusals; the output options; a time-boxed
random comparison against the restatement tests/homog_ref.py."""
import gzip
import hashlib
import json
import os
import os.path as op
import time

import numpy as np
import pytest

import homog_cases as HC
import homog_ref as HR
from wgbs_tools_amd import _lib, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'homog_cases.json')) as f:
        return json.load(f)


def _write_case(d, case, bgzf=True):
    pat = op.join(d, 'smp.pat.gz')
    text = HC.case_pat(case['pat'])
    if bgzf:
        homog.write_bgzf(pat, text, 4)
    else:
        with gzip.open(pat, 'wb') as f:
            f.write(text)
    blocks = op.join(d, 'blocks.bed')
    with open(blocks, 'w') as f:
        f.write(HC.case_blocks(case['blocks'])[2])
    return pat, blocks, text


@pytest.mark.parametrize('name', sorted(HC.CASES))
def test_cli_matches_reference(name, golden, tmp_path):
    rec = golden[name]
    case = HC.CASES[name]
    pat, blocks, _ = _write_case(str(tmp_path), case, bgzf=name != 'nested')      # (one plain-gzip input as well)
    assert wgbs_tools.main(['wgbstools', 'homog', pat, '-b', blocks, '-o', str(tmp_path)] + case['args']) == 0
    if '--binary' in case['args']:
        got = open(str(tmp_path / 'smp.uxm'), 'rb').read()
        assert hashlib.sha1(got).hexdigest() == rec['bin_sha1'], name
    else:
        got = HR.read_output(str(tmp_path / 'smp.uxm.bed.gz'))
        assert got.decode().splitlines()[:len(rec['head'])] == rec['head'], name
        assert hashlib.sha1(got).hexdigest() == rec['text_sha1'], name


def _sorted_blocks(case):
    s, e, _ = HC.case_blocks(case['blocks'])
    o = np.lexsort((e, s))
    return s[o], e[o]


def test_ragged_chunks_match_one_feed():
    case = HC.CASES['long_reads_signed']
    s, e = _sorted_blocks(case)
    text = HC.case_pat(case['pat'])
    edges = homog.parse_range(homog.range_text(4))
    with _lib.Homog(s, e, edges, 4) as h:
        h.feed(text)
        one = h.finish()
    want = HR.count_sorted(text, s, e, edges, 4, False)
    assert np.array_equal(one.astype(np.int64), want)
    rng = np.random.default_rng(3)
    for _ in range(3):
        with _lib.Homog(s, e, edges, 4) as h:
            pos = 0
            while pos < len(text):
                cut = text.find(b'\n', min(len(text) - 1, pos + int(rng.integers(1, 20000)))) + 1
                h.feed(text[pos:cut])
                pos = cut
            assert h.kernel_ms() >= 0
            got = h.finish()
        assert np.array_equal(got, one)


def test_bins_exhaustive():
    """the device's bin for every (nrC, nrT) with nrC + nrT <= 4096 against numpy float32 division, l = 2..10"""
    M = 4096
    t = np.repeat(np.arange(M + 1), np.arange(1, M + 2)).astype(np.int64)
    c = np.concatenate([np.arange(k + 1) for k in range(M + 1)]).astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        meth = c.astype(np.float32) / t.astype(np.float32)
    for rlen in range(2, 11):
        text = homog.range_text(rlen, '0.25,0.75' if rlen == 2 else None)
        edges = homog.parse_range(text)
        got = _lib.debug_homog_bins(edges, M)
        nb = edges.size - 1
        want = np.full(meth.size, nb - 1, dtype=np.int8)
        for b in range(nb - 1, -1, -1):
            want[(meth >= edges[b]) & (meth < edges[b + 1])] = b
        assert np.array_equal(got, want), rlen


def test_refusals(tmp_path):
    s, e = np.array([1, 10], dtype=np.int64), np.array([5, 20], dtype=np.int64)
    edges = homog.parse_range(homog.range_text(3))
    good = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\n'
    for bad in (b'chr1\t5\tCT\n', b'chr1\tx\tCT\t3\n', b'chr1\t5\tCT\t\n'):
        with _lib.Homog(s, e, edges, 3) as h:
            h.feed(good)
            h.feed(bad)
            with pytest.raises(_lib.SegmentorError, match='byte offset %d' % len(good)):
                h.finish()
    # a descending read: inside a chunk, across tiles and across chunks
    with _lib.Homog(s, e, edges, 3) as h:
        h.feed(good + b'chr1\t2\tCCC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='not sorted.*byte offset %d' % len(good)):
            h.finish()
    filler = b''.join(b'chr1\t%d\tCCCT\t1\n' % (3 + i // 1000) for i in range(3000))
    with _lib.Homog(s, e, edges, 3) as h:
        h.feed(good + filler + b'chr1\t4\tCCC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='byte offset %d' % (len(good) + len(filler))):
            h.finish()
    with _lib.Homog(s, e, edges, 3) as h:
        h.feed(good)
        h.feed(b'\n\n')
        h.feed(b'chr1\t2\tCCC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='byte offset %d' % (len(good) + 2)):
            h.finish()
    with pytest.raises(_lib.SegmentorError, match='startCpG 0 < 1'):
        _lib.Homog(np.array([0]), np.array([3]), edges, 3)
    # through the command line: the messages name the offset / the row
    pat = str(tmp_path / 'u.pat.gz')
    with gzip.open(pat, 'wb') as f:
        f.write(good + b'chr1\t2\tCCC\t1\n')
    blocks = tmp_path / 'b.bed'
    blocks.write_text('chr1\t10\t20\t1\t5\nchr1\t30\t40\t10\t20\n')
    with pytest.raises(Exception, match='not sorted'):
        homog.main([pat, '-b', str(blocks), '-o', str(tmp_path)])
    blocks.write_text('chr1\t10\t20\t1\t5\nchr1\t30\t40\t0\t20\n')
    with pytest.raises(Exception, match='row 2 has startCpG 0'):
        homog.main([pat, '-b', str(blocks), '-o', str(tmp_path)])


def test_output_options_and_several_files(tmp_path, capsys):
    case = HC.CASES['header_comments']
    d = str(tmp_path)
    pat, blocks, text = _write_case(d, case)
    pat2 = op.join(d, 'another.pat.gz')
    homog.write_bgzf(pat2, text[:text.rfind(b'\n', 0, len(text) // 2) + 1], 2)
    zero = op.join(d, 'zero.pat.gz')
    with gzip.open(zero, 'wb') as f:
        f.write(b'chr1\t1\tCC\t5\n')
    out = op.join(d, 'out', 'sub')
    assert wgbs_tools.main(['wgbstools', 'homog', pat2, pat, zero, '-b', blocks, '-o', out]) == 0
    err = capsys.readouterr().err
    assert '[ wt homog ]  [ zero ] WARNING: all zeros!' in err
    for n in ('smp', 'another', 'zero'):
        assert op.isfile(op.join(out, n + '.uxm.bed.gz'))
    first = HR.read_output(op.join(out, 'smp.uxm.bed.gz'))
    # skip without -f, overwrite with it
    t0 = op.getmtime(op.join(out, 'smp.uxm.bed.gz'))
    assert wgbs_tools.main(['wgbstools', 'homog', pat, '-b', blocks, '-o', out]) == 0
    assert 'skipping smp. Use -f to overwrite' in capsys.readouterr().err
    assert op.getmtime(op.join(out, 'smp.uxm.bed.gz')) == t0
    assert wgbs_tools.main(['wgbstools', 'homog', pat, '-b', blocks, '-o', out, '-f']) == 0
    assert HR.read_output(op.join(out, 'smp.uxm.bed.gz')) == first
    # -p: the prefix names the output, its directory is created
    pre = op.join(d, 'p', 'q', 'mine')
    assert wgbs_tools.main(['wgbstools', 'homog', pat, '-b', blocks, '-p', pre, '--binary']) == 0
    assert op.isfile(pre + '.uxm')
    import pandas as pd
    df = pd.read_csv(op.join(out, 'smp.uxm.bed.gz'), sep='\t', header=None)
    assert df.shape[1] == 8


def test_random_against_restatement():
    """random blocks (nested, unsorted, duplicated) and reads against homog_ref, for at most ~20 s"""
    seed0 = int.from_bytes(os.urandom(4), 'little')
    print('homog random comparison: seeds from', seed0)
    t_end = time.time() + 18
    k = 0
    while time.time() < t_end and k < 200:
        rng = np.random.default_rng(seed0 + k)
        n_sites = int(rng.integers(50, 3000))
        nb = int(rng.integers(1, 400))
        s = rng.integers(1, n_sites, nb)
        e = s + rng.integers(1, rng.choice([5, 40, 2 * n_sites]), nb)
        o = np.lexsort((e, s))
        s, e = s[o], e[o]
        nr = int(rng.integers(1, 3000))
        st = np.sort(rng.integers(-5, n_sites + 5, nr))
        ln = rng.integers(0, rng.choice([8, 40, 300]), nr)
        alphabet = np.array(list('CTH.'))
        lines = ['chr1\t%d\t%s\t%d\n' % (st[i], ''.join(rng.choice(alphabet, ln[i])), rng.integers(-50, 100)) for i in range(nr)]
        text = ''.join(lines).encode()
        rlen = int(rng.integers(2, 7))
        th = '0.3,0.6' if rlen == 2 else None
        edges = homog.parse_range(homog.range_text(rlen, th))
        incl = bool(rng.integers(0, 2))
        with _lib.Homog(s, e, edges, rlen, incl) as h:
            h.feed(text)
            got = h.finish()
        want = HR.count_sorted(text, s, e, edges, rlen, incl)
        assert np.array_equal(got.astype(np.int64), want), ('seed', seed0 + k)
        k += 1
    assert k > 0
