"""`wgbstools beta2bed` on the GPU (k_bed_len, k_bed_scan, k_bed_emit behind wgbsseg_beta2bed): every case of
tests/bed_cases.py through the command line against what the reference printed (tests/golden/bed_cases.json), byte for byte
or by sha1 and counts; the small world again through the ABI in slabs of 64, 256 and 1000 sites and the default; the
direct-to-global path, forced through the plan's stage_bytes and reached by high multiplicities; slabs without text inside the
two-slab pipeline; bit-identical repeats; the refusals that need a device context; a failed write with slabs in flight and the
next call on the same context."""
import errno
import gzip
import hashlib
import json
import os
import os.path as op

import numpy as np
import pytest

import bed_cases as BC
import bed_ref as BR
from wgbs_tools_amd import _lib, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
CASES = BC.cases()


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'bed_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def worlds():
    return BC.worlds()


@pytest.fixture(scope='module')
def where(tmp_path_factory, worlds):
    td = str(tmp_path_factory.mktemp('bed'))
    return {name: BC.write_world(td, name, w) for name, w in worlds.items()}


@pytest.fixture(scope='module')
def seg():
    with _lib.Segmenter(0) as s:
        yield s


def _load(seg, w, file_name):
    rows = w['files'][file_name]
    (seg.set_lbetas if rows.dtype == np.uint16 else seg.set_betas)([rows])
    seg.set_loci(w['loci'])
    return rows


def _emit(seg, w, tmp_path, **kw):
    """Segmenter.beta2bed into a file -> (its bytes, lines, bytes reported)"""
    path = str(tmp_path / 'out.bed')
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        lines, nbytes = seg.beta2bed(fd, 0, w['names'], np.cumsum(w['sizes']), **kw)
    finally:
        os.close(fd)
    with open(path, 'rb') as f:
        return f.read(), lines, nbytes


# ---- the command line against the reference's text ----
@pytest.mark.parametrize('name', sorted(CASES))
def test_cli_equals_the_reference(name, golden, where, tmp_path, capsys):
    case, entry = CASES[name], golden['cases'][name]
    d = where[case['world']]
    out = str(tmp_path / ('out.bed.gz' if case['gz'] else 'out.bed'))
    rc = wgbs_tools.main(['wgbstools', 'beta2bed'] + BC.argv_of(case, op.join(d['dir'], case['file']), d['ref'], out, d['dir']))
    if 'error' in entry:
        assert rc == 1 and entry['error'] in capsys.readouterr().err and not op.exists(out)
        return
    assert rc == 0
    with (gzip.open if case['gz'] else open)(out, 'rb') as f:
        text = f.read()
    if case['gz']:
        assert open(out, 'rb').read(2) == b'\x1f\x8b'
    if 'text' in entry:
        assert text == entry['text'].encode()
    else:
        lines = text.split(b'\n')[:-1]
        assert (len(text), len(lines)) == (entry['bytes'], entry['lines'])
        assert [ln.decode() for ln in lines[:3]] == entry['first'] and [ln.decode() for ln in lines[-3:]] == entry['last']
        assert hashlib.sha1(text).hexdigest() == entry['sha1']


def test_force_overwrites_and_stdout_is_the_default(where, tmp_path, capfd):
    d = where['small']
    beta = op.join(d['dir'], 'small.beta')
    out = str(tmp_path / 'out.bed')
    open(out, 'w').write('old\n')
    assert wgbs_tools.main(['wgbstools', 'beta2bed', beta, '--genome', d['ref'], '-o', out, '-s', '1']) == 0
    assert open(out).read() == 'old\n' and 'already exists' in capfd.readouterr().err
    assert wgbs_tools.main(['wgbstools', 'beta2bed', beta, '--genome', d['ref'], '-o', out, '-s', '1', '-f']) == 0
    assert open(out).read() == 'chr1\t4\t6\t3\t7\n'
    assert wgbs_tools.main(['wgbstools', 'beta2bed', beta, '--genome', d['ref'], '-s', '1', '--mean']) == 0
    assert capfd.readouterr().out == 'chr1\t4\t6\t0.429\n'


# ---- the ABI: slabs ----
@pytest.mark.parametrize('file_name', ['small.beta', 'small.lbeta'])
@pytest.mark.parametrize('slab_sites', [64, 256, 1000, 0])
def test_slabs_give_the_single_slab_bytes(seg, worlds, tmp_path, slab_sites, file_name):
    w = worlds['small']
    rows = _load(seg, w, file_name)
    n = len(rows)
    assert slab_sites == 0 or -(-n // slab_sites) >= 3
    for o in BC.GRID:
        want = BR.text_of(w['names'], w['sizes'], w['loci'], rows, 0, n, **o)
        got, lines, nbytes = _emit(seg, w, tmp_path, slab_sites=slab_sites, **o)
        assert got == want, (o, slab_sites)
        assert (lines, nbytes) == (want.count(b'\n'), len(want))
        assert seg.last_block_sums_ms() >= 0.0 and abs(sum(seg.beta2bed_pass_ms()) - seg.last_block_sums_ms()) < 1e-9
    # a range that begins and ends inside chromosomes and crosses two borders; one site; nothing
    for a, b in ((249, 530), (2999, 3000), (700, 700), (1000, 1600)):
        want = BR.text_of(w['names'], w['sizes'], w['loci'], rows, a, b, keep_na=False, mean=True, min_cov=2)
        got, lines, nbytes = _emit(seg, w, tmp_path, start0=a, end0=b, slab_sites=slab_sites, mean=True, min_cov=2)
        assert got == want and (lines, nbytes) == (want.count(b'\n'), len(want)), (a, b)


@pytest.mark.parametrize('file_name', ['small.beta', 'small.lbeta'])
@pytest.mark.parametrize('gap', [(256, 768), (0, 256), (2816, 3000)])
def test_empty_slabs_inside_the_pipeline(seg, worlds, tmp_path, gap, file_name):
    """slabs of 256 sites whose multiplicities are all zero — two in the middle, the first, the last — write nothing, between
    slabs that do write: the two-slab pipeline skips their emit pass and their write and keeps its place"""
    w = worlds['small']
    rows = _load(seg, w, file_name)
    n, slab = len(rows), 256
    assert n == 3000 and gap[0] % slab == 0 and (gap[1] % slab == 0 or gap[1] == n)
    mult = np.ones(n, dtype=np.uint16)
    mult[gap[0]:gap[1]] = 0
    for o in (dict(keep_na=True), dict(mean=True, min_cov=2)):
        text = lambda a, b: BR.text_of(w['names'], w['sizes'], w['loci'], rows, a, b, mult[a:b], **o)
        want = text(0, n)
        # the gap is empty, the slabs next to it are not
        assert text(*gap) == b'' and (gap[0] == 0 or text(gap[0] - slab, gap[0])) and (gap[1] == n or text(gap[1], min(gap[1] + slab, n)))
        got, lines, nbytes = _emit(seg, w, tmp_path, mult=mult, slab_sites=slab, **o)
        assert got == want, (o, gap)
        assert (lines, nbytes) == (want.count(b'\n'), len(want))
        assert sum(seg.beta2bed_pass_ms()) == seg.last_block_sums_ms()


# ---- the staging rule and the direct path ----
def _deep_mult(w):
    return BR.multiplicity_by_rows(w['names'], w['sizes'], w['loci'], BC.small_beds(w)['deep.bed']).astype(np.uint16)


@pytest.mark.parametrize('stage_bytes', [1, 64, 1000, 0])
def test_direct_path_gives_the_staged_bytes(seg, worlds, tmp_path, stage_bytes):
    w = worlds['small']
    mult = _deep_mult(w)
    assert mult.max() == 4 and (mult == 3).any() and (mult == 0).any()
    for file_name in ('small.beta', 'small.lbeta'):
        rows = _load(seg, w, file_name)
        for o in (dict(min_cov=1, mean=False, keep_na=True), dict(min_cov=2, mean=True, keep_na=False)):
            want = BR.text_of(w['names'], w['sizes'], w['loci'], rows, 0, len(rows), mult, **o)
            for slab_sites in (0, 300):
                got, lines, nbytes = _emit(seg, w, tmp_path, mult=mult, stage_bytes=stage_bytes, slab_sites=slab_sites, **o)
                assert got == want and (lines, nbytes) == (want.count(b'\n'), len(want)), (file_name, o, slab_sites)


def test_multiplicities_beyond_the_staging_area(seg, worlds, tmp_path):
    """workgroups whose text outgrows the staging area on its own (a site 700 times), beside staged ones"""
    w = worlds['small']
    rows = _load(seg, w, 'small.beta')
    rng = np.random.default_rng(BC.SEED)
    mult = rng.integers(0, 4, len(rows)).astype(np.uint16)
    mult[[3, 255, 256, 700, 2999]] = (700, 650, 2, 65534, 9)
    want = BR.text_of(w['names'], w['sizes'], w['loci'], rows, 0, len(rows), mult, keep_na=True)
    assert len(want) > 256 * 66 * 3
    for slab_sites in (0, 256, 999):
        got, lines, nbytes = _emit(seg, w, tmp_path, mult=mult, keep_na=True, slab_sites=slab_sites)
        assert got == want and (lines, nbytes) == (int(mult.sum()), len(want)), slab_sites
    part = BR.text_of(w['names'], w['sizes'], w['loci'], rows, 200, 800, mult[200:800], mean=True)
    assert _emit(seg, w, tmp_path, start0=200, end0=800, mult=mult[200:800], mean=True)[0] == part


def test_repeats_give_identical_bytes(seg, worlds, tmp_path):
    w = worlds['every_pair']
    rows = _load(seg, w, 'every_pair.beta')
    a = _emit(seg, w, tmp_path, mean=True)
    b = _emit(seg, w, tmp_path, mean=True)
    assert a == b and a[1] == int((rows[:, 1] > 0).sum())
    c = _emit(seg, w, tmp_path, mean=True, slab_sites=4099)
    assert c == a


def test_many_chromosomes_take_the_table_from_global_memory(seg, tmp_path):
    """more chromosomes than the LDS table holds"""
    n_chroms = _lib.beta2bed_limits()['max_name'] * 3                       # 93 > 64
    sizes = [3 + (i % 5) for i in range(n_chroms)]
    names = ['c%d_%s' % (i, 'x' * (i % 20)) for i in range(n_chroms)]
    n = sum(sizes)
    rng = np.random.default_rng(BC.SEED + 1)
    rows = rng.integers(0, 200, (n, 2)).astype(np.uint8)
    loci = np.concatenate([100 + 7 * np.arange(s) for s in sizes]).astype(np.uint32)
    w = dict(names=names, sizes=sizes, loci=loci)
    seg.set_betas([rows])
    seg.set_loci(loci)
    want = BR.text_of(names, sizes, loci, rows, 0, n, keep_na=True)
    assert _emit(seg, w, tmp_path, keep_na=True)[0] == want


# ---- refusals that need a device context ----
def test_refusals(worlds, tmp_path):
    w = worlds['small']
    cum = np.cumsum(w['sizes'])
    fd = os.open(str(tmp_path / 'never.bed'), os.O_WRONLY | os.O_CREAT, 0o644)
    try:
        with _lib.Segmenter(0) as s:
            with pytest.raises(_lib.SegmentorError) as e:
                s.beta2bed(fd, 0, w['names'], cum, 0, 3000)
            assert e.value.code == _lib.E_STATE and 'betas not set' in e.value.msg
            s.set_betas([w['files']['small.beta']])
            with pytest.raises(_lib.SegmentorError) as e:
                s.beta2bed(fd, 0, w['names'], cum)
            assert e.value.code == _lib.E_STATE and 'loci not set' in e.value.msg
            s.set_loci(w['loci'][:-1])
            with pytest.raises(_lib.SegmentorError) as e:
                s.beta2bed(fd, 0, w['names'], cum)
            assert e.value.code == _lib.E_STATE and '2999 vs 3000' in e.value.msg
            s.set_loci(w['loci'])
            mult = np.ones(3000, dtype=np.uint16)
            mult[1234] = 65535
            for kw, word in ((dict(start0=0, end0=3001), 'sites [0, 3001) are outside the 3000 resident sites'), (dict(start0=10, end0=9), 'sites [10, 9)'),
                             (dict(mult=mult), 'site 1234 has multiplicity 65535'), (dict(start0=1000, end0=2000, mult=mult[1000:2000]), 'site 1234 has multiplicity 65535'),
                             (dict(sample=1), 'sample 1 is outside the 1 resident samples'), (dict(min_cov=0), 'min_cov = 0'),
                             (dict(chrom_cum=cum - 1), 'chrom_cum ends at 2999'), (dict(chrom_names=['chr1', 'MT', 'c' * 32, 'chrX']), 'has 32 bytes, at most 31'),
                             (dict(slab_sites=-5), 'slab_sites = -5'), (dict(stage_bytes=1 << 20), 'stage_bytes = 1048576')):
                args = dict(sample=0, chrom_names=w['names'], chrom_cum=cum)
                args.update(kw)
                with pytest.raises(_lib.SegmentorError) as e:
                    s.beta2bed(fd, **args)
                assert e.value.code == _lib.E_ARG and word in e.value.msg, (kw, e.value.msg)
            assert s.beta2bed(fd, 0, w['names'], cum, 700, 700) == (0, 0)
        assert os.fstat(fd).st_size == 0
    finally:
        os.close(fd)


def test_a_reader_that_went_away_is_a_broken_pipe(seg, worlds):
    w = worlds['small']
    _load(seg, w, 'small.beta')
    r, wr = os.pipe()
    os.close(r)
    try:
        with pytest.raises(BrokenPipeError) as e:
            seg.beta2bed(wr, 0, w['names'], np.cumsum(w['sizes']), keep_na=True)
        assert e.value.errno == errno.EPIPE
    finally:
        os.close(wr)
    lim = _lib.beta2bed_limits()
    assert lim['default_slab'] == 1 << 20 and lim['max_name'] == 31 and lim['max_stage_bytes'] == 256 * 66


def test_a_failed_write_with_slabs_in_flight_leaves_the_context_usable(seg, worlds, tmp_path):
    """slabs of 256 sites: when the write of slab 0 fails, the text of slab 1 and the lengths of slab 2 are queued; they land in
    buffers the context keeps, and the next call on the same context writes what a single-slab call writes"""
    w = worlds['small']
    rows = _load(seg, w, 'small.beta')
    r, wr = os.pipe()
    os.close(r)
    try:
        with pytest.raises(BrokenPipeError) as e:
            seg.beta2bed(wr, 0, w['names'], np.cumsum(w['sizes']), keep_na=True, slab_sites=256)
        assert e.value.errno == errno.EPIPE
    finally:
        os.close(wr)
    got, lines, nbytes = _emit(seg, w, tmp_path, keep_na=True, slab_sites=256)
    assert (got, lines, nbytes) == _emit(seg, w, tmp_path, keep_na=True, slab_sites=len(rows)) and lines == len(rows)
    assert got == BR.text_of(w['names'], w['sizes'], w['loci'], rows, 0, len(rows), keep_na=True)
