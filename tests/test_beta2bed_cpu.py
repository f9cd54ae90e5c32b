"""`wgbstools beta2bed` without a GPU: the dispatcher and the flags; the "%.3g" rule of csrc/bed_fmt.h, compiled for the host
(tests/native/bed_host.cpp), against Python's own '%.3g' on every uint8 pair and on the tie world; the host plan csrc/bed_plan.h
(refusals, the line bound against the fixture's longest line, the slab arithmetic, the chromosome and workgroup tables, the
text buffers' capacity, the slab parity); the -L multiplicity builder against the
row-by-row rule of tests/bed_ref.py; tests/bed_ref.py's restatement against the text the reference printed
(tests/golden/bed_cases.json); the sanitizer run of the host-only code as a stand-alone program."""
import ctypes as C
import hashlib
import json
import os
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import bed_cases as BC
import bed_ref as BR
from wgbs_tools_amd import _lib, beta2bed, wgbs_tools
from wgbs_tools_amd.genome import GenomeRefPaths, IllegalArgumentError

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
SRC = op.join(ROOT, 'tests', 'native', 'bed_host.cpp')
LIB = op.join(ROOT, 'tests', 'native', 'libbed_host.so')
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'bed_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def worlds():
    return BC.worlds()


@pytest.fixture(scope='module')
def host():
    """tests/native/libbed_host.so (built when missing or older than its sources)"""
    deps = [SRC, op.join(CSRC, 'bed_fmt.h'), op.join(CSRC, 'bed_plan.h'), op.join(ROOT, 'include', 'wgbsseg.h')]
    if not op.isfile(LIB) or any(op.getmtime(d) > op.getmtime(LIB) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', SRC, '-o', LIB])
    L = C.CDLL(LIB)
    L.bed_line_bound.restype = C.c_int64
    L.bed_line_bound.argtypes = [C.c_int64]
    L.bed_check_slab_bytes.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]
    L.bed_check_mult.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]
    L.bed_slab.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p]
    L.bed_g3.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.bed_dec.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.bed_plan.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_void_p, C.c_void_p,
                           C.c_char_p, C.c_size_t]
    L.bed_constants.argtypes = [C.c_void_p]
    L.bed_staged.argtypes = [C.c_uint32, C.c_uint32]
    L.bed_chrom_table.restype = C.c_int64
    L.bed_chrom_table.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.bed_wg_table.argtypes = [C.c_int64, C.c_void_p]
    L.bed_text_capacity.argtypes = [C.c_uint64, C.c_int64, C.c_void_p]
    L.bed_parity.argtypes = [C.c_int64]
    return L


def _constants(host):
    out = np.zeros(8, dtype=np.int64)
    host.bed_constants(out.ctypes.data)
    return dict(zip(('block', 'max_name', 'max_line', 'stage_bytes', 'default_slab', 'max_slab', 'mult_too_many', 'lds_chroms'), out.tolist()))


def _g3(host, m, c):
    m = np.ascontiguousarray(m, dtype=np.uint32)
    c = np.ascontiguousarray(c, dtype=np.uint32)
    text = np.zeros((m.size, 8), dtype=np.uint8)
    length = np.zeros(m.size, dtype=np.int32)
    host.bed_g3(m.ctypes.data, c.ctypes.data, m.size, text.ctypes.data, length.ctypes.data)
    return [bytes(t[:n]).decode() for t, n in zip(text, length.tolist())]


# ---- dispatcher and flags ----
def test_dispatcher_knows_the_command(capsys):
    assert 'beta2bed' in wgbs_tools.COMMANDS and 'beta2bed' not in wgbs_tools.REFERENCE_ONLY
    assert 'view' in wgbs_tools.REFERENCE_ONLY and 'beta2bw' in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'beta2bed', '-h'])
    assert e.value.code == 0
    cap = capsys.readouterr()
    assert '--keep_na' in cap.out and 'not part of this build' not in cap.out + cap.err
    wgbs_tools.print_help()
    assert '\tbeta2bed\n' in capsys.readouterr().out


def test_help_shows_the_reference_flags(capsys):
    with pytest.raises(SystemExit) as e:
        beta2bed.parse_args(['-h'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for f in ['beta_path', '-f', '--force', '--keep_na', '--mean', '-c', '--min_cov', '--outpath', '-o', '-s', '--sites', '-r', '--region', '-L', '--bed_file',
              '--genome', '--device', 'Only relevant if --mean is specified', 'Output path. [stdout]']:
        assert f in out, f
    a = beta2bed.parse_args(['x.beta'])
    assert (a.min_cov, a.mean, a.keep_na, a.force, a.outpath, a.bed_file) == (1, False, False, False, '/dev/stdout', None)


def test_selection_flags_exclude_each_other(capsys):
    for pair in (['-s', '1-5', '-r', 'chr1:1-100'], ['-s', '1-5', '-L', 'x.bed'], ['-r', 'chr1', '-L', 'x.bed']):
        with pytest.raises(SystemExit) as e:
            beta2bed.parse_args(['a.beta'] + pair)
        assert e.value.code == 2
        assert 'not allowed with argument' in capsys.readouterr().err


def test_bad_inputs_are_refused_before_any_device_work(tmp_path, capsys):
    w = BC.write_world(str(tmp_path), 'small')
    assert wgbs_tools.main(['wgbstools', 'beta2bed', str(tmp_path / 'missing.beta'), '--genome', w['ref']]) == 1
    assert 'No such file' in capsys.readouterr().err
    wrong = op.join(w['dir'], 'small.txt')
    shutil.copy(op.join(w['dir'], 'small.beta'), wrong)
    assert wgbs_tools.main(['wgbstools', 'beta2bed', wrong, '--genome', w['ref']]) == 1
    assert 'Invalid input format for view beta' in capsys.readouterr().err
    short = op.join(w['dir'], 'short.beta')
    open(short, 'wb').write(b'\x01\x02' * 10)
    assert wgbs_tools.main(['wgbstools', 'beta2bed', short, '--genome', w['ref']]) == 1
    err = capsys.readouterr().err
    assert 'incomatible with current genome reference' in err and 'differ in their number of sites' in err
    assert wgbs_tools.main(['wgbstools', 'beta2bed', op.join(w['dir'], 'small.beta'), '--genome', w['ref'], '-s', '250-260']) == 1
    assert 'Invalid sites input' in capsys.readouterr().err
    existing = op.join(w['dir'], 'out.bed')
    open(existing, 'w').write('kept\n')
    assert wgbs_tools.main(['wgbstools', 'beta2bed', op.join(w['dir'], 'small.beta'), '--genome', w['ref'], '-o', existing]) == 0
    assert 'already exists. Skipping it. Use [-f] flag to force overwrite.' in capsys.readouterr().err
    assert open(existing).read() == 'kept\n'


# ---- the "%.3g" rule ----
def test_g3_equals_python_on_every_uint8_pair(host):
    i = np.arange(65536)
    m, c = i >> 8, i & 255
    keep = c > 0
    got = _g3(host, m[keep], c[keep])
    want = ['%.3g' % (int(a) / int(b)) for a, b in zip(m[keep], c[keep])]
    assert len(got) == 65280 and got == want


def test_g3_equals_python_on_the_tie_world(host):
    rows, n_ties = BC.tie_rows()
    assert n_ties > 8000 and len(rows) > 40000
    m, c = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    assert (c > 0).all()
    got = _g3(host, m, c)
    want = ['%.3g' % (int(a) / int(b)) for a, b in zip(m, c)]
    bad = [(int(a), int(b), g, w) for a, b, g, w in zip(m, c, got, want) if g != w]
    assert not bad, bad[:5]
    # the ties really are ties, and both directions of the rounding occur among them
    ties = BC.tie_pairs()
    text = dict(zip(zip(m.tolist(), c.tolist()), got))
    assert text[(5, 16)] == '0.312' and text[(7, 16)] == '0.438' and text[(3, 32)] == '0.0938'
    assert text[(1, 65535)] == '1.53e-05' and text[(65535, 1)] == '6.55e+04' and text[(65535, 65535)] == '1'
    assert len(ties) == n_ties


def test_g3_forms(host):
    cases = {(0, 7): '0', (1000, 1): '1e+03', (999, 1): '999', (9995, 10): '1e+03', (1, 1000): '0.001', (1, 10000): '0.0001', (1, 8): '0.125',
             (12, 1): '12', (1205, 100): '12.1', (255, 1): '255', (200, 3): '66.7', (100, 1): '100', (2, 65535): '3.05e-05', (6, 60000): '0.0001',
             (50000, 5): '1e+04', (65535, 2): '3.28e+04'}
    got = _g3(host, [m for m, _ in cases], [c for _, c in cases])
    assert got == list(cases.values()) == ['%.3g' % (m / c) for m, c in cases]


def test_decimal_digits(host):
    v = np.array([0, 9, 10, 99, 100, 4294967293, 4294967295, 4294967296, 2 ** 64 - 1], dtype=np.uint64)
    text = np.zeros((v.size, 20), dtype=np.uint8)
    length = np.zeros(v.size, dtype=np.int32)
    host.bed_dec(v.ctypes.data, v.size, text.ctypes.data, length.ctypes.data)
    assert [bytes(t[:n]).decode() for t, n in zip(text, length.tolist())] == [str(int(x)) for x in v]


# ---- the host plan ----
def _plan(host, sample=0, n_samples=1, start0=0, end0=3000, n_total=3000, cum=(3000,), names=('chr1',), opts=(1, 0, 0, 0, 0), null_opts=False):
    cum = np.array(cum, dtype=np.int64)
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    o = _lib.BedOpts(*opts)
    out = np.zeros(4, dtype=np.int64)
    msg = C.create_string_buffer(600)
    rc = host.bed_plan(sample, n_samples, start0, end0, n_total, cum.ctypes.data if cum.size else None, arr, len(names), None if null_opts else C.addressof(o),
                       out.ctypes.data, msg, 600)
    return rc, msg.value.decode(), out.tolist()


def test_plan_refusals_name_the_offender(host):
    k = _constants(host)
    assert _plan(host)[0] == _lib.OK
    for kw, word in ((dict(sample=1), 'sample 1 is outside the 1 resident samples'), (dict(sample=-1), 'sample -1'),
                     (dict(end0=3001), 'sites [0, 3001) are outside the 3000 resident sites'), (dict(start0=5, end0=4), 'sites [5, 4)'),
                     (dict(start0=-1), 'sites [-1, 3000)'), (dict(opts=(0, 0, 0, 0, 0)), 'min_cov = 0 must be at least 1'),
                     (dict(opts=(-3, 1, 0, 0, 0)), 'min_cov = -3'), (dict(cum=(1, 2999), names=('a', 'b')), 'chrom_cum ends at 2999, the resident rows have 3000 sites'),
                     (dict(cum=(5, 4, 3000), names=('a', 'b', 'c')), 'chrom_cum[1] = 4 descends'),
                     (dict(names=('c' * (k['max_name'] + 1),)), 'has %d bytes, at most %d are supported' % (k['max_name'] + 1, k['max_name'])),
                     (dict(names=('',)), 'chromosome 0 has no name'), (dict(cum=(), names=()), 'chromosome table is empty'),
                     (dict(opts=(1, 0, 0, k['stage_bytes'] + 1, 0)), 'stage_bytes = %d' % (k['stage_bytes'] + 1)), (dict(opts=(1, 0, 0, -1, 0)), 'stage_bytes = -1'),
                     (dict(opts=(1, 0, 0, 0, k['max_slab'] + 1)), 'slab_sites = %d' % (k['max_slab'] + 1)), (dict(opts=(1, 0, 0, 0, -1)), 'slab_sites = -1'),
                     (dict(null_opts=True), 'opts is NULL')):
        rc, msg, _ = _plan(host, **kw)
        assert rc == _lib.E_ARG and word in msg and msg.startswith('beta2bed: '), (kw, msg)
    assert _plan(host, names=('c' * k['max_name'],))[0] == _lib.OK
    msg = C.create_string_buffer(600)
    mult = np.full(1000, 7, dtype=np.uint16)
    assert host.bed_check_mult(mult.ctypes.data, mult.size, 40, msg, 600) == _lib.OK and host.bed_check_mult(None, 1000, 0, msg, 600) == _lib.OK
    mult[123] = k['mult_too_many']
    assert host.bed_check_mult(mult.ctypes.data, mult.size, 40, msg, 600) == _lib.E_ARG
    assert 'site 163 has multiplicity 65535' in msg.value.decode()
    assert host.bed_check_slab_bytes(2 ** 32 - 1, 3, 1000, msg, 600) == _lib.OK
    assert host.bed_check_slab_bytes(2 ** 32, 3, 1000, msg, 600) == _lib.E_CAPACITY
    assert 'slab 3 (1000 sites) would write 4294967296 bytes' in msg.value.decode()


def test_line_bound_holds_for_the_longest_line(host, golden, worlds):
    k = _constants(host)
    assert k['block'] == 256 and k['max_line'] == host.bed_line_bound(k['max_name']) and k['stage_bytes'] == k['block'] * k['max_line']
    longest = 0
    for name, case in BC.cases().items():
        w = worlds[case['world']]
        if 'error' in golden['cases'][name] or case['world'] != 'small':
            continue
        beds = BC.small_beds(w)
        text = BR.case_text(w, case, sites=golden['cases'][name].get('sites'), bed_text=beds[case['where'][1]] if case['where'] and case['where'][0] == '-L' else None)
        for line in text.split(b'\n')[:-1]:
            longest = max(longest, len(line) + 1)
            assert len(line) + 1 <= host.bed_line_bound(len(line.split(b'\t')[0])), line
    assert len('chrX\t4294967293\t4294967295\t65535\t65535\n') <= longest <= host.bed_line_bound(k['max_name'])
    # the bound is reached: the longest name, the largest locus, five-digit counts
    assert host.bed_line_bound(4) == len('chrX\t4294967294\t4294967296\t65535\t65535\n')
    assert len('%.3g' % (1 / 65535)) == 8 and host.bed_line_bound(4) >= len('chrX\t4294967294\t4294967296\t1.53e-05\n')
    assert host.bed_staged(k['stage_bytes'], k['stage_bytes']) == 1 and host.bed_staged(k['stage_bytes'] + 1, k['stage_bytes']) == 0
    assert host.bed_staged(0, 64) == 1 and host.bed_staged(65, 64) == 0


@pytest.mark.parametrize('slab_sites', [1, 255, 256, 257])
def test_slab_arithmetic(host, slab_sites):
    start0, end0 = 5, 2999
    rc, _, (got_slab, n_slabs, stage, max_name) = _plan(host, start0=start0, end0=end0, names=('chr21',), opts=(1, 0, 0, 0, slab_sites))
    assert rc == _lib.OK and got_slab == slab_sites and n_slabs == -(-(end0 - start0) // slab_sites) and max_name == 5
    at, out = start0, np.zeros(4, dtype=np.int64)
    for s in range(n_slabs):
        host.bed_slab(start0, end0, slab_sites, max_name, s, out.ctypes.data)
        first, count, wgs, bound = out.tolist()
        assert first == at and count == min(slab_sites, end0 - at) and count >= 1
        assert wgs == -(-count // 256) and bound == count * (5 + 35)
        at += count
    assert at == end0
    k = _constants(host)
    assert _plan(host)[2][:3] == [k['default_slab'], 1, k['stage_bytes']]
    assert _plan(host, start0=7, end0=7)[2][1] == 0


@pytest.mark.parametrize('n_chroms', [1, 64, 65])
def test_chromosome_table_bytes(host, n_chroms):
    """the table as the device reads it: the cumulative counts, then a 32-byte record per name, zero-padded, its length in byte 31"""
    k = _constants(host)
    names = [('c' if i % 2 else 'x' * k['max_name']) for i in range(n_chroms)]          # lengths 1 and 31
    names[-1] = 'y' * k['max_name']
    if n_chroms > 1:
        names[0] = 'z'
    cum = np.cumsum(np.arange(n_chroms) % 7 + 1).astype(np.int64)
    rec = k['max_name'] + 1
    want = cum.tobytes() + b''.join(n.encode() + bytes(rec - 1 - len(n)) + bytes([len(n)]) for n in names)
    assert len(want) == n_chroms * (8 + rec)
    out = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
    offs = np.zeros(2, dtype=np.int64)
    arr = (C.c_char_p * n_chroms)(*[n.encode() for n in names])
    size = host.bed_chrom_table(cum.ctypes.data, arr, n_chroms, out.ctypes.data, out.size, offs.ctypes.data)
    assert size == len(want) and out[:size].tobytes() == want and (out[size:] == 0xAA).all()
    assert offs.tolist() == [0, 8 * n_chroms]


@pytest.mark.parametrize('max_wgs', [1, 2, 4096])
def test_workgroup_table_layout(host, max_wgs):
    """bytes | lines | base, max_wgs words each, then the two totals: in this order, disjoint, nothing between or behind them"""
    out = np.zeros(7, dtype=np.int64)
    host.bed_wg_table(max_wgs, out.ctypes.data)
    b, l, base, tb, tl, words, size = out.tolist()
    parts = [(b, max_wgs), (l, max_wgs), (base, max_wgs), (tb, 1), (tl, 1)]
    at = 0
    for first, n in parts:
        assert first == at
        at += n
    assert words == at == 3 * max_wgs + 2 and size == 8 * words


def test_text_capacity_and_parity(host):
    out = np.zeros(2, dtype=np.uint64)
    for bound in (1, 40 * 256, 66 * (1 << 20)):
        for tot in (0, bound - 1, bound, bound + 1):
            host.bed_text_capacity(tot, bound, out.ctypes.data)
            assert out.tolist() == [max(tot, bound), max(tot, bound) + 16], (tot, bound)
    host.bed_text_capacity(2 ** 32 - 1, 1000, out.ctypes.data)
    assert out.tolist() == [2 ** 32 - 1, 2 ** 32 + 15]
    assert [host.bed_parity(k) for k in (0, 1, 2, 3, 4096, 4097, 2 ** 40 + 1)] == [0, 1, 0, 1, 0, 1, 1]


# ---- -L: the multiplicities ----
def test_multiplicities_equal_the_row_by_row_rule(tmp_path, worlds):
    w = worlds['small']
    where = BC.write_world(str(tmp_path), 'small', w)
    genome = GenomeRefPaths(where['ref'])
    from wgbs_tools_amd.beta_stats import bed_rows
    for name, text in BC.small_beds(w).items():
        want = BR.multiplicity_by_rows(w['names'], w['sizes'], w['loci'], text)
        first, mult = beta2bed.multiplicities(genome, bed_rows(op.join(where['dir'], name)))
        got = np.zeros(len(want), dtype=np.int64)
        got[first:first + mult.size] = mult
        assert np.array_equal(got, want), name
        assert mult.dtype == np.uint16 and (mult.size == 0 or (mult[0] > 0 and mult[-1] > 0)), name
    deep = BR.multiplicity_by_rows(w['names'], w['sizes'], w['loci'], BC.small_beds(w)['deep.bed'])
    assert deep.max() == 4 and (deep == 3).any()
    # more rows over one site than a uint16 counts
    many = [('chrX', 9, 11)] * 65535
    with pytest.raises(IllegalArgumentError, match='65,535 rows over CpG 514'):
        beta2bed.multiplicities(genome, many)
    assert int(beta2bed.multiplicities(genome, many[:-1])[1][0]) == 65534


# ---- the fixture ----
def _check_against(entry, text, what):
    if 'text' in entry:
        assert text == entry['text'].encode(), what
    else:
        lines = text.split(b'\n')[:-1]
        assert (len(text), len(lines)) == (entry['bytes'], entry['lines']), what
        assert [ln.decode() for ln in lines[:3]] == entry['first'] and [ln.decode() for ln in lines[-3:]] == entry['last'], what
        assert hashlib.sha1(text).hexdigest() == entry['sha1'], what


def test_restatement_equals_the_reference_text(golden, worlds):
    assert golden['stand_ins']['bedtools_for_L'] is False and set(golden['cases']) == set(BC.cases())
    beds = BC.small_beds(worlds['small'])
    whole = 0
    for name, case in BC.cases().items():
        entry = golden['cases'][name]
        if 'error' in entry:
            assert name.startswith('small_sites_border') and entry['error'] == 'Invalid sites input'
            continue
        bed = beds[case['where'][1]] if case['where'] and case['where'][0] == '-L' else None
        _check_against(entry, BR.case_text(worlds[case['world']], case, sites=entry.get('sites'), bed_text=bed), name)
        whole += 'text' in entry
    assert whole >= 15
    assert golden['cases']['small_empty_run']['text'] == '' and golden['cases']['small_L_nothing_mean']['text'] == ''


# ---- sanitizers: the host-only code as a stand-alone program ----
def _have(flags):
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null'] + flags, input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


@pytest.mark.skipif(not _have(SAN), reason='no g++ with sanitizer runtimes')
def test_formatter_and_plan_under_sanitizers(tmp_path):
    """csrc/bed_fmt.h and csrc/bed_plan.h compiled plain and with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
    program (tests/native/san_bed.cpp): both finish clean and print the same lines"""
    outs = []
    for name, flags in (('plain', []), ('asan_ubsan', SAN)):
        exe = str(tmp_path / ('san_bed_' + name))
        r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-I', CSRC, op.join(ROOT, 'tests', 'native', 'san_bed.cpp'), '-o', exe] + flags,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert lines[0] == 'g3 mismatches: 0' and lines[1] == 'digits: 1 10 20'
    assert sum(': refused (-1): ' in ln for ln in lines) == 13 and sum(': accepted: ' in ln for ln in lines) == 3
    assert 'mult: -1 beta2bed: site 1039 has multiplicity 65535' in outs[0] and 'slab bytes: 0 -6 beta2bed: slab 3' in outs[0]
    tables = [ln for ln in lines if ln.startswith('table of ')]
    assert [ln.split(',')[0] + ln.split(',')[2] for ln in tables] == ['table of 1: 40 bytes (cum 0 last record 1 bytes', 'table of 4: 160 bytes (cum 0 last record 31 bytes',
                                                                        'table of 65: 2600 bytes (cum 0 last record 31 bytes']
    assert 'wg table of 4096: 0 4096 8192 12288 12289, 12290 words, 98320 bytes' in lines
    assert 'capacity for 10001 of 10000: 10001 at home, 10017 on the device' in lines and lines[-1] == 'parity: 0 1 0 1'
