"""`wgbstools beta_to_450k` without a GPU: the dispatcher and the flags; the "%.3f" rule of csrc/bed_fmt.h and the host plan
csrc/array_plan.h as a stand-alone program (tests/native/array_host.cpp: wg_fmt_f3 against snprintf on every uint8 pair, on the
exact ties and on 10^6 random 16-bit pairs; the text of a value; the slab arithmetic; every refusal that needs no device), built
plain and with the sanitizers; tests/array_ref.py's restatement against the text the reference printed
(tests/golden/array_cases.json); the command's own map / ref merge and warnings against the same fixture."""
import hashlib
import json
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import array_cases as AC
import array_ref as AR
from wgbs_tools_amd import _lib, beta_to_450k, wgbs_tools

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
CASES = AC.cases()


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'array_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def worlds():
    return AC.worlds()


@pytest.fixture(scope='module')
def where(tmp_path_factory, worlds):
    td = str(tmp_path_factory.mktemp('array'))
    return {name: AC.write_world(td, name, w) for name, w in worlds.items()}


def check_against(entry, text, what):
    if 'text' in entry:
        assert text == entry['text'].encode(), what
    else:
        lines = text.split(b'\n')[:-1]
        assert (len(text), len(lines)) == (entry['bytes'], entry['lines']), what
        assert [ln.decode() for ln in lines[:3]] == entry['first'] and [ln.decode() for ln in lines[-3:]] == entry['last'], what
        assert hashlib.sha1(text).hexdigest() == entry['sha1'], what


# ---- dispatcher and flags ----
def test_dispatcher_knows_the_command(capsys):
    assert 'beta_to_450k' in wgbs_tools.COMMANDS and 'beta_to_450k' not in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'beta_to_450k', '-h'])
    assert e.value.code == 0
    cap = capsys.readouterr()
    assert '--EPIC' in cap.out and 'not part of this build' not in cap.out + cap.err
    for f in ['input_files', '-o', '--out_path', '-c', '--cov_thresh', '--ref', '-@', '--threads', '--genome', '--device', 'cov_thresh are ignored [3]']:
        assert f in cap.out, f
    wgbs_tools.print_help()
    assert '\tbeta_to_450k\n' in capsys.readouterr().out
    a = beta_to_450k.parse_args(['x.beta', 'y.beta'])
    assert (a.input_files, a.cov_thresh, a.ref, a.EPIC, a.out_path, a.device) == (['x.beta', 'y.beta'], 3, None, False, '/dev/stdout', 0)
    assert 'Deliberate deviations' in beta_to_450k.__doc__
    assert {'wgbsseg_site_counts', 'wgbsseg_site_table', 'wgbsseg_site_table_limits'} <= set(_lib.EXPORTS)


def test_bad_inputs_are_refused_before_any_device_work(where, tmp_path, capsys):
    d = where['small']
    beta, out = op.join(d['dir'], 's00.beta'), str(tmp_path / 'never.csv')
    run = lambda *argv: wgbs_tools.main(['wgbstools', 'beta_to_450k'] + list(argv) + ['--genome', d['ref'], '-o', out])
    assert run(op.join(d['dir'], 'missing.beta')) == 1
    assert 'No such file' in capsys.readouterr().err
    assert run(beta, op.join(d['dir'], 's00.lbeta')) == 1
    assert 'must end with .beta' in capsys.readouterr().err
    assert run(op.join(d['dir'], 'short', 'ab.beta'), beta) == 1
    err = capsys.readouterr().err
    assert 'incomatible with current genome reference' in err and 'beta incompatible with genome' in err
    assert run(beta, op.join(d['dir'], 'short', 'ab.beta')) == 1                 # (deviation: every file is checked)
    assert 'short/ab.beta: the file and the genome hg38 differ in their number of sites' in capsys.readouterr().err
    assert run(beta, '--ref', op.join(d['dir'], 'no_such_ref.csv')) == 1
    assert 'No such file' in capsys.readouterr().err
    assert not op.exists(out)


def test_a_cpg_outside_the_genome_is_refused_by_name(worlds, tmp_path, capsys):
    w = dict(worlds['small'])
    for cpg in (0, AC.SMALL_SITES + 1):
        w['map'] = [list(r) for r in worlds['small']['map']]
        w['map'][5] = ['cg00012345', cpg, 450]
        d = AC.write_world(str(tmp_path / ('w%d' % cpg)), 'small', w, n_samples=1)
        out = str(tmp_path / 'never.csv')
        assert wgbs_tools.main(['wgbstools', 'beta_to_450k', op.join(d['dir'], 's00.beta'), '--genome', d['ref'], '-o', out]) == 1
        assert 'probe cg00012345 maps to CpG %d, outside 1 .. 3,000' % cpg in capsys.readouterr().err and not op.exists(out)


def test_a_genome_without_a_map_is_refused(where, tmp_path, capsys):
    import os
    d = where['small']
    ref = str(tmp_path / 'hg38')
    shutil.copytree(d['ref'], ref)
    os.remove(op.join(ref, 'ilmn2CpG.tsv.gz'))
    assert wgbs_tools.main(['wgbstools', 'beta_to_450k', op.join(d['dir'], 's00.beta'), '--genome', ref, '-o', str(tmp_path / 'never.csv')]) == 1
    assert 'Input file is None' in capsys.readouterr().err and not op.exists(str(tmp_path / 'never.csv'))


# ---- the native program: the "%.3f" rule and the host plan ----
def _have(flags):
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null'] + flags, input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _run_native(tmp_path, name, flags):
    exe = str(tmp_path / ('array_host_' + name))
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', op.join(ROOT, 'tests', 'native', 'array_host.cpp'), '-o', exe] + flags,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope='module')
def native(tmp_path_factory):
    return _run_native(tmp_path_factory.mktemp('native'), 'plain', [])


def test_f3_equals_snprintf(native):
    lines = native.splitlines()
    assert lines[0] == 'every 8-bit pair: 65280 checked, 0 mismatches'
    assert lines[1] == 'exact ties: 66594 checked, 0 mismatches'
    assert lines[2] == 'random 16-bit pairs: 1000000 checked, 0 mismatches'
    assert 'MISMATCH' not in native
    # the text of a value: below the threshold, 3/3, 0/0 and 7/0 let through, 7/0 not let through, meth > cov, the longest, a tie (1/16 = 0.0625)
    assert lines[3] == 'values: NA 1.000 NA inf NA 2.500 65535.000 NA 0.062'
    assert ['%.3f' % (1 / 2 ** k) for k in (4, 3)] == ['0.062', '0.125']


def test_the_tie_world_is_the_native_enumeration_cut_short():
    ties = AC.tie_pairs()
    assert len(ties) == 57471 and all((2000 * m) % c == 0 and (2000 * m // c) % 2 == 1 for m, c in ties)
    up = sum(('%.3f' % (m / c)) == '%d.%03d' % divmod(1000 * m // c + 1, 1000) for m, c in ties)
    assert 0 < up < len(ties)                                      # both directions of the rounding occur


def test_plan_constants_and_slabs(native):
    lim = dict(block=256, label=63, field=64, stage=16384, cols=4096)
    assert 'constants: block %(block)d, label %(label)d, field %(field)d, stage %(stage)d, cols %(cols)d, slab rows 65536 / 4194304, slab fields 2097152 / 67108864' % lim in native
    assert 'default slab rows: 65536 65536 63550 511' in native       # 2^21 fields: 2^21 // 33 = 63550, 2^21 // 4097 = 511
    assert 'as it is: accepted: 4 rows x 3, slabs of 65536: 1, longest label 63, bound of slab 0: 376' in native      # 4 x (64 + 3 x 10)
    assert 'slabs of 3: accepted: 4 rows x 3, slabs of 3: 2, longest label 63, bound of slab 0: 282' in native
    assert 'no rows: accepted: 0 rows x 3, slabs of 65536: 0' in native
    assert 'the largest slab: accepted' in native
    slabs = [ln for ln in native.splitlines() if ln.startswith('slab ')]
    assert slabs == ['slab %d: first %d rows %d fields %d cells %d workgroups %d bound %d' % (k, 300 * k, n, 34 * n, 33 * n, -(-34 * n // 256), n * (11 + 330))
                     for k, n in enumerate((300, 300, 300, 100))]
    assert native.splitlines()[-1] == 'rows in slabs: 1000'


def test_plan_refusals_name_the_offender(native):
    said = dict(ln.split(': refused (-1): site_table: ') for ln in native.splitlines() if ': refused (' in ln)
    want = {'n_rows -1': 'n_rows = -1 is negative', 'n_cols 0': 'n_cols = 0 is outside 1 .. 4096', 'n_cols above': 'n_cols = 4097 is outside 1 .. 4096',
            'site0 NULL': 'site0 is NULL', 'samples NULL': 'samples is NULL', 'label_off NULL': 'label_off is NULL', 'labels NULL': 'labels is NULL',
            'opts NULL': 'opts is NULL', 'sample 2': 'column 1: sample 2 is outside the 2 resident samples', 'sample -1': 'column 2: sample -1 is outside',
            'site 3000': 'row 1: site 3000 is outside the 3000 resident sites', 'site -1': 'row 3: site -1 is outside', 'min_cov -1': 'min_cov = -1 is negative',
            'offsets descend': 'label_off[2] = 2 descends', 'label of 65 bytes': 'the label of row 3 has 65 bytes, at most 63 are supported',
            'slab_rows -1': 'slab_rows = -1 is outside 0 .. 4194304', 'slab_rows above': 'slab_rows = 4194305 is outside',
            'too many fields': 'slab_rows = 4194304 rows of 17 fields are more than 67108864 fields in a slab'}
    assert set(said) == set(want)
    for k, word in want.items():
        assert word in said[k], (k, said[k])


@pytest.mark.skipif(not _have(SAN), reason='no g++ with sanitizer runtimes')
def test_native_program_under_sanitizers(native, tmp_path):
    assert _run_native(tmp_path, 'asan_ubsan', SAN) == native


# ---- the fixture ----
def test_restatement_equals_the_reference_text(golden, worlds, where):
    assert set(golden['cases']) == set(CASES) and golden['map_placeholder'] == AR.MAP
    whole = 0
    for name, case in CASES.items():
        entry = golden['cases'][name]
        if 'error' in entry:
            assert name == 'small_beta_short_first_file' and entry['error'] == 'beta incompatible with genome' and 'incomatible' in entry['stderr']
            continue
        d = where[case['world']]
        text, warnings = AR.case_text(worlds[case['world']], case, d['map'], op.join(d['dir'], case['ref']) if case['ref'] else None, AC.case_paths(case, where),
                                      AC.case_rows(case, worlds[case['world']]))
        check_against(entry, text, name)
        assert ''.join(x + '\n' for x in warnings) == entry['stderr'], name
        whole += 'text' in entry
    assert whole >= 25
    assert golden['cases']['small_beta_f2_c3_ref_none_known']['text'] == 'ilmn,s03,s04\n'
    assert golden['cases']['small_beta_same_base_name']['text'].startswith('ilmn,s00,s01\n')
    assert '"cg,0000comma",' in golden['cases']['small_beta_f2_c3_ref_quoted']['text']
    assert ',inf' in golden['cases']['small_beta_f1_c0']['text'] and ',inf' not in golden['cases']['small_beta_f1_c1']['text']


# ---- the command's own reading of the map and the ref, and its warnings ----
@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c['world'].startswith('small') and 'short' not in n))
def test_merge_rules_and_warnings(name, golden, where, worlds, capsys):
    case, entry = CASES[name], golden['cases'][name]
    d = where[case['world']]
    map_ids, map_cpg = beta_to_450k.load_map(d['map'], case['epic'], case['ref'] is not None)
    ref_ids = beta_to_450k.load_ref(op.join(d['dir'], case['ref'])) if case['ref'] else None
    ids, cpg = beta_to_450k.select_probes(map_ids, map_cpg, ref_ids, case['epic'], d['map'])
    said = capsys.readouterr().err.replace(d['map'], AR.MAP)
    both = AR.REF_AND_EPIC + '\n' if case['epic'] and case['ref'] else ''           # (main() says that one)
    assert both + said == entry['stderr']
    want_rows, width = AR.read_map(d['map'])
    want_ids, want_cpg, _ = AR.select(want_rows, width, AR.read_ref(op.join(d['dir'], case['ref'])) if case['ref'] else None, case['epic'])
    assert [str(i) for i in ids] == want_ids and np.array_equal(cpg, want_cpg) and cpg.dtype == np.int64
    # the text the library call is asked for, made by the restatement from the command's own selection
    names, files = beta_to_450k.columns_of(AC.case_paths(case, where))
    rows = AC.case_rows(case, worlds[case['world']])
    header = ','.join(beta_to_450k.csv_field(n) for n in ['ilmn'] + names) + '\n'
    body = AR.table_body([beta_to_450k.csv_field(str(i)) for i in ids], cpg - 1, [rows[f] for f in files], max(0, case['c']))
    check_against(entry, header.encode() + body, name)

