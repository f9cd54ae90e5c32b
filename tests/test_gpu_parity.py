"""GPU parity tests: the HIP path (through the C ABI, libwgbsseg.so) against the oracle, the committed golden
vectors and numpy, stage by stage so that a failure names the kernel at fault.  Bit-exact everywhere
(integer / byte / index work, and IEEE arithmetic restated exactly — no tolerance).

Most tests here compare border lists, and a border list forgives a cost that is wrong in its last bits.  The scored blocks
(fp64 bit patterns) and the back-pointers themselves are compared with the oracle's in tests/test_gpu_intermediates.py: every
CHUNK_CASES entry but two, every forced tile shape and division core, the worlds of test_16 / test_17 / test_18 chunk by chunk
in their batches, every recurrence build and staging.  Borders only, still: `default_chunk` and `deep_long` (the oracle's
debug band is ~480 MB for each) and the full-size runs (test_gpu_fullsize.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import staging
from intermediates import _first_diff, _numpy_windows
from oracle import oracle
from wgbs_tools_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    s = _lib.Segmenter(0)
    yield s
    s.close()


def _load_case(seg, spec):
    slices, loci = cases.build_case(spec)
    seg.set_betas(slices)
    seg.set_loci(loci)
    return slices, loci


# ---------------------------------------------------------------------------------------------------------
# 1. arithmetic: the device restatement of the platform libm, and the per-(block, sample) term
# ---------------------------------------------------------------------------------------------------------
def test_01_device_log2_matches_host_libm_exhaustively(seg):
    """Every float p in (0,1]: device log2f(p) == live libm; device exact log2(1-(double)p) == live libm; device fast
    log2 == the host build of the same code bit for bit (IEEE fma), hence within the 1 ulp measured on the host."""
    from test_exact_log2_cpu import load_exact, FAST_FIRST
    H = load_exact()
    O = oracle.lib()
    threads = os.cpu_count() or 1
    first, last = 0x00800000, 0x3f800000
    B = 1 << 25
    bad_f = bad_d = bad_g = 0
    max_ulp = 0
    msg = ''
    q = first
    while q <= last:
        cnt = min(B, last - q + 1)
        f, d, g = seg.debug_log2(q, cnt, want_fast=True)
        fb = C.c_uint32(0)
        nf = O.probe_log2f_compare(q, cnt, f.ctypes.data, threads, C.byref(fb))
        if nf and not msg:
            msg = 'log2f first bad bits 0x%08x' % fb.value
        cnt_d = cnt if q + cnt - 1 < last else cnt - 1
        nd = O.probe_log2_1mp_compare(q, cnt_d, d.ctypes.data, threads, C.byref(fb)) if cnt_d else 0
        if nd and not msg:
            msg = 'log2(1-p) first bad bits 0x%08x' % fb.value
        if cnt_d:
            hg = np.empty(cnt_d, np.uint64)
            H.fast_log2_1mp_fill(q, cnt_d, hg.ctypes.data, threads)
            bad_g += int((hg != g[:cnt_d]).sum())
            lo_f = max(q, FAST_FIRST)                    # ulp bound only claimed for x = 1 - p strictly below 1
            if q + cnt_d > lo_f:
                gg = np.ascontiguousarray(g[lo_f - q:cnt_d])
                max_ulp = max(max_ulp, int(O.probe_log2_1mp_maxulp(lo_f, gg.size, gg.ctypes.data, threads)))
        bad_f += nf
        bad_d += nd
        q += cnt
    assert bad_f == 0 and bad_d == 0 and bad_g == 0 and max_ulp <= 1, \
        'log2f mismatches %d, log2(1-p) mismatches %d, fast log2 device!=host %d, fast log2 max ulp %d; %s' % (bad_f, bad_d, bad_g, max_ulp, msg)


@pytest.mark.parametrize('pcount', [15.0, 0.0, 0.5, 0.99999994, 1.0, 4.0, 3.9999998, 1e-30, 2e-6, 16777216.0, 3e38])
def test_02_device_sample_term_matches_oracle(seg, pcount):
    """20 M (nmeth, ntotal) pairs per pseudo-count: the device term (fast log2 + exact fallback) == the oracle's."""
    from test_exact_log2_cpu import _term_inputs
    m, t = _term_inputs(1234, 10000000)
    got = seg.debug_sample_terms(m, t, pcount)
    want = np.empty_like(t)
    th = os.cpu_count() or 1
    import threading
    parts = np.array_split(np.arange(t.size), th)

    def work(ix):
        want[ix] = oracle.sample_terms(m[ix], t[ix], pcount)
    ths = [threading.Thread(target=work, args=(ix,)) for ix in parts]
    [x.start() for x in ths]
    [x.join() for x in ths]
    assert _first_diff(got.view(np.uint32), want.view(np.uint32)) is None, _first_diff(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('pcount', [15.0, 0.0, 0.5, 1.0, 2e-6, 3.25])
def test_02b_division_core_equals_ieee_division(seg, pcount):
    """p = (nmeth+pc)/(ntotal+2pc): the kernel's 8-instruction division core vs the compiler's IEEE `/`, on the device,
    for EVERY (nmeth, ntotal) with ntotal <= 4000 (8 M pairs) plus 8 M random pairs up to 255*1000."""
    pc = np.float32(pcount)
    t = np.repeat(np.arange(1, 4001, dtype=np.int64), np.arange(2, 4002))
    m = np.concatenate([np.arange(0, tt + 1) for tt in range(1, 4001)])
    rng = np.random.default_rng(3)
    t2 = rng.integers(1, 255 * 1000 + 1, 8000000)
    m2 = (rng.random(t2.size) * (t2 + 1)).astype(np.int64)
    t = np.concatenate([t, t2]).astype(np.float32)
    m = np.minimum(np.concatenate([m, m2]), t).astype(np.float32)
    a = (m + pc).astype(np.float32)
    b = (t + (pc + pc)).astype(np.float32)
    fast, ieee = seg.debug_div(a, b)
    assert _first_diff(fast, ieee) is None, _first_diff(fast, ieee)
    # and the device's IEEE division is numpy's
    want = (a / b).astype(np.float32).view(np.uint32)
    assert _first_diff(ieee, want) is None


@pytest.mark.parametrize('pcount', [15.0, 1.0, 2.0, 100.0, 1000.0, 1.5, 3.25, 1.1, 7.77, 1.0000001, 123.456, 16777216.0])
def test_02c_short_division_core_is_used_only_where_it_is_exact(seg, pcount):
    """Narrow scoring tiles divide with a 4-instruction core (v_rcp_f32, quotient, one correction) when k_check_div finds it
    equal to IEEE `/` on EVERY operand pair such a tile can form with the call's pseudo count.  Here: (1) the verdict
    kernel counts exactly the mismatches that numpy finds when it compares the core's quotients with IEEE division, on the
    full lattice up to ntotal 3000 (and so is not blind); (2) integer pseudo counts pass on the whole narrow-tile domain
    (ntotal <= 255 * 60), as the distance of a / b from a rounding midpoint guarantees."""
    pc = np.float32(pcount)
    T = 3000
    t = np.repeat(np.arange(0, T + 1, dtype=np.int64), np.arange(1, T + 2))
    m = np.concatenate([np.arange(0, tt + 1) for tt in range(0, T + 1)])
    a = (m.astype(np.float32) + pc).astype(np.float32)
    b = (t.astype(np.float32) + (pc + pc)).astype(np.float32)
    short = seg.debug_div_short(a, b)
    want = (a / b).astype(np.float32).view(np.uint32)
    n_bad = int((short != want).sum())
    assert seg.debug_check_div(pcount, T) == n_bad
    full = seg.debug_check_div(pcount)
    print('pseudo count %r: %d of %d pairs differ up to ntotal %d, %d on the narrow-tile domain' % (pcount, n_bad, a.size, T, full))
    if float(pcount).is_integer() and pcount < 2 ** 23:
        assert full == 0


def test_02d_verdict_kernel_is_not_blind(seg):
    """Where the short core cannot work — a pseudo count whose double overflows: b = inf, IEEE gives 0, the core's residual is
    NaN — the verdict kernel must count every pair.  (On full-width random floats the core has not been seen to differ from
    IEEE division at all — v_rcp_f32 is better than its 1 ulp bound there — which is recorded here, not relied upon.)"""
    assert seg.debug_check_div(3e38, 100) == 101 * 102 // 2
    rng = np.random.default_rng(11)
    a = rng.uniform(1.0, 2.0, 20000000).astype(np.float32)
    b = rng.uniform(1.0, 2.0, 20000000).astype(np.float32)
    short = seg.debug_div_short(a, b)
    want = (a / b).astype(np.float32).view(np.uint32)
    print('short core vs IEEE on 2e7 random pairs of full-width floats: %d differ' % int((short != want).sum()))


@pytest.mark.parametrize('ti,ns', [(128, 0), (64, 0), (32, 0), (16, 0), (64, 4), (32, 8)])
def test_07d_every_narrow_tile_shape_on_every_case(ti, ns, golden_chunks):
    """The launcher picks the narrow tile width (128 / 64 / 32 / 16 start sites; 128 with its block -> start byte map) and the
    samples per LDS group by cohort size and LDS budget; here every shape is forced onto every golden case (a shape that does
    not fit a case's LDS budget falls back to the launcher's choice)."""
    os.environ['WGBSSEG_TI'] = str(ti)
    if ns: os.environ['WGBSSEG_NS'] = str(ns)
    try:
        sg = _lib.Segmenter(0)
    finally:
        del os.environ['WGBSSEG_TI']
        os.environ.pop('WGBSSEG_NS', None)
    try:
        for name in cases.CHUNK_CASES:
            g = golden_chunks[name]
            spec = g['spec']
            _load_case(sg, spec)
            got = sg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
            assert got.tolist() == g['borders'], '%s, TI %d NS %d: %s' % (name, ti, ns, _first_diff(got, np.array(g['borders'])))
    finally:
        sg.close()


def test_07c_full_division_core_on_every_case(golden_chunks):
    """WGBSSEG_DIV_SHORT=0 keeps the 8-instruction core in the narrow tiles: same borders on every golden case."""
    os.environ['WGBSSEG_DIV_SHORT'] = '0'
    try:
        sg = _lib.Segmenter(0)
    finally:
        del os.environ['WGBSSEG_DIV_SHORT']
    try:
        for name in cases.CHUNK_CASES:
            g = golden_chunks[name]
            spec = g['spec']
            _load_case(sg, spec)
            got = sg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
            assert got.tolist() == g['borders'], '%s: %s' % (name, _first_diff(got, np.array(g['borders'])))
    finally:
        sg.close()


# ---------------------------------------------------------------------------------------------------------
# 2. scan pass
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('start0,length', [(0, 1), (0, 64), (3, 700), (8, 512), (13, 5000), (1001, 60000), (0, 4097)])
def test_03_prefix_sums_equal_numpy_cumsum(seg, start0, length):
    n = 70000
    slices = [synth.synth_betas(cases.SEED, s, 0, n) for s in range(5)]
    seg.set_betas(slices)
    got = seg.prefix_sums(start0, length)
    for s, sl in enumerate(slices):
        want = np.zeros((length + 1, 2), dtype=np.uint32)
        want[1:] = np.cumsum(sl[start0:start0 + length].astype(np.uint32), axis=0)
        assert _first_diff(got[s], want) is None, 'sample %d: %s' % (s, _first_diff(got[s], want))


def test_04_meth_gt_cov_is_reported(seg):
    spec = cases.CHUNK_CASES['tiny']
    slices, loci = cases.build_case(spec)
    slices[1][37, 0] = slices[1][37, 1] + 1
    seg.set_betas(slices)
    seg.set_loci(loci)
    with pytest.raises(_lib.SegmentorError) as e:
        seg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])
    assert e.value.code == _lib.E_METH_GT_COV and 'sample 1' in e.value.msg and 'site 37' in e.value.msg
    # a bad site OUTSIDE the requested chunks is not an error (the reference only reads the chunk's bytes)
    b = seg.segment_chunks([40], [spec['n'] - 40], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
    assert b[0] == 0 and b[-1] == spec['n'] - 40


@pytest.mark.parametrize('piece', [0, 1024, 4096])
def test_04b_validation_pass_sees_every_site_of_every_chunk_and_nothing_else(piece, monkeypatch):
    """The read-only scan of a job without wide tiles works on the union of the chunks, cut into pieces: a `meth > cov` site is
    found wherever it sits (first / last site of a chunk, either side of a piece boundary, in a patch-like chunk that overlaps
    others, in the last vector of the row), the LOWEST (sample, site) is the one named, sites between chunks are never read,
    and a region-level call (chunks + junction patches in one batch, patches again in the follow-up batch) reports it too."""
    if piece: monkeypatch.setenv('WGBSSEG_SCAN_PIECE_SITES', str(piece))
    sg = _lib.Segmenter(0)
    try:
        n, N = 40003, 3                                                    # (no multiple of the 8 sites of a 16-byte vector)
        rng = np.random.default_rng(5)
        clean = [synth.synth_betas(cases.SEED, s, 0, n) for s in range(N)]
        loci = np.cumsum(rng.integers(2, 300, n)).astype(np.uint32)
        sg.set_loci(loci)
        chunks = [(100, 9000), (9100, 5000), (14100, 3333), (17433, 4096), (21529, 18471 - 100), (8900, 400), (14000, 300)]   # two runs + a gap [39900, n), two overlapping patch-like chunks
        st0 = [c[0] for c in chunks]; ln = [c[1] for c in chunks]
        covered = np.zeros(n, dtype=bool)
        for a, l in chunks: covered[a:a + l] = True
        def run(bad):
            sl = [x.copy() for x in clean]
            for s_, site in bad: sl[s_][site, 0] = sl[s_][site, 1] + 1
            sg.set_betas(sl)
            return sg.segment_chunks(st0, ln, 15.0, 1000, 2000)
        run([])                                                                    # clean: no error
        for site in [100, 9099, 9100, 14099, 14100, 1023, 1024, 1025, 4095, 4096, 16383, 16384, 16385, 17432, 17433, 21528, 21529, 32768, 39899]:
            assert covered[site]
            for s_ in (0, N - 1):
                with pytest.raises(_lib.SegmentorError) as e:
                    run([(s_, site)])
                assert e.value.code == _lib.E_METH_GT_COV and 'sample %d' % s_ in e.value.msg and 'site %d ' % site in e.value.msg, (site, s_, e.value.msg)
        for site in [0, 99, 39900, 39999, 40002]:                                  # outside every chunk: never read
            assert not covered[site]
            run([(1, site)])
        with pytest.raises(_lib.SegmentorError) as e:                              # the lowest (sample, site) wins
            run([(2, 150), (1, 30000), (1, 9000), (2, 120)])
        assert 'sample 1' in e.value.msg and 'site 9000 ' in e.value.msg
        # region level: [1, n] in chunks of 5000 -> chunks + junction patches (+ follow-up batches of patches)
        sl = [x.copy() for x in clean]
        sg.set_betas(sl)
        ok, _ = sg.segment_regions([1], [n + 1], 5000, 15.0, 1000, 2000)
        assert ok[0][0] == 1 and ok[0][-1] == n + 1
        for site in [0, 4999, 5000, 5003, 39999, 40000, 40002]:
            sl = [x.copy() for x in clean]
            sl[1][site, 0] = sl[1][site, 1] + 1
            sg.set_betas(sl)
            with pytest.raises(_lib.SegmentorError) as e:
                sg.segment_regions([1], [n + 1], 5000, 15.0, 1000, 2000)
            assert e.value.code == _lib.E_METH_GT_COV and 'site %d ' % site in e.value.msg, e.value.msg
    finally:
        sg.close()


# ---------------------------------------------------------------------------------------------------------
# 3. window extents, scored blocks, recurrence — against the oracle's intermediates
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny', 'max_cpg_binds', 'dense_w_gt_64', 'equal_loci', 'zero_stretch', 'island_mix', 'deep'])
def test_05_intermediates_match_oracle(name, golden_chunks):
    os.environ['WGBSSEG_FORCE_STAGES'] = '1'
    try:
        sg = _lib.Segmenter(0)
    finally:
        del os.environ['WGBSSEG_FORCE_STAGES']
    try:
        spec = golden_chunks[name]['spec']
        slices, loci = _load_case(sg, spec)
        n, max_cpg = spec['n'], spec['max_cpg']
        got = sg.segment_chunks([0], [n], spec['pcount'], max_cpg, spec['max_bp'])[0]
        staging.assert_form(sg.last_plan(), n, stages=1, gated=0, label=name)
        W = _numpy_windows(loci, max_cpg, spec['max_bp'])
        gW = sg.debug_fetch('window', np.uint16, n).astype(np.int64)
        assert _first_diff(gW, W) is None, 'window: ' + _first_diff(gW, W)
        cum = np.concatenate([[0], np.cumsum(W)[:-1]])
        gcum = sg.debug_fetch('cum', np.uint32, n).astype(np.int64)
        assert _first_diff(gcum, cum) is None, 'cum: ' + _first_diff(gcum, cum)
        b, M, T, band = oracle.segment_chunk(slices, loci, spec['pcount'], max_cpg, spec['max_bp'], debug=True)
        # the device matrix is start-major like the oracle's band: row k = band[k, 0..F_k)
        gcost = sg.debug_fetch('cost', np.float64, int(W.sum()))
        want = np.empty(int(W.sum()), dtype=np.float64)
        for k in range(n):
            want[cum[k]:cum[k] + W[k]] = band[k, :W[k]]
        d = _first_diff(gcost.view(np.uint64), want.view(np.uint64))
        if d is not None:
            j = int(np.flatnonzero(gcost.view(np.uint64) != want.view(np.uint64))[0])
            k = int(np.searchsorted(cum, j, 'right') - 1)
            raise AssertionError('cost: %s (start site %d, end %d): got %r want %r' % (d, k, k + j - cum[k], gcost[j], want[j]))
        gback = sg.debug_fetch('back', np.uint16, n).astype(np.int64)
        wback = np.arange(1, n + 1) - T[1:]
        assert _first_diff(gback, wback) is None, 'back-pointers: ' + _first_diff(gback, wback)
        assert got.tolist() == b.tolist()
    finally:
        sg.close()


# ---------------------------------------------------------------------------------------------------------
# 4. borders against the golden vectors captured from the reference binary
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.CHUNK_CASES))
def test_06_borders_match_reference_golden(seg, name, golden_chunks):
    g = golden_chunks[name]
    spec = g['spec']
    slices, loci = _load_case(seg, spec)
    assert cases.case_checksum(slices, loci) == g['input_crc32']
    got = seg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
    assert got.tolist() == g['borders'], _first_diff(got, np.array(g['borders']))


@pytest.mark.parametrize('name', list(cases.OFFSET_CASES))
def test_06b_chunks_inside_a_world_match_reference_golden(name, golden_offsets):
    """Chunks of a larger resident world, on and next to the boundaries of carries (every 128th absolute site), units, tiles and
    batches, against the reference binary's `-s start0 -n len` output: every chunk alone, then all in one batch; another job's
    numbers are left in the device buffers first."""
    g = golden_offsets[name]
    spec = g['spec']
    with _lib.Segmenter(0) as sg:
        slices, loci = _load_case(sg, spec)
        assert cases.case_checksum(slices, loci) == g['input_crc32']
        n = spec['n']
        poison = ([3, n // 3 + 1, 2 * (n // 3) + 2], [n // 3 - 7, n // 3 - 1, n - 2 * (n // 3) - 2])
        sg.segment_chunks(poison[0], poison[1], 100.0, 200, 100000)
        for (st, ln), want in zip(g['chunks'], g['borders']):
            got = sg.segment_chunks([st], [ln], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
            assert got.tolist() == want, 'chunk [%d,+%d) alone: %s' % (st, ln, _first_diff(got, np.array(want)))
        sg.segment_chunks(poison[0], poison[1], 100.0, 200, 100000)
        res = sg.segment_chunks([c[0] for c in g['chunks']], [c[1] for c in g['chunks']], spec['pcount'], spec['max_cpg'], spec['max_bp'])
        for (st, ln), got, want in zip(g['chunks'], res, g['borders']):
            assert got.tolist() == want, 'chunk [%d,+%d) of the batch: %s' % (st, ln, _first_diff(got, np.array(want)))


@pytest.mark.parametrize('stages', [2, 3, 7, 64])
def test_07_staging_does_not_change_borders(stages, golden_chunks):
    os.environ['WGBSSEG_FORCE_STAGES'] = str(stages)
    try:
        sg = _lib.Segmenter(0)
    finally:
        del os.environ['WGBSSEG_FORCE_STAGES']
    try:
        for name in ['default_chunk', 'dense_w_gt_64', 'deep']:
            g = golden_chunks[name]
            spec = g['spec']
            _load_case(sg, spec)
            got = sg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
            assert got.tolist() == g['borders'], '%s with %d stages: %s' % (name, stages, _first_diff(got, np.array(g['borders'])))
            assert sg.timings()['n_stages'] >= min(stages, 2)
            # the form that ran: the bounds of `stages` forced stages; gated (the default switches) only with no other context alive on the device
            plan = staging.assert_form(sg.last_plan(), spec['n'], stages=stages, dp_mode=staging.auto_dp_mode(sg.timings()['max_window']),
                                       default_gate=True, label='%s, %d stages' % (name, stages))
            assert plan['n_stages'] == sg.timings()['n_stages']
    finally:
        sg.close()


@pytest.mark.parametrize('stages,slack,last_pct', [(3, 1, 100), (7, 8, 40), (8, 4096, 300), (5, 64, 200)])
def test_07c_gated_stages_and_a_short_last_stage(stages, slack, last_pct, golden_chunks):
    """A staged all-narrow job with its stages alternating between the two scoring streams behind k_stage_gate (WGBSSEG_STAGE_GATE = tiles of
    slack) and with a LAST stage shorter than the others (WGBSSEG_LAST_STAGE_PCT): only the timing may change.  Cases with wider windows
    (dense_w_gt_64, deep) are gated under the same switches too, as last_plan() shows: WGBSSEG_STAGE_GATE_SHARED=1 lifts both the
    one-context rule and the evaluations-per-step threshold that keeps a job with medium / wide tiles off the gate by default (plan_stages);
    their recurrences are the 32-step builds, so no stage of theirs runs k_dp16."""
    os.environ['WGBSSEG_FORCE_STAGES'] = str(stages)
    os.environ['WGBSSEG_STAGE_GATE'] = str(slack)
    os.environ['WGBSSEG_LAST_STAGE_PCT'] = str(last_pct)
    os.environ['WGBSSEG_STAGE_GATE_SHARED'] = '1'              # (other tests' contexts are alive on the device: gate all the same)
    try:
        sg = _lib.Segmenter(0)
    finally:
        for k in ('WGBSSEG_FORCE_STAGES', 'WGBSSEG_STAGE_GATE', 'WGBSSEG_LAST_STAGE_PCT', 'WGBSSEG_STAGE_GATE_SHARED'):
            del os.environ[k]
    try:
        for rep in range(2):                                   # (twice: the second run finds the first one's counters and buffers)
            for name in ['default_chunk', 'dense_w_gt_64', 'deep']:
                g = golden_chunks[name]
                spec = g['spec']
                _load_case(sg, spec)
                got = sg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
                assert got.tolist() == g['borders'], '%s with %d gated stages: %s' % (name, stages, _first_diff(got, np.array(g['borders'])))
                assert sg.timings()['n_stages'] >= 2
                plan = staging.assert_form(sg.last_plan(), spec['n'], stages=stages, gated=1, last_pct=last_pct,
                                           dp_mode=staging.auto_dp_mode(sg.timings()['max_window']), label='%s, %d gated stages' % (name, stages))
                assert plan['n_stages'] >= 2 and plan['all_narrow'] == (sg.timings()['max_window'] <= 60)
            g = golden_chunks['chr21']
            spec = g['spec']
            _load_case(sg, spec)
            starts = np.array(g['starts'], dtype=np.int64)
            lens = np.minimum(spec['chunk'], spec['n'] - starts).astype(np.int32)
            res = sg.segment_chunks(starts, lens, spec['pcount'], spec['max_cpg'], spec['max_bp'])
            for c, (got, want) in enumerate(zip(res, g['borders'])):
                assert got.tolist() == want, 'chr21 chunk %d, %d gated stages: %s' % (c, stages, _first_diff(got, np.array(want)))
            plan = staging.assert_form(sg.last_plan(), int(lens.max()), stages=stages, gated=1, last_pct=last_pct, label='chr21, %d gated stages' % stages)
            assert plan['n_stages'] >= 2 and plan['n_chunks'] == len(starts)
    finally:
        sg.close()


@pytest.mark.parametrize('mode,stages', [(1, 0), (2, 0), (1, 3), (2, 2), (1, 64)])
def test_07b_wide_window_recurrence_on_every_case(mode, stages, golden_chunks):
    """The recurrence has three builds (64-step batches; 32-step batches with a second pending register and worker
    pushes for blocks > 128 sites; the same with 15 worker waves).  The launcher picks by the job's widest window;
    here the wide builds are forced onto EVERY golden case, alone and across stage boundaries."""
    os.environ['WGBSSEG_DP_MODE'] = str(mode)
    if stages: os.environ['WGBSSEG_FORCE_STAGES'] = str(stages)
    try:
        sg = _lib.Segmenter(0)
    finally:
        del os.environ['WGBSSEG_DP_MODE']
        os.environ.pop('WGBSSEG_FORCE_STAGES', None)
    try:
        for name in cases.CHUNK_CASES:
            g = golden_chunks[name]
            spec = g['spec']
            _load_case(sg, spec)
            got = sg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
            assert got.tolist() == g['borders'], '%s, dp mode %d, %d stages: %s' % (name, mode, stages, _first_diff(got, np.array(g['borders'])))
            plan = staging.assert_form(sg.last_plan(), spec['n'], stages=stages or None, dp_mode=max(mode, staging.auto_dp_mode(sg.timings()['max_window'])),
                                       default_gate=True, label='%s, dp mode %d, %d stages' % (name, mode, stages))
            assert plan['dp16'] == [0] * plan['n_stages']            # a forced wide build: k_dp16 in no stage
        g = golden_chunks['chr21']
        spec = g['spec']
        _load_case(sg, spec)
        starts = np.array(g['starts'], dtype=np.int64)
        lens = np.minimum(spec['chunk'], spec['n'] - starts).astype(np.int32)
        res = sg.segment_chunks(starts, lens, spec['pcount'], spec['max_cpg'], spec['max_bp'])
        for c, (got, want) in enumerate(zip(res, g['borders'])):
            assert got.tolist() == want, 'chr21 chunk %d, dp mode %d: %s' % (c, mode, _first_diff(got, np.array(want)))
        staging.assert_form(sg.last_plan(), int(lens.max()), stages=stages or None, dp_mode=max(mode, staging.auto_dp_mode(sg.timings()['max_window'])),
                            default_gate=True, label='chr21, dp mode %d, %d stages' % (mode, stages))
    finally:
        sg.close()


def test_08_chr21_shaped_multichunk_matches_reference_golden(seg, golden_chunks):
    """BASELINE.json configs[1]: 400,000 CpGs x 8 betas, default chunk grid, bit-exact vs the CPU reference."""
    g = golden_chunks['chr21']
    spec = g['spec']
    slices, loci = _load_case(seg, spec)
    assert cases.case_checksum(slices, loci) == g['input_crc32']
    starts = np.array(g['starts'], dtype=np.int64)
    lens = np.minimum(spec['chunk'], spec['n'] - starts).astype(np.int32)
    res = seg.segment_chunks(starts, lens, spec['pcount'], spec['max_cpg'], spec['max_bp'])
    for c, (got, want) in enumerate(zip(res, g['borders'])):
        assert got.tolist() == want, 'chunk %d: %s' % (c, _first_diff(got, np.array(want)))
    t = seg.timings()
    assert t['sites'] == spec['n'] and t['evals'] == t['pairs'] * 8


def test_09_many_small_and_ragged_chunks_match_oracle(seg):
    """The shape of the stitching batch (segment.py:199-232): hundreds of ~100-site patches, plus ragged sizes,
    overlapping ranges, 1-site chunks and chunks ending at the last site."""
    n = 50000
    slices = [synth.synth_betas(cases.SEED, s, 0, n) for s in range(6)]
    loci = synth.synth_loci(cases.SEED, [n])
    seg.set_betas(slices)
    seg.set_loci(loci)
    rng = np.random.default_rng(7)
    starts = list(range(50, n - 200, 97))
    lens = [100] * len(starts)
    for _ in range(200):
        ln = int(rng.integers(1, 700))
        st = int(rng.integers(0, n - ln + 1))
        starts.append(st)
        lens.append(ln)
    starts += [n - 1, n - 64, n - 65, 0, 0]
    lens += [1, 64, 65, 1, 2]
    got = seg.segment_chunks(starts, lens, 15.0, 1000, 2000)
    want = oracle.segment_chunks(slices, loci, starts, lens, 15.0, 1000, 2000, threads=os.cpu_count() or 1)
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.tolist() == b.tolist(), 'chunk %d [%d,+%d): %s' % (c, starts[c], lens[c], _first_diff(a, b))


def test_10_one_shot_host_entry_point(golden_chunks):
    g = golden_chunks['tiny']
    spec = g['spec']
    slices, loci = cases.build_case(spec)
    res = _lib.segment_chunks_host(slices, loci, [0, 100], [spec['n'], 50], spec['pcount'], spec['max_cpg'], spec['max_bp'])
    assert res[0].tolist() == g['borders']
    want = oracle.segment_chunk([s[100:150] for s in slices], loci[100:150], spec['pcount'], spec['max_cpg'], spec['max_bp'])
    assert res[1].tolist() == want.tolist()


def test_11_argument_errors(seg):
    spec = cases.CHUNK_CASES['tiny']
    _load_case(seg, spec)
    for kw, code in [(dict(max_bp=0), _lib.E_ARG), (dict(max_cpg=0), _lib.E_ARG)]:
        p = dict(pcount=15.0, max_cpg=50, max_bp=700)
        p.update(kw)
        with pytest.raises(_lib.SegmentorError) as e:
            seg.segment_chunks([0], [spec['n']], p['pcount'], p['max_cpg'], p['max_bp'])
        assert e.value.code == code
    # a max_cpg beyond any chunk of the call counts only up to the longest chunk (a window never exceeds its chunk, segmentor.cpp:110)
    a = seg.segment_chunks([0], [spec['n']], 15.0, 70000, 700)[0]
    b = seg.segment_chunks([0], [spec['n']], 15.0, spec['n'], 700)[0]
    assert a.tolist() == b.tolist()
    with pytest.raises(_lib.SegmentorError):
        seg.segment_chunks([spec['n'] - 10], [11], 15.0, 50, 700)           # runs past the file
    with pytest.raises(_lib.SegmentorError):
        seg.segment_chunks([0], [0], 15.0, 50, 700)                          # empty chunk (segment.py:44 asserts)
    # loci going backwards inside a chunk (a chunk crossing chromosomes) are no error: the reference bars the extension and carries on
    # (segmentor.cpp:114-117), and so does the plain path (test_19)
    slices, loci = cases.build_case(spec)
    loci2 = loci.copy()
    loci2[200:] -= loci2[200] - 5
    seg.set_loci(loci2)
    got = seg.segment_chunks([0], [spec['n']], 15.0, 50, 700)[0]
    assert got.tolist() == oracle.segment_chunk(slices, loci2, 15.0, 50, 700).tolist()


def test_12_device_generator_equals_numpy_generator():
    import torch
    S = _lib.load_synth()
    n, N = 100000, 3
    pitch = ((2 * n + 255) // 256) * 256 + 256
    buf = torch.zeros((N, pitch), dtype=torch.uint8, device='cuda:0')
    rc = S.wgbssynth_fill_betas(C.c_void_p(buf.data_ptr()), pitch, n, 0, N, cases.SEED, None)
    assert rc == 0
    host = buf.cpu().numpy()
    for s in range(N):
        want = synth.synth_betas(cases.SEED, s, 0, n).reshape(-1)
        assert _first_diff(host[s, :2 * n], want) is None, 'sample %d: %s' % (s, _first_diff(host[s, :2 * n], want))


# ---------------------------------------------------------------------------------------------------------
# 13. randomised parameters and adversarial inputs against the oracle
# ---------------------------------------------------------------------------------------------------------
def _fuzz_world(rng, n, n_samples):
    """Random loci (dense runs, equal positions, long gaps) and counts (zeros, saturated bytes, meth == cov)."""
    kind = rng.integers(0, 4, n)
    gap = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, 12, n), np.where(kind == 2, rng.integers(2, 300, n), rng.integers(300, 9000, n))))
    loci = (np.cumsum(gap) + 1000).astype(np.uint32)
    slices = []
    for _ in range(n_samples):
        cov = rng.integers(0, 256, n)
        mode = rng.integers(0, 6, n)
        cov = np.where(mode == 0, 0, np.where(mode == 1, 255, cov))
        meth = np.minimum(cov, np.where(mode == 2, cov, np.where(mode == 3, 0, rng.integers(0, 256, n))))
        slices.append(np.stack([meth, cov], axis=1).astype(np.uint8))
    return slices, loci


@pytest.mark.parametrize('seed', range(16))
def test_13_random_parameters_and_adversarial_inputs_match_oracle(seg, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(3000, 9000))
    n_samples = int(rng.choice([1, 2, 3, 7, 33, 40]))
    slices, loci = _fuzz_world(rng, n, n_samples)
    seg.set_betas(slices)
    seg.set_loci(loci)
    for _ in range(4):
        pcount = float(rng.choice([0.0, 0.25, 0.99999994, 1.0, 3.9999998, 15.0, 100.0, 1e-3, 1e-8, 1e30]))     # all three term modes
        max_cpg = int(rng.choice([1, 2, 17, 64, 65, 129, 300, 1000]))
        max_bp = int(rng.choice([1, 2, 50, 700, 2000, 100000]))
        starts, lens = [], []
        for _ in range(12):
            ln = int(rng.integers(1, min(n, 2500)))
            st = int(rng.integers(0, n - ln + 1))
            starts.append(st)
            lens.append(ln)
        got = seg.segment_chunks(starts, lens, pcount, max_cpg, max_bp)
        want = oracle.segment_chunks(slices, loci, starts, lens, pcount, max_cpg, max_bp, threads=os.cpu_count() or 1)
        for c, (a, b) in enumerate(zip(got, want)):
            assert a.tolist() == b.tolist(), 'seed %d pcount %r max_cpg %d max_bp %d chunk [%d,+%d): %s' % (
                seed, pcount, max_cpg, max_bp, starts[c], lens[c], _first_diff(a, b))


@pytest.mark.parametrize('n_samples', [1, 3])
def test_13b_chunk_ending_on_a_carry_boundary_with_a_wide_last_tile(n_samples):
    """Found by tools/extra_fuzz.py (seed 5751): a WIDE scoring tile whose first end site is the chunk's last site wants the prefix
    P[len] alone; when start0 + len is a multiple of 128 (WG_CARRY_G) that position is a carry group of its own, one past the groups the scan
    pass wrote for the chunk.  Needs: len = 1 (mod 16) (a last unit of one start) in a group of start sites that holds a window
    > 60 (or an end tile that begins on the last site: len = 16 m + 129), and the end on a multiple of 128.  The carries are left
    holding another job's numbers first, so a stale entry cannot pass for the right one."""
    rng = np.random.default_rng(77 + n_samples)
    n = 7000
    loci = (np.cumsum(rng.integers(1, 6, n)) + 500).astype(np.uint32)                  # dense: windows are bounded by max_cpg
    slices = []
    for _ in range(n_samples):
        cov = rng.integers(0, 256, n)
        cov[rng.random(n) < 0.3] = 0
        meth = np.minimum(cov, rng.integers(0, 256, n))
        slices.append(np.stack([meth, cov], axis=1).astype(np.uint8))
    chunks = []
    for end in (64 * 20, 64 * 47, 64 * 72, 64 * 100):
        for ln in (1, 17, 65, 129, 193, 145, 16 * 7 + 129, 1345, 1281):
            if ln <= end:
                chunks.append((end - ln, ln))
    with _lib.Segmenter(0) as sg:
        sg.set_betas(slices)
        sg.set_loci(loci)
        for pcount, max_cpg, max_bp in [(3.9999998, 129, 100000), (1.0, 65, 100000), (15.0, 300, 100000), (0.25, 130, 100000), (0.0, 1000, 5000)]:
            sg.segment_chunks([5, 2001, 4099], [1900, 2000, 2500], 100.0, 200, 100000)        # other numbers into the carries
            for st, ln in chunks:                                                           # alone: the chunk's carries end the array
                got = sg.segment_chunks([st], [ln], pcount, max_cpg, max_bp)[0]
                want = oracle.segment_chunks(slices, loci, [st], [ln], pcount, max_cpg, max_bp)[0]
                assert got.tolist() == want.tolist(), 'pcount %r max_cpg %d chunk [%d,+%d): %s' % (pcount, max_cpg, st, ln, _first_diff(got, want))
            sg.segment_chunks([5, 2001, 4099], [1900, 2000, 2500], 100.0, 200, 100000)
            starts = [c[0] for c in chunks]
            lens = [c[1] for c in chunks]
            got = sg.segment_chunks(starts, lens, pcount, max_cpg, max_bp)                      # together: the next chunk's carries follow
            want = oracle.segment_chunks(slices, loci, starts, lens, pcount, max_cpg, max_bp, threads=os.cpu_count() or 1)
            for c, (a, b) in enumerate(zip(got, want)):
                assert a.tolist() == b.tolist(), 'pcount %r max_cpg %d chunk [%d,+%d) of the batch: %s' % (pcount, max_cpg, starts[c], lens[c], _first_diff(a, b))


def test_14_threaded_upload_places_every_byte(monkeypatch):
    """wgbsseg_set_betas_host above 32 MB goes through several threads and page-locked staging pieces: odd row length,
    small pieces, a sample count that does not divide by the threads; every byte must land (checked through the scan)."""
    monkeypatch.setenv('WGBSSEG_UPLOAD_THREADS', '3')
    monkeypatch.setenv('WGBSSEG_UPLOAD_PIECE_KB', '96')
    n = 3_400_001
    slices = [synth.synth_betas(cases.SEED + 1, s, 0, n) for s in range(5)]          # 34 MB
    with _lib.Segmenter(0) as s:
        s.set_betas(slices)
        for start0, length in [(0, 70000), (49152 - 20, 100), (n - 60000, 60000), (1_700_000, 65536)]:
            got = s.prefix_sums(start0, length)
            for k, sl in enumerate(slices):
                want = np.zeros((length + 1, 2), dtype=np.uint32)
                want[1:] = np.cumsum(sl[start0:start0 + length].astype(np.uint32), axis=0)
                assert _first_diff(got[k], want) is None, 'sample %d range [%d,+%d): %s' % (k, start0, length, _first_diff(got[k], want))
        # and whole-row checksums through the block reduction (one block per 1,000,000 sites)
        b = np.arange(0, n + 1, 1_000_000, dtype=np.int64)
        b[-1] = n
        sums = s.block_sums(b[:-1], b[1:], mode=0)
        for k, sl in enumerate(slices):
            want = np.stack([sl[a:e].astype(np.uint64).sum(axis=0) for a, e in zip(b[:-1], b[1:])])
            assert np.array_equal(np.asarray(sums)[k].astype(np.uint64), want), 'sample %d block sums differ' % k


# ---------------------------------------------------------------------------------------------------------
# 15. windows beyond 8000 sites (round 3: the max_cpg cap of rounds 1-2 is gone; VERDICT r02 missing item 1)
# ---------------------------------------------------------------------------------------------------------
def _dense_world(seed, n, n_samples):
    rng = np.random.default_rng(seed)
    loci = (np.cumsum(rng.integers(1, 5, n)) + 777).astype(np.uint32)              # ~2.5 bp apart: 20,000 sites span ~50 kb
    slices = []
    for _ in range(n_samples):
        cov = rng.integers(0, 256, n)
        cov[rng.random(n) < 0.2] = 0
        lvl = np.repeat(rng.random(n // 500 + 1), 500)[:n]
        meth = np.minimum(cov, rng.binomial(cov, lvl))
        slices.append(np.stack([meth, cov], axis=1).astype(np.uint8))
    return slices, loci


@pytest.mark.skipif(not oracle.have_ref(), reason='oracle/_ref/segmentor not built (needs /root/reference at build time)')
def test_15_max_cpg_20000_equals_the_reference_binary():
    """`wgbstools segment --max_cpg 20000 --max_bp 100000` works upstream (segmentor.cpp:92-95 sizes the ring to any max_cpg).
    A 30,000-site dense world, windows of up to 20,000 sites (block totals up to 5.1e6 > 2^21: the wide tiles score with the
    general guarded term form, the narrow ones keep the guard-free one; window pass on loci in L2; recurrence ring of 32,768
    pending steps): borders == the reference binary's, for an integer and a fractional pseudo count."""
    n = 30000
    slices, loci = _dense_world(2026, n, 2)
    with _lib.Segmenter(0) as sg:
        sg.set_betas(slices)
        sg.set_loci(loci)
        for pcount, max_cpg, max_bp in [(15.0, 20000, 100000), (0.5, 12000, 30000)]:
            got = sg.segment_chunks([0], [n], pcount, max_cpg, max_bp)[0]
            tm = sg.timings()
            assert tm['max_window'] > 8224, 'the case must exercise windows whose totals reach 2^21 (widest %d)' % tm['max_window']
            want = oracle.ref_segment_arrays(slices, loci, pcount, max_cpg, max_bp)
            assert got.tolist() == want.tolist(), 'pcount %r max_cpg %d max_bp %d: %s' % (pcount, max_cpg, max_bp, _first_diff(got, want))


def test_15b_windows_between_8000_and_65535_match_the_oracle():
    """The same against the oracle's many-thread restatement, with offsets: a chunk inside a larger world, a second chunk in the same
    call whose windows stay narrow, max_cpg larger than the chunk (counts up to the chunk's length), and the window limit itself
    (65,535 sites: one chunk of 66,000 sites with max_cpg 65,535 is accepted, max_cpg 65,536 on it is refused)."""
    n = 40000
    slices, loci = _dense_world(77, n, 3)
    with _lib.Segmenter(0) as sg:
        sg.set_betas(slices)
        sg.set_loci(loci)
        for pcount, max_cpg, max_bp, st, ln in [(15.0, 9000, 10**6, 1234, 21000), (1.0, 70000, 10**6, 5, 16111), (100.0, 8225, 25000, 20000, 20000)]:
            got = sg.segment_chunks([st, 100], [ln, 700], pcount, max_cpg, max_bp)
            for (a, l), g in zip([(st, ln), (100, 700)], got):
                want = oracle.segment_chunk_mt([s[a:a + l] for s in slices], loci[a:a + l], pcount, min(max_cpg, l), max_bp)
                assert g.tolist() == want.tolist(), 'pcount %r max_cpg %d chunk [%d,+%d): %s' % (pcount, max_cpg, a, l, _first_diff(g, want))
    n = 66000
    rng = np.random.default_rng(5)
    loci = (np.cumsum(rng.integers(50, 150, n)) + 1000).astype(np.uint32)
    slices = [np.stack([np.zeros(n), np.full(n, 3)], axis=1).astype(np.uint8)]
    with _lib.Segmenter(0) as sg:
        sg.set_betas(slices)
        sg.set_loci(loci)
        a = sg.segment_chunks([0], [n], 15.0, 65535, 2000)[0]
        b = sg.segment_chunks([0], [n], 15.0, 1000, 2000)[0]                  # (max_bp 2000 keeps every window ~20 sites: same answer)
        assert a.tolist() == b.tolist()
        with pytest.raises(_lib.SegmentorError) as e:
            sg.segment_chunks([0], [n], 15.0, 65536, 2000)
        assert e.value.code == _lib.E_ARG and '2^24' in str(e.value)


# ---------------------------------------------------------------------------------------------------------
# 16. medium scoring tiles (round 3): units with windows of 61 .. 252 sites, tile-local packed prefixes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_samples,cov_mode', [(1, 'sat'), (3, 'mix'), (40, 'mix')])
def test_16_medium_tiles_match_oracle_and_wide_tiles(monkeypatch, n_samples, cov_mode):
    """Dense worlds whose windows sit on both sides of the class boundaries (60 | 61 and 252 | 253 sites) and of the packed fields'
    capacity: with every count saturated (meth = cov = 255) the prefixes of a 269-entry row run past 2^16 in both fields (carry from
    the #meth into the #cov field, wrap at 2^32) while a block's own counts (<= 252 * 255) still fit — the case the medium tiles'
    difference-of-dwords rests on.  Chunks start off the 8-site vector grid, end inside a unit, and (40 samples) take two LDS sample
    groups.  Borders == oracle, with the medium class on, off (the wide tiles take those units), and cut at 124."""
    slices, loci = cases.medium_tile_world(n_samples, cov_mode)
    chunks = cases.MEDIUM_WORLD_CHUNKS
    starts, lens = [c[0] for c in chunks], [c[1] for c in chunks]
    params = [(15.0, 252), (15.0, 253), (15.0, 61), (1.0, 130), (0.25, 200), (0.0, 252), (7.77, 189), (15.0, 1000)]
    wants = [oracle.segment_chunks(slices, loci, starts, lens, pcount, max_cpg, 10**6, threads=os.cpu_count() or 1) for pcount, max_cpg in params]
    for wm in ('252', '0', '124'):
        monkeypatch.setenv('WGBSSEG_MEDIUM_WMAX', wm)                      # (read when a context is created)
        with _lib.Segmenter(0) as sg:
            sg.set_betas(slices)
            sg.set_loci(loci)
            for (pcount, max_cpg), want in zip(params, wants):
                got = sg.segment_chunks(starts, lens, pcount, max_cpg, 10**6)
                for c, (a, b) in enumerate(zip(got, want)):
                    assert a.tolist() == b.tolist(), 'pcount %r max_cpg %d medium<=%s chunk [%d,+%d): %s' % (pcount, max_cpg, wm, starts[c], lens[c], _first_diff(a, b))
    monkeypatch.delenv('WGBSSEG_MEDIUM_WMAX')


def test_17_lean_step_in_the_narrow_batches_of_a_wide_job(monkeypatch):
    """Round 3: in a job with windows > 64 sites somewhere (32-step batches, a second pending register per lane, the ring), the batches
    whose windows are all <= 60 run a hand-scheduled step in which a finished lane MOVES ON to its second register four steps late.
    Worlds that alternate open sea (windows ~20), islands (windows 61 .. 250: the second register is live when narrow batches
    follow) and very dense stretches (windows > 128: the ring), at chunk offsets that put the batch boundaries on both lane halves;
    borders == oracle, and == the generic step (WGBSSEG_DP_WLEAN=0)."""
    slices, loci = cases.lean_step_world()
    chunks = cases.LEAN_WORLD_CHUNKS
    starts, lens = [c[0] for c in chunks], [c[1] for c in chunks]
    params = cases.LEAN_WORLD_PARAMS
    wants = [oracle.segment_chunks(slices, loci, starts, lens, pcount, max_cpg, max_bp, threads=os.cpu_count() or 1) for pcount, max_cpg, max_bp in params]
    for want in wants:
        assert max(int(w.size) for w in want) > 10
    for wlean in ('1', '0'):
        monkeypatch.setenv('WGBSSEG_DP_WLEAN', wlean)                       # (read when a context is created)
        with _lib.Segmenter(0) as sg:
            sg.set_betas(slices)
            sg.set_loci(loci)
            for (pcount, max_cpg, max_bp), want in zip(params, wants):
                got = sg.segment_chunks(starts, lens, pcount, max_cpg, max_bp)
                if wlean == '1':
                    assert sg.timings()['max_window'] > 64 or max_cpg <= 65, 'the case must be a wide job'
                for c, (a, b) in enumerate(zip(got, want)):
                    assert a.tolist() == b.tolist(), 'pcount %r max_cpg %d max_bp %d lean %s chunk [%d,+%d): %s' % (pcount, max_cpg, max_bp, wlean, starts[c], lens[c], _first_diff(a, b))
    monkeypatch.delenv('WGBSSEG_DP_WLEAN')


# ---------------------------------------------------------------------------------------------------------
# 18. carries of k_scan: staged in LDS for a chunk of up to 512 carry groups, stored directly beyond (round 3)
# ---------------------------------------------------------------------------------------------------------
def test_18_carries_staged_in_lds_and_stored_directly_in_one_batch():
    """k_scan keeps the carries of a row in LDS (512 groups of 128 sites) and writes them when the row is done; a chunk of more groups
    — more than 65,000 sites — stores them from inside its loop.  One batch holds both kinds, at offsets off the vector grid, with
    windows of 300 sites (wide scoring tiles: the consumers of the carries); borders == oracle."""
    slices, loci = cases.carry_world(70400)
    chunks = [(7, 70001), (100, 60000), (0, 65536), (129, 65409), (3, 300)]          # 548, 470, 512, 512 and 3 carry groups
    starts, lens = [c[0] for c in chunks], [c[1] for c in chunks]
    want = oracle.segment_chunks(slices, loci, starts, lens, 15.0, 300, 10**6, threads=os.cpu_count() or 1)
    with _lib.Segmenter(0) as sg:
        sg.set_betas(slices)
        sg.set_loci(loci)
        got = sg.segment_chunks(starts, lens, 15.0, 300, 10**6)
        assert sg.timings()['max_window'] == 300
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.tolist() == b.tolist(), 'chunk [%d,+%d): %s' % (starts[c], lens[c], _first_diff(a, b))


# ------------------------------------------------------------------------------------------------------------
# loci that are not ascending inside a chunk (round 4): segmentor.cpp:114-117 bars the extension and leaves the site out of
# the start's running sums; csrc/plain_dp.h follows the reference's loops as written for such chunks
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden_disorder():
    import json
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'disorder_cases.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', sorted(cases.DISORDER_CASES))
def test_19_non_ascending_loci_match_the_reference(seg, name, golden_disorder):
    g = golden_disorder[name]
    spec = cases.DISORDER_CASES[name]
    slices, loci = cases.build_disorder_case(spec)
    assert cases.case_checksum(slices, loci) == g['input_crc32']
    seg.set_betas(slices)
    seg.set_loci(loci)
    got = seg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])[0]
    assert got.tolist() == g['borders'], _first_diff(got, g['borders'])                # the reference binary's own output
    assert got.tolist() == oracle.segment_chunk(slices, loci, spec['pcount'], spec['max_cpg'], spec['max_bp']).tolist()
    if oracle.have_ref():
        assert got.tolist() == oracle.ref_segment_arrays(slices, loci, spec['pcount'], spec['max_cpg'], spec['max_bp']).tolist()


def test_19b_ordered_and_disordered_chunks_in_one_batch(seg):
    """A batch of chunks inside a resident world, some of them across a place where the positions start again: every chunk as the
    reference computes it, in the caller's order; the ring of the plain path forced to wrap (a deep window on a long chunk)."""
    spec = dict(n=9000, a=20000, samples=[0, 1, 2], pcount=15.0, max_cpg=1000, max_bp=2000)
    slices, loci = cases.build_case(spec)
    loci = loci.astype(np.int64)
    loci[3000:] -= loci[3000] - 7            # a second chromosome from site 3000
    loci[6100:6110] = loci[6100:6110][::-1]  # and a descending run
    loci = loci.astype(np.uint32)
    seg.set_betas(slices)
    seg.set_loci(loci)
    starts = [0, 2500, 3000, 2999, 5000, 6000, 8000, 6105]
    lens = [2500, 1000, 2000, 2, 1000, 300, 1000, 1]
    for pcount, max_cpg, max_bp in [(15.0, 1000, 2000), (0.0, 40, 700), (0.5, 3000, 100000)]:
        got = seg.segment_chunks(starts, lens, pcount, max_cpg, max_bp)
        want = oracle.segment_chunks(slices, loci, starts, lens, pcount, max_cpg, max_bp, threads=4)
        for c, (a, b) in enumerate(zip(got, want)):
            assert a.tolist() == b.tolist(), (pcount, max_cpg, max_bp, starts[c], lens[c], _first_diff(a, b))


@pytest.mark.parametrize('ring_rows', [1, 130, 257, 1000])
def test_19e_plain_path_banded_ring(seg, ring_rows, monkeypatch):
    """The plain path's ring of rows with FEWER rows than the chunk has sites (R < n: bands of R - (W - 1) steps, slot k % R reused across the
    k_plain_rows / k_plain_dp launches) — at the default ~1 GB budget a suite-sized chunk never gets there, so the rows are capped
    through WGBSSEG_PLAIN_RING_ROWS (floored at W by the library: bands of ONE step at ring_rows = 1)."""
    spec = dict(n=2400, a=52000, samples=[0, 1, 2, 3], pcount=15.0, max_cpg=1000, max_bp=2000)
    slices, loci = cases.build_case(spec)
    loci = loci.astype(np.int64)
    loci[1000:] -= loci[1000] - 3            # a second chromosome
    loci[1700:1720] = loci[1700:1720][::-1]  # a descending run
    loci[300] = loci[299]                    # equal positions
    loci = loci.astype(np.uint32)
    seg.set_betas(slices)
    seg.set_loci(loci)
    monkeypatch.setenv('WGBSSEG_PLAIN_RING_ROWS', str(ring_rows))
    for pcount, max_cpg, max_bp in [(15.0, 120, 2000), (0.0, 37, 900), (1.0, 256, 100000)]:
        assert max(ring_rows, max_cpg) < spec['n']            # the ring does wrap
        got = seg.segment_chunks([0, 900], [spec['n'], 1300], pcount, max_cpg, max_bp)
        want = oracle.segment_chunks(slices, loci, [0, 900], [spec['n'], 1300], pcount, max_cpg, max_bp, threads=2)
        for a, b in zip(got, want):
            assert a.tolist() == b.tolist(), (ring_rows, pcount, max_cpg, max_bp, _first_diff(a, b))


def test_19c_invalid_counts_in_a_disordered_chunk(seg):
    spec = cases.DISORDER_CASES['two_chromosomes']
    slices, loci = cases.build_disorder_case(spec)
    slices = [s.copy() for s in slices]
    slices[1][700] = (9, 3)
    seg.set_betas(slices)
    seg.set_loci(loci)
    with pytest.raises(_lib.SegmentorError) as e:
        seg.segment_chunks([0], [spec['n']], spec['pcount'], spec['max_cpg'], spec['max_bp'])
    assert e.value.code == _lib.E_METH_GT_COV


def test_19d_whole_region_call_over_a_genome_with_disordered_loci(seg):
    """wgbsseg_segment_regions (chunk grid + junction patches + the tree, one native call) over ONE region whose loci start again in
    the middle and hold a descending run: chunks and patches that touch those places take the plain path inside the same batches as the
    others; the merged borders equal the reference's pairwise tree (tests/reftree.py) walked over the ORACLE's chunk DPs."""
    import reftree
    spec = dict(n=9000, a=30000, samples=[0, 1, 2], pcount=15.0, max_cpg=1000, max_bp=2000)
    slices, loci = cases.build_case(spec)
    loci = loci.astype(np.int64)
    loci[3000:] -= loci[3000] - 7            # exactly on a chunk boundary of the 1500-site grid: the junction patch straddles it
    loci[4400:4440] = loci[4400:4440][::-1]  # inside a chunk
    loci[7499:7502] = loci[7499:7502][::-1]  # across a chunk boundary
    loci = loci.astype(np.uint32)
    seg.set_betas(slices)
    seg.set_loci(loci)
    n = spec['n']
    for chunk in (1500, 4000):
        got, stats = seg.segment_regions(np.array([1]), np.array([n + 1]), chunk, spec['pcount'], spec['max_cpg'], spec['max_bp'])

        def many(sites):                     # 1-based half-open site ranges -> absolute border lists, as segment_process returns them
            return [oracle.segment_chunk([s[a - 1:b - 1] for s in slices], loci[a - 1:b - 1], spec['pcount'], spec['max_cpg'], spec['max_bp']).astype(np.int64) + a
                    for a, b in sites]
        grid = [(s, min(s + chunk, n + 1)) for s in range(1, n + 1, chunk)]
        want = reftree.tree(many(grid), many)
        assert np.array_equal(np.asarray(got[0], dtype=np.int64), want), (chunk, _first_diff(got[0], want))
