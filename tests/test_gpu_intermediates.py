"""Scored blocks (k_cost) and back-pointers (k_dp, k_dp16) bit for bit against the oracle, in every form the kernels take:
every golden case, every narrow tile shape and both division cores, the medium | wide class boundaries in many-chunk batches,
wide tiles fed by k_scan's carries, the three recurrence builds with the lean step and staging — and the fetch hook itself.

Every assertion is exact equality (fp64 bit patterns for the scored blocks).  A failure names the kernel output, the form, the
chunk, the start site and the end site (tests/intermediates.py), not a moved border.  Not compared here, borders only:
`default_chunk` and `deep_long` (the oracle's debug band is ~480 MB for each) and the full-size runs of test_gpu_fullsize.py.
"""
import contextlib
import os

import numpy as np
import pytest

import cases
import intermediates as im
import staging
from wgbs_tools_amd import _lib

pytestmark = pytest.mark.gpu

ALL = ('window', 'cum', 'cost', 'back')

# the oracle's [n, max_cpg] debug band of these two is ~480 MB each; island_mix (160 MB) is the largest that stays
LEFT_OUT = ('default_chunk', 'deep_long')
EVERY_CASE = [name for name in cases.CHUNK_CASES if name not in LEFT_OUT]


@contextlib.contextmanager
def _segmenter(**env):
    """A context created under WGBSSEG_<KEY>=value switches (they are read when a context is created)."""
    keys = {'WGBSSEG_' + k: str(v) for k, v in env.items() if v is not None}
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    try:
        sg = _lib.Segmenter(0)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    try:
        yield sg
    finally:
        sg.close()


@pytest.fixture(scope='module')
def seg1():
    """one-stage jobs: the scored blocks of the whole call stay in one buffer"""
    with _segmenter(FORCE_STAGES=1) as sg:
        yield sg


@pytest.fixture(scope='module')
def worlds():
    """name -> (slices, loci, chunks, params, [Expected]): the oracle's values once per world and parameter set, shared by the tests"""
    cache = {}

    def get(name, build):
        if name not in cache:
            slices, loci, chunks, params = build()
            cache[name] = (slices, loci, chunks, params, im.expected(slices, loci, chunks, *params))
        return cache[name]
    yield get
    cache.clear()


def _golden_case(worlds, name):
    def build():
        spec = cases.CHUNK_CASES[name]
        slices, loci = cases.build_case(spec)
        return slices, loci, [(0, spec['n'])], (spec['pcount'], spec['max_cpg'], spec['max_bp'])
    return worlds(name, build)


def _lean_world(worlds, q):
    def build():
        slices, loci = cases.lean_step_world()
        return slices, loci, cases.LEAN_WORLD_CHUNKS, cases.LEAN_WORLD_PARAMS[q]
    return worlds('lean_step_world/%d' % q, build)


def _run(sg, world, whats, label):
    slices, loci, chunks, params, exp = world
    sg.set_betas(slices)
    sg.set_loci(loci)
    got = sg.segment_chunks([c[0] for c in chunks], [c[1] for c in chunks], *params)
    im.check_call(sg, exp, got, whats, label)
    return sg.timings()


def _form(sg, world, label='', **claims):
    """the last call's plan against the form the test claims (staging.assert_form) -> plan"""
    return staging.assert_form(sg.last_plan(), max(c[1] for c in world[2]), label=label, **claims)


# ---------------------------------------------------------------------------------------------------------
# a. every case, the launcher's own choice of form
# ---------------------------------------------------------------------------------------------------------
def test_a0_the_cases_left_out_are_named():
    assert LEFT_OUT == ('default_chunk', 'deep_long') and all(name in cases.CHUNK_CASES for name in LEFT_OUT)
    assert sorted(EVERY_CASE + list(LEFT_OUT)) == sorted(cases.CHUNK_CASES) and len(EVERY_CASE) == len(cases.CHUNK_CASES) - 2


@pytest.mark.parametrize('name', EVERY_CASE)
def test_a_every_case_default_form(seg1, worlds, golden_chunks, name):
    """Window extents, row offsets, scored blocks and back-pointers of every golden case but the two of LEFT_OUT: more than 4 samples
    (2 to 16 LDS sample groups), all three term modes, saturated / zero / single samples.  One context serves all cases, so each finds
    the previous one's numbers in the buffers."""
    world = _golden_case(worlds, name)
    t = _run(seg1, world, ALL, name)
    assert t['n_stages'] == 1
    _form(seg1, world, name, stages=1, gated=0, dp_mode=staging.auto_dp_mode(t['max_window']))
    assert world[4][0].borders.tolist() == golden_chunks[name]['borders']


# ---------------------------------------------------------------------------------------------------------
# b. every narrow tile shape, both division cores
# ---------------------------------------------------------------------------------------------------------
SHAPE_CASES = ['tiny', 'pcount0', 'pcount_half', 'saturated', 'zero_stretch', 'n33_samples', 'n200_samples', 'n512_samples']


@pytest.mark.parametrize('ti,ns,div_short', [(128, 0, None), (64, 0, None), (32, 0, None), (16, 0, None), (64, 4, None), (32, 8, None), (0, 0, 0)])
def test_b_narrow_tile_shapes_and_division_cores(worlds, ti, ns, div_short):
    """The six (TI, NS) settings of test_07d, and WGBSSEG_DIV_SHORT=0 (the 8-instruction core in the launcher's own shape): the scored blocks
    of cases with 3 to 512 samples, all three term modes, saturated counts and zero stretches.  A shape that does not fit a case's LDS budget
    falls back inside the launcher (plan_tiles: 128 start sites need every sample in one LDS group, so the 200- and 512-sample cases cannot
    take them).  wgbsseg_timings has NO field for the tile shape that ran, so which ones fell back cannot be read here; what it does report —
    whether the short division core was in use — is printed per case."""
    with _segmenter(FORCE_STAGES=1, TI=ti or None, NS=ns or None, DIV_SHORT=div_short) as sg:
        for name in SHAPE_CASES:
            t = _run(sg, _golden_case(worlds, name), ('cost', 'back'), '%s, TI %d NS %d DIV_SHORT %r' % (name, ti, ns, div_short))
            print('%s TI %d NS %d: short division core %s, widest window %d' % (name, ti, ns, 'on' if t['div_short'] else 'off', t['max_window']))
            assert t['n_stages'] == 1
            _form(sg, _golden_case(worlds, name), name, stages=1, gated=0)
            if div_short == 0:
                assert t['div_short'] == 0


# ---------------------------------------------------------------------------------------------------------
# c. class boundaries (60 | 61 and 252 | 253 sites) in a batch of seven chunks
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pcount,max_cpg', [(15.0, 252), (15.0, 253), (15.0, 61), (0.0, 252), (15.0, 60)])
@pytest.mark.parametrize('n_samples,cov_mode', [(1, 'sat'), (3, 'mix'), (40, 'mix')])
def test_c_class_boundaries_in_one_batch(worlds, n_samples, cov_mode, pcount, max_cpg):
    """test_16's world (saturated counts: the packed prefixes of a medium tile's row carry from the #meth into the #cov field; 40 samples: two
    LDS sample groups), its seven chunks off the vector grid in ONE batch, windows on both sides of the narrow | medium | wide boundaries, with
    the medium class on, off and cut at 124: scored blocks and back-pointers of every chunk.  The oracle runs once per parameter set."""
    def build():
        slices, loci = cases.medium_tile_world(n_samples, cov_mode)
        return slices, loci, cases.MEDIUM_WORLD_CHUNKS, (pcount, max_cpg, 10**6)
    world = worlds('medium_tile_world/%d/%s/%r/%d' % (n_samples, cov_mode, pcount, max_cpg), build)
    assert max(int(e.W.max()) for e in world[4]) == max_cpg
    for wm in ('252', '0', '124'):
        with _segmenter(FORCE_STAGES=1, MEDIUM_WMAX=wm) as sg:
            t = _run(sg, world, ALL, '%d samples (%s), pcount %r max_cpg %d, medium <= %s' % (n_samples, cov_mode, pcount, max_cpg, wm))
            assert t['max_window'] == max_cpg and t['n_stages'] == 1
            assert _form(sg, world, 'medium <= %s' % wm, stages=1, gated=0)['all_narrow'] == (max_cpg <= 60)


# ---------------------------------------------------------------------------------------------------------
# d. wide tiles on the carries of k_scan
# ---------------------------------------------------------------------------------------------------------
def test_d_wide_tiles_on_carries(seg1, worlds):
    """A cut-down form of test_18's world (20,000 sites; the 512-group LDS limit stays with test_18): windows of 300 sites — wide tiles, the
    consumers of the carries — in chunks that start at sites 3, 7 and 129, cross 1 to 71 carry groups (128 absolute sites each) and end on,
    before and after a group boundary, in one batch; another job's numbers are left in the carries first."""
    def build():
        slices, loci = cases.carry_world(20000)
        chunks = [(7, 9001), (100, 6000), (0, 4096), (129, 8063), (3, 300), (129, 127), (12000, 8000)]
        return slices, loci, chunks, (15.0, 300, 10**6)
    world = worlds('carry_world', build)
    seg1.set_betas(world[0])
    seg1.set_loci(world[1])
    seg1.segment_chunks([5, 2001, 4099], [1900, 2000, 2500], 100.0, 200, 10**6)
    t = _run(seg1, world, ALL, 'carry world')
    assert t['max_window'] == 300 and t['n_stages'] == 1
    plan = _form(seg1, world, 'carry world', stages=1, gated=0, dp_mode=1)
    assert all(row[1] > 0 for row in plan['stage_tiles'])          # wide tiles, the consumers of the carries


# ---------------------------------------------------------------------------------------------------------
# e. the recurrence builds, the lean step, staging
# ---------------------------------------------------------------------------------------------------------
# the gate axis: WGBSSEG_STAGE_GATE=0 (no gate: every stage's scoring on one stream), and the gate lifted over the one-context rule
# (WGBSSEG_STAGE_GATE_SHARED=1: this module's `seg1` is alive beside every context made here) with a slack of 1 tile (a stage waits for all
# tiles of the stage before but one) and of 4096 (more than any stage here has: the count to wait for clamps to 1, the gate opens at once
# and neighbouring stages overlap as much as they can)
GATES = {'off': dict(STAGE_GATE=0), 'slack1': dict(STAGE_GATE=1, STAGE_GATE_SHARED=1), 'slack4096': dict(STAGE_GATE=4096, STAGE_GATE_SHARED=1)}

# chunk lengths of 1 (mod 64), the longest not first.  The stage bounds of a 1025-site job are 576 (two equal stages), 320 (two stages, the
# last of 300 percent), 384 / 768, 448 / 896 and 256 / 512 (three stages, the last of 100, 40 and 300 percent): for every bound b a chunk of
# b + 1 sites, whose last stage is ONE start site and whose last site the bound falls on; 65 and 1 end before any second stage begins.
STAGED_LENGTHS = [577, 1025, 65, 257, 321, 385, 449, 513, 769, 897, 1]
STAGED_WORLDS = {
    # no window beyond the narrow tiles' 60 sites (open sea of ~20, islands cut at 60): the host's own tile counts, k_dp16 in the early stages
    'narrow': (lambda: cases.lean_step_world(), [37, 4131, 123, 9001, 14003, 2005, 15001, 300, 7777, 11111, 19998], (15.0, 60, 2000)),
    # test_c's world on the wide side of the 252 | 253 boundary with 40 samples (two LDS sample groups): wide tiles, medium and narrow ones towards every chunk's end
    'classes': (lambda: cases.medium_tile_world(40, 'mix'), [3, 1999, 8737, 4103, 5, 2005, 6001, 7003, 101, 8000, 8999], (15.0, 253, 10**6)),
    # test_d's world: windows of 300 sites, wide tiles on k_scan's carries, chunks on and off the 128-site carry groups
    'carries': (lambda: cases.carry_world(20000), [7, 129, 3, 12000, 100, 4097, 8063, 16001, 2049, 5555, 19999], (15.0, 300, 10**6)),
}


def _staged_world(worlds, name):
    def build():
        make, starts, params = STAGED_WORLDS[name]
        slices, loci = make()
        return slices, loci, list(zip(starts, STAGED_LENGTHS)), params
    return worlds('staged/' + name, build)


def _default_last_pct(world):
    """the last stage's length a gated job gets without WGBSSEG_LAST_STAGE_PCT (plan_stages): 300 percent up to 52,500 evaluations per step"""
    pairs = sum(e.cost.size for e in world[4])
    return 300 if float(pairs) * len(world[0]) / max(1.0, float(max(c[1] for c in world[2]))) <= 52500.0 else 100


def _check_staged(sg, world, label, stages, gate, mode=None):
    """One call on `world` under forced stages and a gate setting: windows, cum and back-pointers of every chunk, the scored blocks whenever
    every stage kept its buffer (refused otherwise), and the form that ran."""
    gated = int(bool(stages) and stages > 1 and 'STAGE_GATE_SHARED' in GATES[gate])
    t = _run(sg, world, ('window', 'cum', 'back'), label)
    plan = _form(sg, world, label, stages=stages, gated=gated, last_pct=_default_last_pct(world) if gated else 100,
                 dp_mode=None if mode is None else max(mode, staging.auto_dp_mode(t['max_window'])))
    assert plan['n_stages'] == t['n_stages'] and plan['nbuf'] == (1 if plan['n_stages'] == 1 else 3 if gated and plan['n_stages'] > 2 else 2), (label, plan)
    assert plan['dp16'] == [int(plan['dp_mode'] == 0 and s + 1 < plan['n_stages']) for s in range(plan['n_stages'])], (label, plan)
    if plan['n_stages'] <= plan['nbuf']:
        im.check_call(sg, world[4], [e.borders for e in world[4]], ('cost',), label)
    else:
        with pytest.raises(_lib.SegmentorError) as e:              # a later stage has scored into an earlier one's buffer: refused
            sg.debug_fetch('cost', np.float64, 16)
        assert e.value.code == _lib.E_STATE
    return t, plan


@pytest.mark.parametrize('stages', [None, 2, 3, 7])
@pytest.mark.parametrize('wlean', [1, 0])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_e_recurrence_builds(worlds, mode, wlean, stages):
    """Back-pointers (and the windows they rest on) under WGBSSEG_DP_MODE 0 / 1 / 2 (64-step batches; 32-step batches with a second pending
    register and the ring; the same with 15 worker waves), with the lean step on and off, in the launcher's own staging and in 2, 3 and 7
    stages: windows > 64, islands in open sea, windows of thousands of sites, and the six chunks of test_17's world with its first two
    parameter sets.  This is the UNGATED value of the gate axis (WGBSSEG_STAGE_GATE=0; test_e_gated_recurrence_builds has the other two):
    without the switch the form would hang on how many other contexts are alive.  last_plan() shows that a world with a window > 64 never
    runs k_dp16, whatever the mode asked for (the launcher only raises it): the all-narrow world of STAGED_WORLDS is here for that kernel."""
    label = 'dp mode %d, lean %d, stages %r, ungated' % (mode, wlean, stages)
    with _segmenter(DP_MODE=mode, DP_WLEAN=wlean, FORCE_STAGES=stages, **GATES['off']) as sg:
        for name in ('dense_w_gt_64', 'island_mix', 'deep'):
            world = _golden_case(worlds, name)
            t = _run(sg, world, ('window', 'cum', 'back'), '%s, %s' % (name, label))
            plan = _form(sg, world, '%s, %s' % (name, label), stages=stages, gated=0, dp_mode=max(mode, staging.auto_dp_mode(t['max_window'])))
            assert plan['dp16'] == [0] * plan['n_stages']
            if stages:
                assert t['n_stages'] == stages
        for q in (0, 1):
            t, plan = _check_staged(sg, _lean_world(worlds, q), 'lean-step world %r, %s' % (cases.LEAN_WORLD_PARAMS[q], label), stages, 'off', mode)
            assert t['max_window'] > 64
            if stages:
                assert t['n_stages'] == stages
        if stages:
            t, plan = _check_staged(sg, _staged_world(worlds, 'narrow'), 'all-narrow world, ' + label, stages, 'off', mode)
            assert plan['all_narrow'] == 1 and plan['dp_mode'] == mode and plan['gated'] == 0


@pytest.mark.parametrize('stages', [2, 3, 7])
@pytest.mark.parametrize('wlean', [1, 0])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('gate', ['slack1', 'slack4096'])
def test_e_gated_recurrence_builds(worlds, gate, mode, wlean, stages):
    """The gated values of test_e's gate axis, every form of it (2, 3 and 7 stages, the three recurrence builds, the lean step on and off): the
    stages alternate between the two scoring streams behind k_stage_gate, a third scored-block buffer from three stages on, a last stage of
    300 percent.  Pruned by WORLD: the many-chunk batches, where stages have narrow and wide tiles side by side (test_17's six chunks, both
    parameter sets), one single chunk with windows > 64, and the all-narrow world (k_dp16 in every stage but the last in mode 0); island_mix
    and deep stay with the ungated value.  Windows, cum and back-pointers of every chunk; the scored blocks too where the buffers survive
    (2 stages, 3 gated stages)."""
    label = 'dp mode %d, lean %d, stages %d, gate %s' % (mode, wlean, stages, gate)
    with _segmenter(DP_MODE=mode, DP_WLEAN=wlean, FORCE_STAGES=stages, **GATES[gate]) as sg:
        _check_staged(sg, _golden_case(worlds, 'dense_w_gt_64'), 'dense_w_gt_64, ' + label, stages, gate, mode)
        for q in (0, 1):
            t, plan = _check_staged(sg, _lean_world(worlds, q), 'lean-step world %r, %s' % (cases.LEAN_WORLD_PARAMS[q], label), stages, gate, mode)
            assert t['n_stages'] == stages and plan['gated'] == 1 and plan['nbuf'] == (3 if stages > 2 else 2)
        t, plan = _check_staged(sg, _staged_world(worlds, 'narrow'), 'all-narrow world, ' + label, stages, gate, mode)
        assert plan['all_narrow'] == 1 and plan['gated'] == 1 and plan['dp16'] == [int(mode == 0)] * (plan['n_stages'] - 1) + [0]


# ---------------------------------------------------------------------------------------------------------
# chunks inside a larger world, on the kernels' boundaries (the offset cases of test_06b), in one batch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.OFFSET_CASES))
def test_e2_chunks_on_carry_unit_and_tile_boundaries(seg1, worlds, golden_offsets, name):
    """Chunks that end on and next to every 128th absolute site (k_scan's carries) with lengths of 1 (mod 16) and 1 (mod 64) (a last unit / tile
    of one start), tens of them in one batch: everything the device holds for each, not only its borders."""
    def build():
        spec = cases.OFFSET_CASES[name]
        slices, loci = cases.build_case(spec)
        return slices, loci, cases.offset_chunks(spec), (spec['pcount'], spec['max_cpg'], spec['max_bp'])
    world = worlds('offset/' + name, build)
    assert [list(c) for c in world[2]] == [list(c) for c in golden_offsets[name]['chunks']]
    _run(seg1, world, ALL, name)
    _form(seg1, world, name, stages=1, gated=0)
    for e, want in zip(world[4], golden_offsets[name]['borders']):
        assert e.borders.tolist() == want


# ---------------------------------------------------------------------------------------------------------
# f. the hook
# ---------------------------------------------------------------------------------------------------------
def test_f_dense_fetch_of_a_batch_equals_the_chunks_fetched_alone(seg1, worlds):
    """Chunks of 1, 7, 9, 1025 and 300 sites at odd offsets (none a multiple of the 8 entries the library pads its arrays to): the dense
    window / cum / back / cost of the batch are the concatenation of the same chunks fetched one job at a time — and the oracle's."""
    def build():
        slices, loci = cases.medium_tile_world(3, 'mix')
        return slices, loci, [(3, 1), (11, 7), (101, 9), (777, 1025), (2501, 300)], (15.0, 100, 10**6)
    world = worlds('hook', build)
    slices, loci, chunks, params, exp = world
    seg1.set_betas(slices)
    seg1.set_loci(loci)
    alone = {w: [] for w in ALL}
    for (a, l), e in zip(chunks, exp):
        b = seg1.segment_chunks([a], [l], *params)
        im.check_call(seg1, [e], b, ALL, 'chunk [%d,+%d) alone' % (a, l))
        for w in ALL:
            alone[w].append(im.fetch(seg1, w, [e]))
    _run(seg1, world, ALL, 'the batch')
    assert _form(seg1, world, 'the batch', stages=1, gated=0)['n_chunks'] == len(chunks)
    for w in ALL:
        got, want = im.fetch(seg1, w, exp), np.concatenate(alone[w])
        assert got.dtype == want.dtype and np.array_equal(got, want), '%s: %s' % (w, im._first_diff(got, want))
    # a buffer that is too small is refused, not cut
    with pytest.raises(_lib.SegmentorError) as e:
        seg1.debug_fetch('window', np.uint16, sum(c[1] for c in chunks) - 1)
    assert e.value.code == _lib.E_CAPACITY


# ---------------------------------------------------------------------------------------------------------
# g. the scored blocks of staged calls: every stage's tile plan, the three scored-block buffers, the gate's streams
# ---------------------------------------------------------------------------------------------------------
STAGED_FORMS = {
    '2 ungated':        (2, 'off', None),
    '2 gated':          (2, 'slack1', None),            # (the launcher's own last stage: _default_last_pct)
    '3 gated, last 40': (3, 'slack1', 40),
    '3 gated, last 100': (3, 'slack4096', 100),
    '3 gated, last 300': (3, 'slack1', 300),
}


@pytest.mark.parametrize('form', list(STAGED_FORMS))
@pytest.mark.parametrize('name', list(STAGED_WORLDS))
def test_g_staged_scored_blocks(worlds, name, form):
    """k_cost's output under staging, bit for bit: the tiles are cut at the stage bounds (k_tile_count, k_stage_plan, k_tile_emit per stage),
    stage s scores into buffer s % nbuf, and "cost" puts the rows together again.  Eleven chunks of 1 (mod 64) sites in one batch (STAGED_LENGTHS:
    a last stage of one start site for every bound of every form, two chunks that end before the second stage begins), on an all-narrow
    world, on test_c's world with the three tile classes and two LDS sample groups, and on test_d's wide tiles fed by the carries.  Each call
    runs twice on its context and once more behind a job of another shape: no counter, third buffer or event of an earlier call may show."""
    stages, gate, pct = STAGED_FORMS[form]
    world = _staged_world(worlds, name)
    lengths = [c[1] for c in world[2]]
    assert all(l % 64 == 1 for l in lengths) and max(lengths) != lengths[0]
    gated = int(gate != 'off')
    want_pct = pct if pct is not None else (_default_last_pct(world) if gated else 100)
    with _segmenter(FORCE_STAGES=stages, LAST_STAGE_PCT=pct, **GATES[gate]) as sg:
        for visit in ('first call', 'second call', 'after a job of another shape'):
            if visit == 'after a job of another shape':
                sg.segment_chunks([5, 2001, 4099], [1900, 2000, 2500], 100.0, 200, 10**6)
                assert sg.last_plan()['bounds'] != staging.expected_bounds(1025, stages, want_pct)
            label = '%s world, %s, %s' % (name, form, visit)
            t = _run(sg, world, ('window', 'cum', 'back'), label)
            plan = _form(sg, world, label, stages=stages, gated=gated, last_pct=want_pct, dp_mode=staging.auto_dp_mode(t['max_window']))
            im.check_call(sg, world[4], [e.borders for e in world[4]], ('cost',), label)      # (after the form: three UNGATED stages would have no "cost")
            assert plan['n_stages'] == stages and plan['nbuf'] == (3 if gated and stages == 3 else 2) and plan['n_chunks'] == len(lengths), (label, plan)
            assert plan['all_narrow'] == (name == 'narrow') and plan['dp16'] == [int(name == 'narrow')] * (stages - 1) + [0], (label, plan)
            for b in plan['bounds'][1:-1]:                     # a chunk whose last stage is the one start site at the bound, chunks with nothing behind it
                assert b + 1 in lengths and min(lengths) < b, (label, plan)
            if name != 'narrow':                               # wide tiles (and, on test_c's world, medium ones) beside the narrow ones
                tiles = np.asarray(plan['stage_tiles']).sum(axis=0)
                assert tiles[0] > 0 and tiles[1] > 0 and (name != 'classes' or tiles[2] > 0), (label, plan)


# ---------------------------------------------------------------------------------------------------------
# h. the hooks on staged calls
# ---------------------------------------------------------------------------------------------------------
def test_h_last_plan_needs_a_finished_call(worlds):
    """last_plan() before any call, and after set_betas (which invalidates what the last call left), is WGBSSEG_E_STATE; so is "cost" after a
    call of seven stages, whose later stages have overwritten the earlier ones' blocks."""
    world = _staged_world(worlds, 'narrow')
    with _segmenter(FORCE_STAGES=7, **GATES['slack1']) as sg:
        with pytest.raises(_lib.SegmentorError) as e:
            sg.last_plan()
        assert e.value.code == _lib.E_STATE
        _run(sg, world, ('window', 'cum', 'back'), 'seven stages')
        plan = _form(sg, world, 'seven stages', stages=7, gated=1, last_pct=_default_last_pct(world), dp_mode=0)
        assert plan['n_stages'] > plan['nbuf'] == 3
        with pytest.raises(_lib.SegmentorError) as e:
            sg.debug_fetch('cost', np.float64, sum(x.cost.size for x in world[4]))
        assert e.value.code == _lib.E_STATE
        sg.set_betas(world[0])
        with pytest.raises(_lib.SegmentorError) as e:
            sg.last_plan()
        assert e.value.code == _lib.E_STATE


@pytest.mark.parametrize('gate', ['off', 'slack1'])
def test_h_dense_cost_of_a_staged_batch_equals_the_chunks_fetched_alone(seg1, worlds, gate):
    """test_f's property for a two-stage batch: chunks of 1, 7, 9, 1025 and 300 sites at odd offsets — the dense "cost" (and window / cum / back)
    of the staged batch is the concatenation of the same chunks fetched from one-stage calls of one chunk each."""
    def build():
        slices, loci = cases.medium_tile_world(3, 'mix')
        return slices, loci, [(3, 1), (11, 7), (101, 9), (777, 1025), (2501, 300)], (15.0, 100, 10**6)
    world = worlds('hook', build)
    slices, loci, chunks, params, exp = world
    seg1.set_betas(slices)
    seg1.set_loci(loci)
    alone = {w: [] for w in ALL}
    for (a, l), e in zip(chunks, exp):
        seg1.segment_chunks([a], [l], *params)
        assert seg1.last_plan()['n_stages'] == 1
        for w in ALL:
            alone[w].append(im.fetch(seg1, w, [e]))
    with _segmenter(FORCE_STAGES=2, **GATES[gate]) as sg:
        _run(sg, world, ALL, 'the batch in two stages')
        plan = _form(sg, world, 'the batch in two stages', stages=2, gated=int(gate != 'off'), dp_mode=1)
        assert plan['n_stages'] == 2 and plan['n_chunks'] == len(chunks)
        for w in ALL:
            got, want = im.fetch(sg, w, exp), np.concatenate(alone[w])
            assert got.dtype == want.dtype and np.array_equal(got, want), '%s: %s' % (w, im._first_diff(got, want))
        with pytest.raises(_lib.SegmentorError) as e:              # a buffer that is too small is refused, not cut
            sg.debug_fetch('cost', np.float64, sum(x.cost.size for x in exp) - 1)
        assert e.value.code == _lib.E_CAPACITY
