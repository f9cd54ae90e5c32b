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


# ---------------------------------------------------------------------------------------------------------
# e. the recurrence builds, the lean step, staging
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stages', [None, 2, 3, 7])
@pytest.mark.parametrize('wlean', [1, 0])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_e_recurrence_builds(worlds, mode, wlean, stages):
    """Back-pointers (and the windows they rest on) under WGBSSEG_DP_MODE 0 / 1 / 2 (64-step batches; 32-step batches with a second pending
    register and the ring; the same with 15 worker waves), with the lean step on and off, in the launcher's own staging and in 2, 3 and 7
    stages (k_dp16 in every stage but the last when the mode is 0): windows > 64, islands in open sea, windows of thousands of sites, and the
    six chunks of test_17's world with its first two parameter sets."""
    label = 'dp mode %d, lean %d, stages %r' % (mode, wlean, stages)
    with _segmenter(DP_MODE=mode, DP_WLEAN=wlean, FORCE_STAGES=stages) as sg:
        for name in ('dense_w_gt_64', 'island_mix', 'deep'):
            t = _run(sg, _golden_case(worlds, name), ('window', 'cum', 'back'), '%s, %s' % (name, label))
            if stages:
                assert t['n_stages'] == stages
        for q in (0, 1):
            t = _run(sg, _lean_world(worlds, q), ('window', 'cum', 'back'), 'lean-step world %r, %s' % (cases.LEAN_WORLD_PARAMS[q], label))
            assert t['max_window'] > 64
            if stages:
                assert t['n_stages'] == stages
                with pytest.raises(_lib.SegmentorError) as e:          # the scored blocks of a staged job share their buffers: refused
                    sg.debug_fetch('cost', np.float64, 16)
                assert e.value.code == _lib.E_STATE


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
    for w in ALL:
        got, want = im.fetch(seg1, w, exp), np.concatenate(alone[w])
        assert got.dtype == want.dtype and np.array_equal(got, want), '%s: %s' % (w, im._first_diff(got, want))
    # a buffer that is too small is refused, not cut
    with pytest.raises(_lib.SegmentorError) as e:
        seg1.debug_fetch('window', np.uint16, sum(c[1] for c in chunks) - 1)
    assert e.value.code == _lib.E_CAPACITY
