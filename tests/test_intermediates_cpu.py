"""The comparison of tests/intermediates.py is not blind: on `tiny`, a fault planted in the dense arrays a device call would
return makes it fail and name the right cell; and the dense-layout bookkeeping holds for chunk lengths on both sides of the
8-entry grid the library pads its own arrays to."""
import numpy as np
import pytest

import cases
import intermediates as im

TWO_CHUNKS = [(0, 150), (143, 257)]          # (the second off the 8-site grid, overlapping the first)


@pytest.fixture(scope='module')
def tiny():
    spec = cases.CHUNK_CASES['tiny']
    slices, loci = cases.build_case(spec)
    one = im.expected(slices, loci, [(0, spec['n'])], spec['pcount'], spec['max_cpg'], spec['max_bp'])
    two = im.expected(slices, loci, TWO_CHUNKS, spec['pcount'], spec['max_cpg'], spec['max_bp'])
    return spec, slices, loci, one, two


def _cell_by_walking(exp, j):
    """(chunk, start, end) of dense cost entry j, by walking the rows one by one (independent of im.locate_cost)"""
    at = 0
    for c, e in enumerate(exp):
        for k in range(e.length):
            w = int(e.W[k])
            if j < at + w:
                return c, k, k + (j - at)
            at += w
    raise IndexError(j)


def test_expectation_is_the_oracle_per_chunk(tiny):
    spec, slices, loci, one, two = tiny
    from oracle import oracle
    e = one[0]
    n = spec['n']
    assert e.W.size == n and e.cum[0] == 0 and e.cost.size == int(e.W.sum()) and e.back.size == n
    assert np.array_equal(e.cum[1:], np.cumsum(e.W)[:-1])
    b, M, T, band = oracle.segment_chunk(slices, loci, spec['pcount'], spec['max_cpg'], spec['max_bp'], debug=True)
    assert e.borders.tolist() == b.tolist()
    for k in (0, 1, 57, n - 2, n - 1):                       # rows are start-major: row k = band[k, :F_k]
        row = e.cost[e.cum[k]:e.cum[k] + e.W[k]]
        assert np.array_equal(row, band[k, :e.W[k]].view(np.uint64))
    assert np.all(e.back >= 1) and np.all(e.back <= np.arange(1, n + 1))
    # the back-pointers walk to the oracle's borders
    i, walk = n, [n]
    while i > 0:
        i -= int(e.back[i - 1])
        walk.append(i)
    assert walk[::-1] == b.tolist()
    # a chunk inside the world is scored on its own slice: cum starts again at 0, the windows end with the chunk
    for e2, (a, l) in zip(two, TWO_CHUNKS):
        assert (e2.start0, e2.length) == (a, l) and e2.cum[0] == 0 and e2.W[-1] == 1
        alone = oracle.segment_chunk([s[a:a + l] for s in slices], loci[a:a + l], spec['pcount'], spec['max_cpg'], spec['max_bp'])
        assert e2.borders.tolist() == alone.tolist()
    assert im.diff_cost(im.dense(two, 'cost'), two) is None
    assert all(im.diff_sites(w, im.dense(two, w), two) is None for w in ('window', 'cum', 'back'))


def test_last_mantissa_bit_of_one_cost_cell(tiny):
    _, _, _, one, two = tiny
    for exp in (one, two):
        want = im.dense(exp, 'cost')
        for j in (0, 1234, want.size // 2 + 3, want.size - 1):
            got = want.copy()
            got[j] ^= np.uint64(1)
            m = im.diff_cost(got, exp)
            assert m is not None and m.count == 1 and (m.chunk, m.start, m.end) == _cell_by_walking(exp, j)
            assert m.got == int(got[j]) and m.want == int(want[j]) and m.got ^ m.want == 1
            m2 = im.diff_cost(got.view(np.float64), exp)                # the doubles themselves are taken bit for bit too
            assert m2 == m
            text = im.describe_cost(m)
            assert 'chunk %d' % m.chunk in text and 'start site %d' % m.start in text and 'end site %d' % m.end in text


def test_two_cells_of_one_row_swapped(tiny):
    _, _, _, one, _ = tiny
    e = one[0]
    want = im.dense(one, 'cost')
    k = int(np.flatnonzero(e.W >= 5)[3])
    a, b = int(e.cum[k]) + 1, int(e.cum[k]) + 4
    assert want[a] != want[b]
    got = want.copy()
    got[a], got[b] = want[b], want[a]
    m = im.diff_cost(got, one)
    assert m is not None and m.count == 2 and (m.chunk, m.start, m.end) == (0, k, k + 1)
    assert m.got == int(want[b]) and m.want == int(want[a])


def test_one_chunks_rows_shifted_by_one_entry(tiny):
    """What a hook that placed the second chunk one entry late (or early) would return."""
    _, _, _, _, two = tiny
    want = im.dense(two, 'cost')
    n0 = two[0].cost.size
    for got in (np.concatenate([want[:n0], want[n0 - 1:-1]]), np.concatenate([want[:n0], want[n0 + 1:], want[-1:]])):
        assert got.size == want.size
        j = int(np.flatnonzero(got != want)[0])
        assert j >= n0
        m = im.diff_cost(got, two)
        assert m is not None and m.chunk == 1 and (m.chunk, m.start, m.end) == _cell_by_walking(two, j)
        assert j - n0 <= 1 and m.start == 0                  # the very first row of the shifted chunk gives it away
    short = want[:-1]
    m = im.diff_cost(short, two)
    assert m is not None and m.chunk is None and (m.got, m.want) == (want.size - 1, want.size)
    assert 'entries fetched' in im.describe(m)


def test_one_back_pointer_off_by_one(tiny):
    _, _, _, one, two = tiny
    for exp in (one, two):
        want = im.dense(exp, 'back')
        off = im.dense_offsets([e.length for e in exp])
        for j in (0, 77, want.size - 1, int(off[-2]), int(off[-2]) + 5):
            for step in (1, -1):
                got = want.astype(np.uint16)
                got[j] = int(want[j]) + step
                m = im.diff_sites('back', got, exp)
                c = int(np.searchsorted(off, j, 'right') - 1)
                assert m is not None and m.count == 1 and (m.chunk, m.start, m.end) == (c, None, j - int(off[c]))
                assert (m.got, m.want) == (int(want[j]) + step, int(want[j]))
                assert 'end site %d' % (j - int(off[c])) in im.describe(m)
    # and the window extents / row offsets name the start site
    got = im.dense(two, 'window').astype(np.uint16)
    j = two[0].length + 9
    got[j] += 1
    m = im.diff_sites('window', got, two)
    assert (m.chunk, m.start, m.end, m.count) == (1, 9, None, 1)


@pytest.mark.parametrize('lens', [[1], [7], [8], [9], [1025], [1, 7, 8, 9, 1025], [1025, 9, 8, 7, 1], [7, 7, 7], [9, 1, 9]])
def test_dense_layout_bookkeeping(lens):
    """Chunk lengths on both sides of the 8-entry grid (the library keeps every chunk's slice of its own arrays from a multiple of 8 on; the hook
    leaves that padding out).  Dense offsets are the running sums of the lengths / of the chunks' blocks; every entry of the dense arrays maps back
    to its (chunk, start, end); and the first `sites` entries of the PADDED arrays — what the hook returned before it compacted — do not pass for
    the dense ones unless every length but the last is a multiple of 8."""
    rng = np.random.default_rng(sum(lens) + len(lens))
    exp = []
    for c, l in enumerate(lens):
        W = np.minimum(rng.integers(1, 12, l), np.arange(l, 0, -1)).astype(np.int64)
        cum = np.concatenate([[0], np.cumsum(W)[:-1]]).astype(np.int64)
        cost = rng.integers(1, 2 ** 62, int(W.sum())).astype(np.uint64)
        back = np.minimum(rng.integers(1, 12, l), np.arange(1, l + 1)).astype(np.int64)
        exp.append(im.Expected(100 * c + 3, l, W, cum, cost, back, np.array([0, l], dtype=np.int32)))
    soff = im.dense_offsets(lens)
    coff = im.dense_offsets([e.cost.size for e in exp])
    assert soff.tolist() == [sum(lens[:c]) for c in range(len(lens) + 1)]
    assert coff.tolist() == [sum(int(e.W.sum()) for e in exp[:c]) for c in range(len(lens) + 1)]
    for what in ('window', 'cum', 'back', 'cost'):
        d = im.dense(exp, what)
        assert d.size == (coff[-1] if what == 'cost' else soff[-1])
    # every entry maps back to its cell
    j = 0
    for c, e in enumerate(exp):
        for k in range(e.length):
            assert im.locate_site(exp, int(soff[c]) + k) == (c, k)
            for t in (0, int(e.W[k]) - 1):
                assert im.locate_cost(exp, j + t) == (c, k, k + t)
            j += int(e.W[k])
    assert j == coff[-1]
    # the padded arrays of the library, cut at `sites` entries
    poff = np.concatenate([[0], np.cumsum([(l + 7) // 8 * 8 for l in lens])])
    for what in ('window', 'cum', 'back'):
        field = {'window': 'W', 'cum': 'cum', 'back': 'back'}[what]
        padded = np.full(int(poff[-1]), 0xdead, dtype=np.int64)
        for c, e in enumerate(exp):
            padded[poff[c]:poff[c] + e.length] = getattr(e, field)
        m = im.diff_sites(what, padded[:soff[-1]], exp)
        first_gap = next((c for c, l in enumerate(lens[:-1]) if l % 8), None)
        if first_gap is None:
            assert m is None
        else:
            assert m is not None and (m.chunk, m.start if what != 'back' else m.end) == (first_gap + 1, 0) and m.got == 0xdead
