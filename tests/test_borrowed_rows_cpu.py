"""tests/borrowed_rows.py on device='cpu': the layout it promises — rows where ptr and pitch say, poison everywhere else, the
alignments, guards of 64 KB whatever n — and assert_untouched(), which must pass on a fresh object and fail after one byte of a
pad, of a guard or of a row has changed.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import borrowed_rows as BW

SIZES = [1, 7, 8, 9, 15, 16, 17, 1023, 4099]


def _rows(n, N, seed=3):
    rng = np.random.default_rng([seed, n, N])
    cov = rng.integers(1, 255, (N, n))                          # 1 .. 254: no row site looks like the 'ff00' / '00ff' poison
    meth = (cov * rng.random((N, n))).astype(np.int64)
    return [np.stack([meth[s], cov[s]], axis=1).astype(np.uint8) for s in range(N)]


def _peek(addr, nbytes):
    return np.frombuffer(C.string_at(addr, nbytes), dtype=np.uint8)


@pytest.mark.parametrize('poison', BW.ROW_POISONS)
@pytest.mark.parametrize('n', SIZES)
def test_rows_layout(n, poison):
    for N in (1, 3, 5):
        rows = _rows(n, N)
        b = BW.BorrowedRows(rows, poison, 'cpu')
        assert (b.n, b.N) == (n, N) and b.pitch == (2 * n + 15) // 16 * 16 and 0 <= b.pitch - 2 * n <= 14
        assert b.ptr % 16 == 0 and b.pitch % 16 == 0 and b.row0 % 16 == 0 and b.row0 >= 65536
        assert b.buf.dim() == 1 and b.buf.dtype == torch.uint8 and b.buf.numel() == 2 * b.row0 + N * b.pitch
        assert b.ptr == b.buf.data_ptr() + b.row0
        for s in range(N):                                      # the rows sit where ptr and pitch say
            assert np.array_equal(_peek(b.ptr + s * b.pitch, 2 * n), rows[s].reshape(-1))
        now = b.bytes_now()
        rest = now[~b.is_row_byte()]
        at = np.flatnonzero(~b.is_row_byte())
        assert rest.size == 2 * b.row0 + N * (b.pitch - 2 * n)
        if poison == 'random':
            assert len(np.unique(rest)) > 200                   # (131,072 seeded bytes and more)
            assert np.array_equal(now, BW.BorrowedRows(rows, poison, 'cpu').bytes_now())
        else:                                                   # as sites counted from row 0: (255, 0) or (0, 255), in front of it and behind
            even = (at - b.row0) % 2 == 0
            m, c = (255, 0) if poison == 'ff00' else (0, 255)
            assert (rest[even] == m).all() and (rest[~even] == c).all()
        b.assert_untouched()


def test_explicit_pitch_and_refusals():
    rows = _rows(9, 2)
    b = BW.BorrowedRows(rows, '00ff', 'cpu', pitch=64)
    assert b.pitch == 64 and np.array_equal(_peek(b.ptr + 64, 18), rows[1].reshape(-1))
    assert (_peek(b.ptr + 18, 46).reshape(-1, 2) == (0, 255)).all()
    for pitch in (16, 24, 40):                                  # below 2 n; no multiple of 16
        with pytest.raises(AssertionError):
            BW.BorrowedRows(rows, '00ff', 'cpu', pitch=pitch)
    with pytest.raises(AssertionError):
        BW.BorrowedRows(rows, 'zeros', 'cpu')


@pytest.mark.parametrize('poison', BW.ROW_POISONS)
def test_rows_assert_untouched_sees_one_byte(poison):
    n, N = 13, 3                                                # pitch 32: pads of 6 bytes
    b = BW.BorrowedRows(_rows(n, N), poison, 'cpu')
    last = b.buf.numel() - 1
    spots = {'front guard': [0, b.row0 - 1], 'back guard': [b.row0 + N * b.pitch, last],
             'pad behind row 0': [b.row0 + 2 * n, b.row0 + b.pitch - 1], 'pad behind row 2': [b.row0 + 2 * b.pitch + 2 * n, b.row0 + 3 * b.pitch - 1],
             'row 0, site 0': [b.row0], 'row 1, site 12': [b.row0 + b.pitch + 2 * n - 1]}
    for name, offs in spots.items():
        for off in offs:
            old = int(b.buf[off])
            b.buf[off] = old ^ 0x10
            with pytest.raises(AssertionError, match=r'offset %d \(%s\)' % (off, name)):
                b.assert_untouched()
            b.buf[off] = old
            b.assert_untouched()


@pytest.mark.parametrize('poison', BW.LOCI_POISONS)
@pytest.mark.parametrize('phase', [0, 1, 2, 3])
def test_loci_layout_and_untouched(poison, phase):
    for n in (1, 3, 4, 5, 1025):
        loci = (np.cumsum(np.random.default_rng(n).integers(1, 300, n)) + 7).astype(np.uint32)
        b = BW.BorrowedLoci(loci, poison, 'cpu', phase_words=phase)
        assert b.ptr % 16 == 4 * phase and b.n == n and b.first * 4 >= 65536 and b.first % 4 == 0
        assert b.words.dtype == torch.int32 and b.words.numel() == 2 * b.first + n and b.ptr == b.words.data_ptr() + 4 * b.first
        assert np.array_equal(_peek(b.ptr, 4 * n).view(np.uint32), loci)
        w = b.bytes_now().view(np.uint32)
        want = 0 if poison == '0' else 0xffffffff
        assert (w[:b.first] == want).all() and (w[b.first + n:] == want).all() and w.size == 2 * b.first + n
        b.assert_untouched()
        for word, name in ((0, 'front guard'), (b.first - 1, 'front guard'), (b.first, 'locus 0'), (b.first + n - 1, 'locus %d' % (n - 1)),
                           (b.first + n, 'back guard'), (w.size - 1, 'back guard')):
            old = int(b.words[word])
            b.words[word] = old ^ 0x100
            with pytest.raises(AssertionError, match=r'\(%s\)' % name):
                b.assert_untouched()
            b.words[word] = old
        b.assert_untouched()
