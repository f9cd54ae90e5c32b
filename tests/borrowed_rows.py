"""TEST INFRASTRUCTURE: resident rows and loci laid out the way a caller of wgbsseg_set_betas_device / wgbsseg_set_loci_device may
lay them out, and the way the library's own rows never are: the tightest pitch include/wgbsseg.h allows and no zeros behind a row.

    [ guard | row 0 | pad | row 1 | pad | ... | row N-1 | pad | guard ]        one flat torch uint8 tensor

  * pitch = 2 n rounded up to 16 bytes (or the caller's), so a pad is 0 .. 14 bytes: the last 16-byte vector of a row holds up to
    7 sites that are not the row's;
  * every byte that is not row data — both guards, every pad — holds a POISON, so that a kernel which counts a site behind a
    row's end, or the site in front of row 0, changes its result;
  * the guards are GUARD bytes whatever n is: whatever a kernel might still read beyond a row lands inside this one allocation;
  * assert_untouched() holds the whole tensor against a copy taken at construction: the library only reads borrowed memory.

Poisons of the rows, by name:  'ff00' (meth 255, cov 0 at every site: meth > cov, and a methylated count),  '00ff' (meth 0,
cov 255: coverage only),  'random' (seeded bytes).  Of the loci:  '0'  and  'ffffffff'.

The constructors work on device='cpu' as well (tests/test_borrowed_rows_cpu.py checks the layout there).  Not imported by the product.
"""
import numpy as np

GUARD = 65536                      # bytes of each guard: a multiple of 16, and more than any kernel's stride past a row's last vector
ROW_POISONS = ('ff00', '00ff', 'random')
LOCI_POISONS = ('0', 'ffffffff')


def round_up(x, m):
    return (x + m - 1) // m * m


def _aligned_tensor(image, device, align, phase):
    """a 1-D torch uint8 tensor holding the bytes `image` whose byte `phase` sits on a multiple of `align`; -> (tensor, keepalive)"""
    import torch
    store = torch.empty(image.size + align, dtype=torch.uint8, device=device)
    skip = (-(store.data_ptr() + phase)) % align
    buf = store[skip:skip + image.size]
    buf.copy_(torch.from_numpy(image))
    return buf, store


class _Borrowed:
    """the tensor, the copy taken at construction and the comparison"""

    def _adopt(self, image, device, align, phase):
        self.image = image                                     # host copy of every byte, as laid out
        self.buf, self._store = _aligned_tensor(image, device, align, phase)
        self.device = device

    def bytes_now(self):
        return self.buf.cpu().numpy()

    def assert_untouched(self):
        now = self.bytes_now()
        bad = np.flatnonzero(now != self.image)
        assert bad.size == 0, '%d bytes of the borrowed buffer changed, the first at offset %d (%s): %d -> %d' % (
            bad.size, bad[0], self.where(int(bad[0])), self.image[bad[0]], now[bad[0]])


class BorrowedRows(_Borrowed):
    """rows: N uint8 arrays [n, 2].  .buf (the flat tensor), .ptr (address of row 0, a multiple of 16), .pitch, .n, .N, .row0 (offset
    of row 0 in .buf), .rows (the arrays, as given)."""

    def __init__(self, rows, poison, device, pitch=None, seed=0):
        rows = [np.ascontiguousarray(r, dtype=np.uint8) for r in rows]
        n = rows[0].shape[0]
        assert len(rows) >= 1 and n >= 1 and all(r.shape == (n, 2) for r in rows)
        pitch = round_up(2 * n, 16) if pitch is None else int(pitch)
        assert pitch % 16 == 0 and pitch >= 2 * n and GUARD % 16 == 0
        assert poison in ROW_POISONS, poison
        N = len(rows)
        total = 2 * GUARD + N * pitch
        if poison == 'random':
            image = np.random.default_rng([20261020, seed, n, N]).integers(0, 256, total, dtype=np.uint8)
        else:
            image = np.empty(total, dtype=np.uint8)            # (row 0 begins on an even offset: even bytes are meth, odd bytes cov)
            image[0::2] = 0xff if poison == 'ff00' else 0x00
            image[1::2] = 0x00 if poison == 'ff00' else 0xff
        for s, r in enumerate(rows):
            image[GUARD + s * pitch:GUARD + s * pitch + 2 * n] = r.reshape(-1)
        self.rows, self.poison, self.n, self.N, self.pitch, self.row0 = rows, poison, n, N, pitch, GUARD
        self._adopt(image, device, 16, GUARD)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def is_row_byte(self):
        """bool mask over .buf: the bytes that are row data"""
        m = np.zeros(self.image.size, dtype=bool)
        for s in range(self.N):
            m[self.row0 + s * self.pitch:self.row0 + s * self.pitch + 2 * self.n] = True
        return m

    def where(self, off):
        if off < self.row0:
            return 'front guard'
        s, b = divmod(off - self.row0, self.pitch)
        if s >= self.N:
            return 'back guard'
        return 'row %d, site %d' % (s, b // 2) if b < 2 * self.n else 'pad behind row %d' % s


class BorrowedLoci(_Borrowed):
    """loci: uint32 [n] inside an int32 tensor between two guards.  .buf (the flat uint8 tensor under it), .words (the same memory as
    int32), .ptr (address of loci[0]: 4 * phase_words bytes behind a multiple of 16), .n, .first (index of loci[0] in .words)."""

    def __init__(self, loci, poison, device, phase_words=0):
        loci = np.ascontiguousarray(loci, dtype=np.uint32)
        assert loci.ndim == 1 and loci.size >= 1 and 0 <= phase_words < 4
        assert str(poison) in LOCI_POISONS, poison
        n = loci.size
        words = 2 * (GUARD // 4) + n
        image = np.full(words, 0 if str(poison) == '0' else 0xffffffff, dtype=np.uint32)
        image[GUARD // 4:GUARD // 4 + n] = loci
        self.loci, self.poison, self.n, self.first = loci, str(poison), n, GUARD // 4
        self._adopt(image.view(np.uint8), device, 16, GUARD - 4 * phase_words)
        import torch
        self.words = self.buf.view(torch.int32)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 4 * phase_words

    def where(self, off):
        w = off // 4
        return 'front guard' if w < self.first else ('back guard' if w >= self.first + self.n else 'locus %d' % (w - self.first))
