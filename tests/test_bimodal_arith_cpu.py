"""The arithmetic k_bim_em applies to a pair of column counts, HOST build (tests/native/exact_host.cpp: the twin of
bimodal_kernels.h's wg_bim_pair / wg_bim_ll0_term over exact_log2.h), against the live libm and numpy's IEEE float64 on the EM's own
lattice (tests/bimodal_lattice.py): every pair with a + b <= 4096, 20 M log-uniform pairs up to 2^32 - 1, the counts next to
2^32 - 1, and the four first-pass constants.  Full-mantissa quotients on both branches of wg_log2 — not the 24-bit arguments
exact_log2.h was written for and tests/test_exact_log2_cpu.py walks.  No mismatch is allowed: the device is then compared with this
twin (tests/test_gpu_bimodal.py), not with the libm of whatever machine holds the GPU."""
import math

import numpy as np
import pytest

import bimodal_lattice as BL
from oracle import oracle

NAMES = ('pa / n', 'pb / n', 'log2(pa / n)', 'log2(pb / n)', 'n', 'll0 term')
NEAR1_LO, NEAR1_HI = 0x3feea4af00000000, 0x3ff0b55900000000      # wg_log2's branch for arguments next to 1


@pytest.fixture(scope='module')
def host():
    return BL.load_host()


def _libm_log2(bits):
    out = np.empty_like(bits)
    oracle.lib().probe_log2_bits_fill(bits.ctypes.data, bits.size, out.ctypes.data, BL.THREADS)
    return out


def test_lattice_is_what_it_claims():
    a, b = BL.small_pairs()
    assert a.size == 8394753 and int((a.astype(np.int64) + b).max()) == BL.SMALL_TOTAL
    assert len(set(zip(a[:6].tolist(), b[:6].tolist()))) == 6 and (a[0], b[0]) == (0, 0) and (a[-1], b[-1]) == (BL.SMALL_TOTAL, 0)
    a, b = BL.random_pairs(100000)
    for v in (a, b):                                              # log-uniform: every binary magnitude, and zero, is drawn
        assert set(np.unique(np.floor(np.log2(v[v > 0]))).astype(int).tolist()) == set(range(32)) and (v == 0).any()
    a, b = BL.edge_pairs()
    assert a.size == 5 * 2001 and int(a.max()) == BL.U32_MAX == int(b.max())


def test_host_twin_equals_libm_and_ieee_on_the_lattice(host):
    bad = dict.fromkeys(NAMES, 0)
    first = {}
    pairs = near1 = 0
    min_exp = 0
    for name, a, b in BL.batches():
        got = BL.host_terms(host, a, b)
        af, bf = a.astype(np.float64), b.astype(np.float64)
        pa, pb = 1e-3 + af, 1e-3 + bf
        n = pa + pb
        qa, qb = pa / n, pb / n
        la, lb = _libm_log2(got[0]), _libm_log2(got[1])
        term = af * la.view(np.float64) + bf * lb.view(np.float64)
        want = (qa.view(np.uint64), qb.view(np.uint64), la, lb, n.view(np.uint64), term.view(np.uint64))
        for k, w in enumerate(want):
            d = np.flatnonzero(got[k] != w)
            bad[NAMES[k]] += d.size
            if d.size:
                first.setdefault(NAMES[k], (name, int(a[d[0]]), int(b[d[0]]), hex(int(got[k][d[0]])), hex(int(w[d[0]]))))
        pairs += a.size
        for q in got[:2]:
            near1 += int(((q >= NEAR1_LO) & (q < NEAR1_HI)).sum())
            min_exp = min(min_exp, int((q >> np.uint64(52)).min()) - 1023)
    print('bimodal lattice: %d pairs, %d arguments in the near-1 branch, lowest binary exponent %d, mismatches %s'
          % (pairs, near1, min_exp, bad))
    assert pairs == 8394753 + BL.N_RANDOM + 5 * 2001
    assert near1 > 300000 and min_exp <= -41                      # both branches, and the smallest arguments uint32 counters give
    assert not any(bad.values()), (bad, first)


def test_first_pass_constants(host):
    x = np.array(BL.CONSTANTS, dtype=np.float64)
    got = np.empty(x.size, dtype=np.uint64)
    host.exact_log2_bits_fill(x.ctypes.data, x.size, got.ctypes.data)
    want = np.array([math.log2(v) for v in BL.CONSTANTS], dtype=np.float64).view(np.uint64)
    assert got.tolist() == want.tolist() == _libm_log2(x.view(np.uint64)).tolist()
