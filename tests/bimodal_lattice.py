"""The column-count pairs (a, b) = (#C, #T) on which the arithmetic of k_bim_em is compared (tests/test_bimodal_arith_cpu.py: the host
twin against the live libm; tests/test_gpu_bimodal.py: the device against the host twin), and the loader of the host twin.  The EM
takes log2 of (1e-3 + a) / ((1e-3 + a) + (1e-3 + b)): full-mantissa doubles down to about 2^-42 for uint32 counts, on both branches
of wg_log2.  Deterministic across platforms: the random pairs are synth.hash_at (splitmix64) and integer shifts."""
import ctypes as C
import os
import os.path as op
import subprocess

import numpy as np

from wgbs_tools_amd.synth import hash_at

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
SRC = op.join(ROOT, 'tests', 'native', 'exact_host.cpp')
LIB = op.join(ROOT, 'tests', 'native', 'libexact_host.so')
HDR = op.join(ROOT, 'wgbs_tools_amd', 'csrc', 'exact_log2.h')
U32_MAX = 2 ** 32 - 1
SMALL_TOTAL = 4096
N_RANDOM = 20000000
SEED = 20261016
CONSTANTS = (0.9, 0.1, 1.0 - 0.9, 1.0 - 0.1)                     # the first pass's p_c and p_t
THREADS = min(16, os.cpu_count() or 1)


def small_pairs():
    """every (a, b) with a + b <= SMALL_TOTAL: 8,394,753 pairs"""
    t = np.repeat(np.arange(SMALL_TOTAL + 1, dtype=np.int64), np.arange(1, SMALL_TOTAL + 2))
    a = np.arange(t.size, dtype=np.int64) - t * (t + 1) // 2
    return a.astype(np.uint32), (t - a).astype(np.uint32)


def random_pairs(n=N_RANDOM, seed=SEED):
    """n pairs, each count log-uniform over 0 .. 2^32 - 1: 32 random bits shifted right by 0 .. 31 places"""
    out = []
    for stream in (1, 2):
        h = hash_at(seed, stream, np.arange(n, dtype=np.int64))
        out.append(((h & np.uint64(U32_MAX)) >> (h >> np.uint64(59))).astype(np.uint32))
    return out[0], out[1]


def edge_pairs():
    """the 2,001 counts next to 2^32 - 1 with 0, with 1 (either way round) and with themselves"""
    v = np.arange(U32_MAX - 2000, U32_MAX + 1, dtype=np.int64)
    z, o = np.zeros_like(v), np.ones_like(v)
    a = np.concatenate([v, z, v, o, v])
    b = np.concatenate([z, v, o, v, v])
    return a.astype(np.uint32), b.astype(np.uint32)


def batches(size=1 << 22):
    """(name, a, b) over the whole lattice in pieces of at most `size` pairs"""
    for name, (a, b) in (('small', small_pairs()), ('random', random_pairs()), ('edge', edge_pairs())):
        for lo in range(0, a.size, size):
            yield '%s[%d:]' % (name, lo), np.ascontiguousarray(a[lo:lo + size]), np.ascontiguousarray(b[lo:lo + size])


def load_host():
    """tests/native/libexact_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(SRC), op.getmtime(HDR)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-pthread', SRC, '-o', LIB])
    L = C.CDLL(LIB)
    L.bimodal_terms_fill.restype = None
    L.bimodal_terms_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
    L.exact_log2_bits_fill.restype = None
    L.exact_log2_bits_fill.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return L


def host_terms(L, a, b):
    """the host twin: uint64 [6][n] bit patterns of pa / n, pb / n, log2 of both, n, the ll0 term"""
    out = np.empty((6, a.size), dtype=np.uint64)
    L.bimodal_terms_fill(a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data, THREADS)
    return out
