"""The small world of the block-plan tests (tests/test_blocks_cpu.py: the host plan against a numpy restatement;
tests/test_gpu_blocks.py: the kernels behind it against the oracle): blocks tables over N_TOTAL = 17,413 sites — two full
runs of eight 1024-site tiles, one partial run, a ragged last 16-byte vector.

ordered()   ordered by first AND by last site (the streaming kernel's tables), with
              * a block edge at every multiple of 896 (the general kernel's tile) and of 1024 (the streaming kernel's; every
                eighth is a run boundary), each -1, 0 and +1: as the edges of a tiling, and, where a long block lies over
                them, as the ends of blocks that begin just before it and the starts of blocks that end with it;
              * blocks of exactly 1024 and 1025 sites, and one of 2,500 sites that starts one site before the run boundary 8192;
              * an empty block at site 0, an empty block at N_TOTAL, a one-site block at N_TOTAL - 1.
shuffled()  the same rows in a fixed shuffled order
nested()    the same rows and one block that contains many others: ordered by first site, not by last
identical() one row forty times
"""
import numpy as np

N_TOTAL = 17413
LONG = ((1500, 2524), (4000, 5025), (8191, 10691))          # 1024, 1025 and 2,500 sites


def ordered():
    edges = sorted({m + d for tile in (896, 1024) for m in range(tile, N_TOTAL, tile) for d in (-1, 0, 1)})
    cuts = {0, N_TOTAL} | {x for x in edges if not any(S < x < T for S, T in LONG)}
    rows = [(0, 0), (N_TOTAL - 1, N_TOTAL), (N_TOTAL, N_TOTAL)]
    for S, T in LONG:
        inside = [x for x in edges if S < x < T]
        cuts |= {S - 1 - len(inside), S, T}
        for j, x in enumerate(inside):
            rows.append((S - len(inside) + j, x))          # ends on the edge; these begin one after the other just before the long block
            rows.append((x, T))                            # starts on the edge, ends with the long block
    cuts = sorted(cuts)
    rows += list(zip(cuts[:-1], cuts[1:]))
    rows.sort()
    s0 = np.array([r[0] for r in rows], dtype=np.int64)
    e0 = np.array([r[1] for r in rows], dtype=np.int64)
    assert (np.diff(s0) >= 0).all() and (np.diff(e0) >= 0).all() and len(rows) < 400
    return s0, e0


def shuffled(keep_ties=True):
    """keep_ties: the two blocks that start at site 0 stay in file order, so that the stable sort leaves the table ordered by last site too"""
    s0, e0 = ordered()
    o = np.random.default_rng(20261018).permutation(s0.size)
    if keep_ties:
        at0 = np.flatnonzero(s0[o] == 0)
        assert at0.size == 2
        o[at0] = np.sort(o[at0])
    return s0[o], e0[o]


def nested():
    s0, e0 = ordered()
    k = int(np.searchsorted(s0, 100))
    return np.insert(s0, k, 100), np.insert(e0, k, 9000)


def identical():
    return np.full(40, 700, dtype=np.int64), np.full(40, 1900, dtype=np.int64)
