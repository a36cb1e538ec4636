"""the batch and the parameter sets of tests/test_bsw_rowmax.py and tests/test_bsw_rowmax_gpu.py (no tests in here)"""
import numpy as np

from tools import gabgen
from tests.util import BSW_PARAM_SETS, bsw_handmade_pairs

# (a, b, ambig, o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w) -> the bsw_dp8 instantiation that runs it
GPU_PARAM_SETS = [
    ("dp8<1,1>", BSW_PARAM_SETS[0]),                              # the driver's defaults
    ("dp8<1,1>", (1, 4, -1, 6, 1, 6, 1, 5, 5, 100)),              # zdrop 5 and 10: the break depends on rowmax_j - best_j
    ("dp8<1,1>", (1, 4, -1, 6, 1, 6, 1, 10, 5, 100)),
    ("dp8<0,1>", (1, 4, -1, 6, 1, 4, 2, 10, 5, 100)),             # asymmetric gaps (SYM false)
    ("dp8<1,0>", (2, 4, -1, 6, 1, 6, 1, 100, 5, 100)),            # max_sc = 2 (MS1 false)
    ("dp8<0,0>", (2, 5, -1, 5, 2, 7, 1, 10, 5, 100)),             # neither
]

_batch = None


def tie_heavy_batch():
    """at most 4 096 pairs.  Homopolymer and period-2 queries of at most 64 bases against references with the same repeat plus single
    substitutions (a row then holds its maximum in several columns), a few of them with one or two substituted query bases; query
    lengths 1 .. 12 at h0 0 .. 3 (beg and end of both parities, bands shorter than one loop trip); the hand-made pairs of
    tests/util.py.  h0 stays below 255 - 144 * 2, so that the 8-bit kernel takes the batch at a match score of 2 as well."""
    global _batch
    if _batch is not None:
        return _batch
    rng = np.random.default_rng(20)
    refs, qrys, h0s = [], [], []

    def repeat(unit, n, phase=0):
        return np.array([unit[(k + phase) % len(unit)] for k in range(n)], np.uint8)

    units = [[0], [1], [2], [3], [0, 1], [2, 3], [0, 2], [3, 1]]
    while len(refs) < 3300:
        unit = units[len(refs) % len(units)]
        qlen = int(rng.integers(4, 65))
        tlen = qlen + int(rng.integers(-3, 40))
        q = repeat(unit, qlen)
        r = repeat(unit, max(tlen, 1), int(rng.integers(0, 2)))
        for _ in range(int(rng.integers(0, 4))):                   # single substitutions in the reference
            at = int(rng.integers(0, len(r)))
            r[at] = (r[at] + int(rng.integers(1, 4))) % 4
        for _ in range(int(rng.integers(0, 3)) // 2 * int(rng.integers(1, 3))):   # ... and now and then in the query
            at = int(rng.integers(0, qlen))
            q[at] = (q[at] + int(rng.integers(1, 4))) % 4
        refs.append(r); qrys.append(q); h0s.append(int(rng.integers(0, 60)) if len(refs) % 5 else int(rng.integers(0, 4)))
    for qlen in range(1, 13):                                      # bands shorter than one loop trip, every parity of beg and end
        for h0 in range(4):
            for unit in ([0], [0, 1], [0, 1, 2, 3]):
                for extra in (0, 1, 7):
                    q = repeat(unit, qlen)
                    r = repeat(unit, qlen + extra, extra & 1)
                    refs.append(r); qrys.append(q); h0s.append(h0)
    hr, hq, hh = bsw_handmade_pairs()
    refs += hr; qrys += hq; h0s += hh
    assert len(refs) <= 4096
    _batch = gabgen.bsw_from_arrays(refs, qrys, h0s)
    return _batch


def gpu_batch(ps, qmax=None):
    """the pairs of the tie-heavy batch that the GPU test runs at parameter set ps: all of them, or -- a match score above 1 fits
    8-bit cells only for short queries -- those with at most 64 query bases; qmax overrides the bound"""
    b = tie_heavy_batch()
    if qmax is None:
        qmax = 64 if max(ps[0], -ps[1], ps[2], 0) > 1 else 256
    idx = np.flatnonzero(b.len2 <= qmax)
    return gabgen.BswBatch(b.ref, b.ref_off[idx].copy(), b.qry, b.qry_off[idx].copy(), b.len1[idx].copy(), b.len2[idx].copy(),
                           b.h0[idx].copy())
