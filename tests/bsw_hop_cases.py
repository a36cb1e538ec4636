"""Hand-made pairs for the hop bound of the seeded prune (tools/gen/bsw_exit_model.c, hop_bound; bsw.hip's header), shared by
tests/test_bsw_hop_bound.py and tests/test_bsw_hop_bound_gpu.py.

Every pair is cut from one query of 100 bases with period 4 (0, 3, 2, 1, ...): against itself shifted by one, two or three bases
it mismatches at every base, so what the ungapped scan and every candidate see behind an indel is known without running anything.
L_hop is written out per pair for the driver's defaults (match 1, mismatch -4, N -1, gaps 6 + 1, z-drop 100, w 100)."""
import numpy as np

from tools import gabgen

Q = np.array([k % 4 for k in range(0, 700, 7)], np.uint8)            # 100 bases
TAIL = (Q[:20] + 2) % 4                                              # what follows the last reference base that belongs to the query


def cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts])


def cases():
    """-> list of (name, reference, query, h0, L_ungapped, L_hop at the defaults)"""
    q = Q
    c = []
    # a base of the query missing in the reference: one inserted query base, 6 + 1
    c.append(("indel after base 1", cat(q[:1], q[2:], TAIL), q, 30, 31, 31 - 7 + 98))
    c.append(("indel after base 40", cat(q[:40], q[41:], TAIL), q, 30, 70, 70 - 7 + 59))
    # two inserted bases, 30 + 29 + 39 matches: the second segment is scanned in chunks of sixteen, its peak is found at the chunk end
    # behind the second indel (82 - 3 mismatches = 70 at step 32), the hop leaves four steps before it (81 at step 28), pays one
    # mismatch and matches the last 39 bases: 81 - 7 - 4 + 39
    c.append(("two indels", cat(q[:30], q[31:60], q[61:], TAIL), q, 30, 60, 81 - 7 - 4 + 39))
    # a base of the reference missing in the query: one deleted reference base
    c.append(("deletion after base 40", cat(q[:40], [(q[40] + 1) % 4], q[40:], TAIL), q, 30, 70, 70 - 7 + 60))
    c.append(("deletion of two after base 40", cat(q[:40], [(q[40] + 1) % 4, (q[40] + 2) % 4], q[40:], TAIL), q, 30, 70, 70 - 8 + 60))
    # two query bases missing in the reference: an insertion of two is not among the gaps, but the query has period 4, so the
    # pair reads as two deleted reference bases as well -- a hop from the peak itself, 6 + 2, then reference bases 42 .. 97
    c.append(("insertion of two bases", cat(q[:40], q[42:], TAIL), q, 30, 70, 70 - 8 + 56))
    # codes above 4 count as N: -1 each at bases 10 and 50 of the main diagonal, and the hop behind base 60 goes on
    r = cat(q[:60], q[61:], TAIL); r[10] = 9
    qq = q.copy(); qq[50] = 200
    c.append(("codes above 4", r, qq, 30, 30 + 60 - 4, 30 + 60 - 4 - 7 + 39))
    c.append(("tlen < qlen", cat(q[:30], q[31:60]), q, 30, 60, 60 - 7 + 29))
    c.append(("qlen 1", q[:30], q[:1], 30, 31, 31))
    c.append(("tlen 1", q[:1], q[:30], 30, 31, 31))
    # the diagonal ends on the last reference base: every candidate's gap would start a segment with no base left
    c.append(("hop past the last reference base", q[:50], q, 30, 80, 80))
    c.append(("first base mismatches", cat([(q[0] + 1) % 4], q[1:]), q, 30, 30 + 95, 30 + 95))      # 26 at base 1, 125 at base 100
    return c


def zdrop_cases():
    """z-drop 10, everything else the defaults -> (name, reference, query, h0, L_ungapped, L_hop).  A step is worth at most
    zdrop + 1 + the smallest path value before it, and h0 is a path value: no L exceeds h0 + 11"""
    q = Q
    x = lambda k: (q[k] + 1) % 4
    c = []
    # 35 at base 5, three mismatches (a dip of 12 to 23), matches from there: capped at 11 + 23 = 34, below the first peak; the peak
    # is not capped (35 - 30 <= 10), so hops are tried from it and from base 1, and every candidate mismatches throughout
    c.append(("dip deeper than the z-drop", cat(q[:5], [x(5), x(6), x(7)], q[8:]), q, 30, 35, 35))
    # 35 at base 5, one inserted base (28: the new minimum), sixteen matches are 44 > 28 + 10: worth 11 + 28
    c.append(("hop, then the cap", cat(q[:5], q[6:], TAIL), q, 30, 35, 39))
    # ... and with two mismatches behind the hop, inside its first chunk: no prefix of the chunk is below 28 - 8 = 20, it ends at
    # 28 + 14 - 8 = 34 > 20 + 10, so it is worth 11 + 20 = 31, less than the first peak
    c.append(("hop, a dip, then the cap", cat(q[:5], q[6:10], [x(10), x(11)], q[12:], TAIL), q, 30, 35, 35))
    # the main diagonal's peak is held down by the cap (41 at base 11 = 30 + 11): no hop is tried
    c.append(("capped peak starts no hop", cat(q[:40], q[41:], TAIL), q, 30, 41, 41))
    return c


def batch(cs=None):
    cs = cases() if cs is None else cs
    return gabgen.bsw_from_arrays([x[1] for x in cs], [x[2] for x in cs], [x[3] for x in cs])
