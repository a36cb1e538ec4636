// bsw -- banded Smith-Waterman seed extension on gfx950.
//
// Semantics: BandedPairWiseSW::scalarBandedSWA
//   (/root/reference/benchmarks/bsw/src/bandedSWA.cpp:132-253), which is what the
//   reference's inter-sequence SIMD path (getScores16, bandedSWA.cpp:1128-1835) emulates
//   lane by lane.  The CPU vectorises ACROSS pairs (one pair per 16-bit SIMD lane) because
//   the adaptive band, the z-drop exit and the first/last-max tie rules make the rows of
//   one pair strictly sequential.  The MI355X equivalent of that idea is one pair per
//   wavefront lane:
//
//   1. bucket  -- counting sort of the pairs by (query length, deficit of the ungapped
//                 extension: bsw_key) so that the 64 lanes of a wave carry near-identical work
//                 and diverge little (the reference sorts by len1 for the same reason,
//                 bandedSWA.cpp:372-407);
//   2. bsw_dp  -- one wave (= one workgroup) per 64 sorted pairs.  The H/E row of every
//                 lane lives in LDS as [column][lane] dwords (bank = lane, conflict-free
//                 for any per-lane column), H and E packed as two u16 in one dword when
//                 max(h0) + qcap*max(mat) fits 15 bits (the reference's own int16 lanes),
//                 else two dwords (bsw_dp8: one byte each when it fits 8 bits); max(h0) is that
//                 of the launch's pairs, qcap the bound of its longest class.  LDS is sized per
//                 launch from the query-length class, so short queries get up to 8 waves/CU
//                 and 256-base queries still fit.
//   Results are scattered back by pair id, so the output order is the input order.
//
// Early exit of score-only calls (result_out == nullptr; the six-field result takes gscore / gtle ties from later rows and
// keeps the reference's sweep).  The score is the largest H over all rows, and in seed extension the reference window is
// longer than the read: once the query is used up the remaining rows only carry E values that decay by e_del per row, never
// z-drop at the default penalties and never beat `best`.  After row i, with the band trimmed to the new [beg, end],
// R = tlen - 1 - i rows left and Hd[j] = H(i, j - 1) the stored diagonal of column j, let
//     pot(j) = Hd[j] + max_sc * min(R, qlen - j)   (0 when Hd[j] == 0).
// The row loop ends when  max( max_{beg <= j <= end} pot(j),  boundary,  stale_pot ) <= best, where
//     boundary  = hb + max_sc * min(R, qlen) while beg == 0 and hb = h0 - o_del - e_del * (i + 2) > 0 (next row's left edge),
//     stale_pot = running max of best + max_sc * (qlen - (i + w + 1)), folded in whenever the band clamp end > i + w + 1
//                 fires: that clamp cuts live cells (each <= best then) which a later, wider row reads again; the zero
//                 trimming leaves only zeros behind.
// Proof that no later row exceeds the bound: every DP move keeps value + max_sc * min(rows left, columns left) from growing --
//   a diagonal step gains at most max_sc and uses a row and a column; an E step loses value and uses a row, an F step loses
//   value and uses a column; a zero diagonal yields M = 0.
//   E cells need no term: Ev[j] <= H(i, j) - e_del = Hd[j + 1] - e_del, and column j + 1's diagonal has as many columns left.
//   `best` only changes on a strictly larger row maximum, so a sweep that stops there returns the reference's score.
// The pass over the band runs only in rows that did not raise `best` and whose maximum cell alone passes the test
// (rowmax + max_sc * min(R, qlen - 1 - rowmax_j) <= best): never inside the matching region, about once per pair behind it.
// On the read-like generator input it removes 23 % of the DP cells and 36 % of the rows (profiles/bsw_early_exit.md);
// tools/gen/bsw_exit_model.c is the CPU model of the rule that the tests pin the cell counter to.
//
// Left prune of score-only calls (same condition as the exit; tools/gen/bsw_exit_model.c is the CPU model of it, and the tests pin
// every kernel's cell counter to that model).  After row i, once both zero trims have run, with R rows left, `best` already updated
// for the row and m(j) = max(Hd[j], Ev[j]) of stored cell j, the left edge moves over cell beg while beg < end and
//     m(beg) == 0                                      (the reference's own trim), or
//     m(beg) + max_sc * min(R, qlen - beg) <= best,    and -- while beg == 0 -- hb <= 0 or hb + max_sc * min(R, qlen) <= best
//                                                      for the next row's left edge hb = h0 - o_del - e_del * (i + 2).
// The exit's bound pass then runs over the narrowed band.  On the read-like input the pruned run evaluates 0.788 of the cells that
// the exit alone leaves (profiles/bsw_left_prune.md).
// The rule is RESTRICTED to pairs with
//   (a) qlen <= w + 1 or h0 - oe_ins - (w + 1) * e_ins <= 0: row -1 is zero from column w + 2 on, so the band clamp of row 0 cuts
//       only zeros.  A later clamp hides no computed cell (the row before wrote cells up to i + w only), and the zero trim leaves only
//       zeros behind, so EVERY cell right of `end` that a later row reads again is zero, in both runs (step 5 needs this: with a live
//       row -1 cell out there the pruned run could read it in a later row than the reference did, against another reference base);
//   (b) zdrop == 0 or zdrop >= 8 * max_sc: economy, not correctness -- under a smaller z-drop the guard below sends so many pairs
//       through a second pass that the cell count rises above the reference's (measured on the adversarial generator input).
// z-drop guard: a pair that has dropped a live cell knows its row maxima only as lower bounds of the reference's.  Either z-drop
// test needs rowmax < best - zdrop to fire, so such a pair, in a row with zdrop > 0, rowmax <= best and rowmax < best - zdrop, abandons
// the pass and runs again from row -1 with the prune off and the exit on; the cell counter keeps the abandoned pass.  Step 5 of the
// proof adds a second, much rarer reason to abandon the pass.
// Proof.  Call a cell of the REFERENCE's run dead when value + max_sc * min(rows left, columns left) <= best (a zero is dead: it
// yields M = 0), P the pruned run's value of a cell.  Invariant after every row: the two runs have the same best, best_i, best_j; for
// every stored cell j >= beg of the pruned run P <= reference, and P == reference or the reference's cell is dead; every cell of the
// reference that the pruned run does not hold (left of its beg, or right of its end) is dead.
//   1. Potential never grows along a move (the exit's proof above: M uses a row and a column for at most max_sc, E a row, F a
//      column, both at a loss; M is taken as max(M, 0), which changes no H, E' or F), `best` never falls and R only shrinks: what is
//      dead stays dead, and a cell whose largest source is dead is dead.  The DP is monotone in its inputs, so P <= reference
//      carries over, and a cell that is not dead has a largest source that is not dead, which by the invariant the pruned run holds
//      at the same value: P == reference there.
//   2. A dropped cell is zero or, by the invariant, stands for a dead cell of the reference (equal value and the rule's test, or
//      dead already).  Hd[beg] leads to cell (i + 1, beg) with qlen - beg columns left, Ev[beg] to the same cell with fewer: the test
//      bounds both.  `beg` never decreases, so the cell is not read again; the next row starts right of it with F = 0 and hleft = 0
//      where the reference carries values that come from dead cells only -- by induction over the columns from its own beg, whose
//      sources are dropped cells, dead F and, at column 0, the left edge.  Column 0 is left only when the edge of the next row is
//      dead; later edges are smaller with fewer rows.  (Stored cell 0 holds this row's edge, which is larger than hb, so its own
//      test implies the edge's; the term is kept as the rule states it.)
//   3. best: a cell above `best` is not dead, so the pruned run holds it at the same value, in the same row, and every column that
//      ties with it too: best, best_i and best_j (last column of the row's maximum) are the reference's.
//   4. rowmax == 0 in the pruned run: its band holds zeros only, so by the invariant every cell of the reference's row is dead, the
//      cells right of `end` are zero by (a) and column 0 was left behind a dead edge (a pair that still holds column 0 has dropped
//      nothing and IS the reference).  No later row of the reference exceeds best: ending here returns its score.
//   5. Right edge: P <= reference, so the pruned run's last non-zero cell and with it its `end` never lie right of the reference's,
//      and they fall short of it only over cells that are zero in the pruned run, hence dead in the reference.  A cell (i, c) that the
//      reference computes right of the pruned band takes M and E from such dead cells (or, by (a), from zeros) and F from the band's
//      last column, which is at most hleft - e_ins for hleft = H(i, end - 1).  Right-edge guard: a pair that has dropped a live cell
//      abandons the pass, as under the z-drop guard, in a row with end < qlen, end != i + w + 1 (at the clamp both bands end alike),
//      hleft > e_ins and hleft - e_ins + max_sc * min(R, qlen - end - 1) > best.  In every row that is kept that F is dead, and so
//      is every cell the reference has beyond the pruned band; none of them exceeds hleft, so the row's maximum and its column
//      stand.  When the pruned band grows again it reads a zero where the reference may hold a dead value: P <= reference,
//      reference dead.  stale_pot is the same number in both runs (best and the clamp are the same) and stays in the bound.
//      (On the generator's inputs this guard has not fired once; it is there because the proof needs it.)
//   6. The exit's bound on P: a later cell of the reference above best is not dead, so its chain of largest sources runs through
//      cells that are not dead, which the pruned run holds at equal values inside [beg, end], at the left edge or among the cells
//      stale_pot stands for: exactly what the bound covers, by the exit's own proof applied to the pruned run.
//   7. z-drop: while nothing live has been dropped the run is the reference.  Afterwards rowmax <= the reference's rowmax, and the
//      reference's test fires only if its rowmax < best - zdrop, hence only if ours is; the guard abandons exactly those rows, before
//      our own test reads a column that may not be the reference's.  In every row that is kept neither run's test can fire.
//
// Right prune of score-only calls (same calls, same pairs: restrictions (a) and (b)).  After the left prune, with jl the last live
// stored cell -- where the reference's right trim stopped; the next end is min(jl + 2, qlen) -- the right edge moves over cell jl
// while jl >= beg and
//     m(jl) == 0   or   m(jl) + max_sc * min(R, qlen - jl) <= best:
// the cell is SET TO ZERO (Hd = Ev = 0), jl moves one cell left, and end = min(jl + 2, qlen) afterwards.  A drop of a live cell
// sets `dropped`.  On the read-like input the run evaluates 0.725 of the cells that the left prune alone leaves
// (profiles/bsw_right_prune.md).
// Cap, both sides: per row an edge moves over at most the four cells next to the edge the row was swept with -- beg0 .. beg0 + 3 on
// the left, end0 - 3 .. end0 on the right, the windows the zero trim fetches anyway -- and a row whose zero trim has run past its
// window prunes nothing on that side.  Any subset of the drops is safe (each drop is justified by its own cell), so the cap needs
// no argument of its own; it costs 0.7 % more cells than the uncapped left rule and removes its cell-by-cell loop.
// Proof, continued.
//   8. The test is step 2's: Hd[jl] leads to cell (i + 1, jl) with qlen - jl columns left, Ev[jl] to the same cell with fewer, so a
//      dropped cell is zero or stands for a dead cell of the reference; writing zero keeps P <= reference with the reference's cell
//      dead.  Unlike a cell left of beg, a cell right of end IS read again when the band grows, and (a) rests on all of those being
//      zero: the zeroing is what keeps (a) true, and with it steps 4 and 5 as they stand.  The rest is the reference's own
//      zero-trim bookkeeping on a row whose last cells are zero: end = jl + 2, the exit's bound pass over [beg, end].
//   9. The guards are unchanged because a right drop sets `dropped` like a left one.  Step 5's F: stored cell jl holds
//      H(i, jl - 1), which has one column more left than the F that leaves column jl - 1 and is at least that F + e_ins, so the
//      cell's test implies the F test for every dropped cell; for the F that leaves the narrowed band in a LATER row the
//      right-edge guard stands as it is.  Step 7 holds for any pair with rowmax <= the reference's.
//  10. Zero-row guard.  Step 4 used "a pair that still holds column 0 has dropped nothing"; the right prune drops cells of such
//      pairs.  With rowmax == 0 every cell of the reference's row is still dead, but dead cells may keep the reference's row maximum
//      above zero and its row loop alive until the left edge raises the score, where the pruned run would stop.  So a row with
//      rowmax == 0 of a pair that has dropped a live cell, has beg == 0 and a left edge hb = h0 - o_del - e_del * (i + 1) > 0
//      (stored cell 0, the diagonal of cell (i + 1, 0)) with hb + max_sc * min(R, qlen) > best abandons the pass like the other
//      two guards.  With a dead or zero edge nothing the reference still holds can exceed best, and ending returns its score.
//      (9 of the 10 M read-like pairs at the defaults; found by the model at a mismatch score of -128, where rows of zeros are common.)
//
// Seeded prune of score-only calls (same calls, same pairs: restrictions (a) and (b); the six-field form is untouched;
// profiles/bsw_seeded_prune.md).  `best` is the score reached SO FAR, about h0 early in a pair, so the tests above keep every cell
// within about (qlen - i) / 2 columns of the diagonal although the pair ends far above h0.  A lower bound L of the pair's FINAL score is
// known before row 0, and a cell whose potential is below L cannot lead to the final score whatever `best` is at its row.
//   L (pass 0 of the sort, one scan of both sequences: inside bsw_hist<true>, or bsw_seed beside DP kernels; the record carries it).  d_0 = h0 and d_{k+1} = d_k +
//     mat[ref[k]][qry[k]] for k = 0 .. min(qlen, tlen) - 1, codes above 4 as N, stopped at the first d <= 0;
//         L = max( h0,  max_k d_k )                                                    with zdrop == 0,
//         L = max( h0,  max_k min( d_k,  zdrop + 1 + min_{m < k} d_m ) )               with zdrop > 0.
//     L <= the reference's score: while every d so far is positive, cell (k, k) takes M from a non-zero diagonal, so H(k, k) >= d_{k+1}
//     (the DP is monotone in its inputs; cell (0, 0) reads h0).  The cell is inside the reference's band in every row: |i - j| = 0 <= w,
//     and the zero trims pass only zero cells while stored cell k + 1 = H(k, k) > 0.  Its row is not a zero row.  So if the reference
//     sweeps row k its score is at least d_{k+1}; the only other way its row loop ends earlier is a z-drop in a row i < k, which needs
//     best - rowmax_i - gap > zdrop with gap >= 0 and rowmax_i >= H(i, i) >= d_{i+1}: its score, that `best`, then exceeds
//     d_{i+1} + zdrop.  (The minimum above also runs over d_0: more conservative than needed.)  The score is never below h0.
//   L with hops (matrices of bwa_fill_scmat's form -- one match score a > 0, one mismatch score, one score wherever a code is 4 or
//     above, neither above a; detected once in gab_bsw_create, BswConst::hop; every other matrix keeps the L above, scanned base by
//     base as before; profiles/bsw_hop_bound.md).  The L above stops growing at a pair's first indel.  It is the value of a PATH of
//     the DP, and so is every path that leaves the diagonal through a gap: from the peak of the main diagonal's scan at most three
//     hops (kHops) follow the alignment, each onto a neighbouring diagonal.
//       Candidates.  With kp the peak's step in the current segment (segment 0: the main diagonal; kp counts diagonal steps from the
//         segment's start), the hop leaves from the segment's cell at step kp, kp - 4 or kp - 8 through one of three gaps: one or
//         two reference bases deleted (o_del + g e_del) or one query base inserted (o_ins + e_ins): nine candidates.  One stays
//         out unless (a) it lands on a positive value, (b) it lands inside the band, |i - j| <= w for the pair's clamped w, (c) its
//         start is at least ONE diagonal step into its segment (never the h0 corner, the left edge or a gap cell), and -- economy --
//         the first min(16, bases left) bases behind the gap hold at most four mismatches or Ns and keep `low` (below) positive.
//         Of those that are left, the ONE with the largest d behind these first bases (the first of them in the order step kp,
//         kp - 4, kp - 8 x del 1, del 2, ins 1 on a tie) is scanned; it becomes the next segment if its peak exceeds L, and the
//         chain ends otherwise.
//       A segment behind a hop is scanned in chunks of sixteen bases counted from its start, by the chunk's COUNTS alone (the lanes
//         of a wave hold different pairs: a walk from base to base costs every lane what it costs the slowest).  With nm mismatches
//         and nn Ns among a chunk's cnt bases, low = d - nm max(0, -mm) - nn max(0, -nsc) is at or below every prefix of the chunk
//         and d + cnt a - nm (a - mm) - nn (a - nsc) is the exact value behind it.  The scan stops in front of the first chunk
//         with low <= 0.  mn, the minimum the z-drop cap is made of, takes every `low` and the landing cell's value, and starts
//         from the minimum of the previous segment up to its peak: at or below every value of the path.  A chunk's end is worth
//         min(d, zdrop + 1 + mn) (d with zdrop == 0); the largest worth is the segment's peak.  Behind the peak's chunk the next
//         sixteen bases are taken once more in steps of four by the same rule, and then the run of matches in front of the next
//         mismatch or N: the peak then lies within four bases of where the diagonal really ends, which is where the next hop has to
//         leave from.  A segment whose peak is held down by the cap starts no hop (no candidate's cap is higher).
//       L = the largest peak.  tools/gen/bsw_exit_model.c (hop_bound) states the rule base by base; gabgen.bsw_hop_bound exports it,
//         gabgen.bsw_seed_bound stays the ungapped L.  On the read-like input S - L falls from 20.6 to 6.1 on average and the model
//         evaluates 0.691 of the cells.
//   Threshold thr = max(best, L - 1) replaces `best` in the left prune's cell test and its column-0 edge test, in the right prune's cell
//     test, in the right-edge guard and in the zero-row guard.  L - 1 and not L: a cell of the diagonal path of a perfect ungapped
//     match has potential exactly L (tools/gen/bsw_exit_model.c has that wrong rule as a negative control).  The z-drop guard, `best`
//     itself and the exit's bound <= best are unchanged.
//   Prune of row -1.  Before row 0 the cells of row -1 are dropped from the right under the right prune's test with R = tlen rows left and
//     best = h0 (stored cell j is the diagonal of cell (0, j)); cell 0 stays.  Value and potential both fall from left to right, so
//     the live cells are a prefix, and no cap applies.  end = min(jl + 2, qlen) for the last live cell jl, and an `end` below
//     min(qlen, w + 1), what the reference sweeps row 0 with, counts as a drop: row 0's F runs on right of the last live cell of
//     row -1, and only the right-edge guard judges the F that leaves the narrowed band.
//   Gates (economy, not correctness; measured on the CPU model, profiles/bsw_seeded_prune.md).  The threshold is on wherever the
//     prunes are.  The prune of row -1 is on only with max_sc <= e_ins: where a match is worth more than an inserted base costs, the
//     right-edge guard sends 40 - 70 % of the read-like pairs through a second pass and the cell count rises by up to a third.  Both are
//     off for a pair whose band cannot hold more than nine cells, min(qlen, 2 w + 1) <= 9: such a band is swept in at most two loop trips
//     and the seed removes next to nothing (and the tests of the narrow band's edge-cell paths read their cases off the rule's trace).
// Proof, continued.  Call a cell dead when value + max_sc * min(rows left, columns left) <= thr, S the reference's score (L <= S).
//  11. thr never falls (best never falls, L is fixed) and thr < S until `best` reaches S, so steps 1, 2 and 8 hold with thr for `best`:
//      what is dead stays dead, a dropped cell is zero or stands for a dead cell, P <= reference, and P == reference wherever the
//      reference's cell is not dead.  The prune of row -1 is step 8 applied to the initial row; it keeps (a) (it only writes zeros).
//  12. Step 3 becomes: the pruned run's `best` may LAG the reference's in a row (a cell above `best` but with potential <= L - 1 may
//      have been dropped), never lead it.  The first cell that holds S has potential >= S along its whole chain of largest sources,
//      which is above thr at every row before it (thr <= max(best, L - 1) < S there): none of them is dead, the pruned run holds
//      them at equal values, and its `best` reaches S in the same row, unless a guard has sent the pair back before.  Nothing
//      else reads best_i / best_j of a pair that has dropped a cell: its own z-drop test cannot fire before the z-drop guard does.
//  13. The run does not end early with best < S.  Exit: the chain to S is held and its potential exceeds best, so the bound does.
//      Zero row: the held cells are zero, so the chain runs through the left edge (the zero-row guard abandons: that edge's potential
//      is >= S > thr), or through cells right of `end`, which are zero by (a).  Right edge: an F that leaves the band with potential
//      above thr abandons the pass (step 5 with thr); every other F is dead.
//  14. Step 7 (z-drop).  In a row where the reference z-drops its `best` is S and the row did not raise it, so S was reached in an
//      earlier row and by step 12 the pruned run's `best` is S too; its rowmax <= the reference's < S - zdrop, so the z-drop guard
//      abandons the pass (a pair that has dropped nothing IS the reference).  In a row where the reference does not z-drop the pruned
//      run either goes on or abandons the pass; the second pass is the exit alone.
//  15. L with hops <= S.  Claim: every cell (i, j) of the path -- diagonal steps and gap cells -- is a cell the reference computes,
//      in a row it reaches, at a value >= the path's value v > 0 there; then S >= every value of the path, up to the z-drop (19).
//      Induction along the path.  A diagonal step from a cell with H >= v > 0 gives M >= v + score (the DP is monotone), and a
//      positive cell is neither trimmed nor outside the band when |i - j| <= w (16).  A deleted reference base is E of the cell
//      below: E(i + 1, j) >= H(i, j) - o_del - e_del, a second one E - e_del; an inserted query base is F of the cell to the right,
//      H(i, j) - o_ins - e_ins.  The path's values are these right-hand sides, positive by (a).
//  16. (b) The reference clamps every row to |i - j| <= w with ITS w, the pair's clamped one; a path cell outside would not be
//      computed (w = 0, or end_bonus = -1000 which leaves w = 1).  The gate tests the landing cell; a two-base deletion's first
//      gap cell has an i - j between the start's and the landing cell's, both inside.
//  17. (c) A hop's start must be a cell the reference has computed as a positive H.  The h0 corner and the left edge are not
//      cells of a row: the reference ends its row loop at a row of zeros although the left edge is still alive (a first base that
//      mismatches under a mismatch score of -128: row 0 is zero, S = h0, and a leading deletion would claim 237).  After one
//      diagonal step the start is stored cell j of a swept row with a positive value.  tools/gen/bsw_exit_model.c has the rule
//      without this gate as a negative control (wrong_hop).
//  18. (d) The inserted base lies inside the row's `end`: the start is a positive stored cell j of the previous row's sweep, so
//      that row's right trim stopped at or behind it and end >= j + 2; the F of the cell right of the start is computed.  One base
//      only: a longer run of inserted bases would need the same of every cell it crosses.  The deleted bases need nothing: E is
//      carried down the start's own column, which stays inside [beg, end) while its value is positive.
//  19. (e) Z-drop.  The reference's row loop can end before the path's last row only by its z-drop test in a row i the path has
//      passed, which needs best - rowmax_i > zdrop with rowmax_i >= the path's value in row i >= mn: S, that `best`, exceeds
//      mn + zdrop.  Every step's worth is held at zdrop + 1 + mn with mn at or below EVERY earlier value of the path (gap cells,
//      earlier segments and every prefix of a chunk included: `low`), so L <= S either way.  (A row in which the path sits in a
//      gap cell of E has rowmax >= that E.)
// The sort key of a score-only call (a six-field call keeps (query length, reference length / 8, h0 / 32) and computes no L) is
// (query length, deficit) with deficit = qlen - (L - h0) / max_sc, the query bases the path behind L does not
// match: under the threshold a cell survives within about deficit / 2 columns of the diagonal, so the deficit is the pair's band width.
//
// Where the rule lives in bsw_dp8 (the 8-bit kernel; profiles/bsw_row_tail.md): score-only is a template argument, so the six-field
// form holds none of the above and the score-only form none of the six-field bookkeeping.  Behind a row's sweep the zero trim and
// both prunes are ONE evaluation of the two four-cell windows -- a zero cell is a dropped cell, so with `best` taken as 0 the
// prune's test is the reference's trim, and a lane whose prune is off (or whose left edge may not move) differs by an operand, not
// by a branch; whatever ends the pair in this row (z-drop, a guard, the exit's bound) is gathered in one flag and acted on once.
// bsw_dp<WIDE> keeps the rule in the order this comment states it.
//
// Roofline: integer-VALU / LDS bound (~20 VALU + 1 LDS read + 1 LDS write per DP cell,
// ~7.4 k cells per ~210 input bytes); HBM traffic is the algorithmic minimum
// len1 + len2 + 12 B per pair plus the 4-byte permutation entry.
#include "gab_internal.h"
#include <atomic>
#include <algorithm>
#include <new>
#include <string.h>
#include <time.h>
#include <stdlib.h>

namespace {

constexpr int kQBuckets = 256;            // query length 1..256 -> 0..255
constexpr int kTBuckets = 256;            // min(tlen >> 3, 255)
constexpr int kNumKeys = kQBuckets * kTBuckets;
constexpr int kClassStep = 16;            // query-length classes for LDS sizing
constexpr int kNumClasses = kQBuckets / kClassStep;
constexpr int kSlices = 2;                // a large batch is sorted in this many slices of its pair range (bsw_run_device_impl)
// The constants are measured (10 M read-like pairs, score-only).  kSortGridBeside with the seeded prune, profiles/bsw_seeded_prune.md
// (its figures below are of that time); kSlice0 and kSeedGridBeside again with the hop bound, profiles/bsw_hop_bound.md; kSliceMin
// was NOT measured again and is the value of profiles/bsw_slices.md.
//   kSlice0: slice 0's DP has to outlast slice 1's sort and the host's wait for it, and every pair of slice 0 sits in a small
//     launch (2^20 pairs in 8 classes are 2 300 waves each, little more than the chip holds at once).  With the hops bsw_seed of
//     slice 1 runs 3.7 ms beside slice 0's DP (1.0 ms with the ungapped bound).  Two runs per size, runs within 0.05 ms:
//     1 048 576 pairs 21.65 ms, 1 572 864 pairs 20.73, 2 097 152 pairs 20.39, 2 621 440 pairs 20.52, 3 145 728 pairs 20.72.
//     Too small and the GPU waits for slice 1's sort, too large and too many pairs sit in slice 0's small launches.
//   kSliceMin (before the seeded prune): a sliced call pays for sixteen class launches instead of eight and gains the sort of
//     slice 1.  It measured 0.23 ms faster than the unsliced call at 3 M pairs, 0.37 at 4 M, 0.46 at 6 M, 0.68 at 8 M; 2^22 is
//     the first size whose gain stood clear of the spread of the runs.
//   kSortGridBeside: medians of three runs, 64 workgroups 22.05 ms, 256 workgroups 21.66, 1 024 workgroups 21.76 (runs within
//     0.07 ms).  At 64 the histogram and the scatter of slice 1 outlast slice 0's DP; at 1 024 they take wave slots from it.
//   kSeedGridBeside: bsw_seed is VALU work like the DP and takes every wave slot it is given.  With the ungapped bound: 2 048
//     workgroups 22.32 ms per step (slice 0's class launches wait for it), 512 22.11, 256 22.63, 128 24.56 (the pass outlasts
//     slice 0's DP and the GPU waits for slice 1's sort).  With the hops, two runs each at kSlice0 = 1 572 864: 256 22.96, 512
//     20.73, 1 024 20.35 with runs 0.13 ms apart -- not clear of five times that, and the larger kSlice0 answers the same wait.
constexpr int64_t kSlice0 = 2097152;      // pairs in slice 0 of a sliced score-only call
constexpr int64_t kSlice0Full = 1 << 20;  // ... of a sliced six-field call: its sort has no scan in it, the value of profiles/bsw_slices.md stays
constexpr int64_t kSliceMin = 1 << 22;    // fewest pairs of a sliced call
constexpr int kSortGridBeside = 256;      // workgroups of bsw_hist / bsw_scatter when they run beside DP kernels
constexpr int kSeedGridBeside = 512;      // workgroups of bsw_seed (it only runs beside DP kernels: bsw_hist<true> makes L otherwise)
static_assert(kSliceMin >= (1 << 21) && kSlice0 < kSliceMin && kSlice0Full >= 64 * 8192 && kSlice0 >= kSlice0Full, "slice 0 has to fill the chip with its class launches, and calls below 2^21 pairs stay unsliced");

struct BswConst {
    int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w, max_sc;
    int32_t seed;         // economy gates of the seeded prune (header comment): bit 0 the threshold max(best, L - 1), bit 1 the prune of row -1
    uint32_t row_lo[5];   // biased (+128) scores mat[t][0..3], one byte each
    uint32_t row_hi[5];   // biased score mat[t][4] in byte 0
    int32_t hop;          // the matrix has bwa_fill_scmat's three-value form: the seed pass makes the hop bound, word-parallel
    int32_t hop_a, hop_mm, hop_n;   // ... its match, mismatch and N scores (hop_a > 0, neither of the others above it)
};

struct BswStats {          // device-side, zeroed per run
    unsigned long long cells;
    int32_t max_h0[kNumClasses];   // largest h0 per query-length class: the cell width of each class's DP launch depends on it
    int32_t bad;           // number of pairs that failed validation
    int32_t first_bad;     // smallest failing index + 1
};
GAB_STATIC_ATOMIC64(BswStats, cells);

struct BswIO {
    const uint8_t *ref; const int64_t *ref_off;
    const uint8_t *qry; const int64_t *qry_off;
    const int32_t *len1, *len2, *h0;
    int64_t ref_bytes, qry_bytes, n;
    int64_t ref_lo, qry_lo;        // lowest readable offset of the two slabs (0 for a caller's device slabs; the staged window's
                                   // start when gab_bsw_run has copied only the part of the host slabs it expects the pairs to use)
    int64_t ref_hi, qry_hi;        // end of the bytes that really hold the caller's data (= ref_bytes / qry_bytes for device slabs; the
};                                 // end of what gab_bsw_run COPIED: its window is padded to 256 bytes, and the padding is not the caller's data)

// (query length, deficit): deficit = qlen - (L - h0) / max_sc is the number of query bases that the path behind the
// seeded prune's lower bound L (bsw_seed) does NOT match, 0 for a perfect ungapped match.  Lanes of a wave then run the same number
// of rows, and bands of similar width: with thr = max(best, L - 1) a cell survives while it lies within about deficit / 2 columns of
// the diagonal.  On the read-like input the deficit alone predicts a pair's cell count (correlation 0.91; reference length and h0,
// the minor parts of the key before: 0.07 and 0.05); profiles/bsw_seeded_prune.md has the candidates this one was picked from.
// A six-field call (seeded == 0) has no exit and no prune: its rows are the reference's, as many as the reference is long, and its
// band starts as wide as h0 allows.  It keeps the key it had, (query length, reference length / 8, h0 / 32), and bsw_seed only
// validates for it: under the deficit key its step at 10 M pairs measured 47.1 ms against 39.3 (profiles/bsw_seeded_prune.md).
__device__ __forceinline__ int bsw_key(int qlen, int tlen, int h0, int L, int max_sc, int seeded) {
    if (!seeded) {
        int tb = tlen >> 3; if (tb > kTBuckets / 4 - 1) tb = kTBuckets / 4 - 1;
        int hc = h0 >> 5; if (hc > 3) hc = 3;
        return (qlen - 1) * kTBuckets + tb * 4 + hc;
    }
    int d = qlen - (L - h0) / (max_sc > 1 ? max_sc : 1);
    d = d < 0 ? 0 : d > kTBuckets - 1 ? kTBuckets - 1 : d;
    return (qlen - 1) * kTBuckets + d;
}

// A 151-bp read set puts almost all pairs into ~256 NEIGHBOURING keys (one query length), i.e. 1 KB of counters behind a
// handful of memory channels, and the histogram pass is bound by the atomic rate of those channels.  The counters are
// therefore stored at a multiplicatively scrambled index (a bijection on 16 bits): neighbouring keys lie 16 KB apart.
__device__ __forceinline__ int bsw_hslot(int key) { return (int)(((uint32_t)key * 4099u) & (uint32_t)(kNumKeys - 1)); }
static_assert((kNumKeys & (kNumKeys - 1)) == 0, "bsw_hslot needs a power-of-two key space");

__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}

// ---- pass 0: validate + the seeded prune's lower bound L per pair ---------------------------
// L (header comment): the ungapped extension from d = h0 along the main diagonal, stopped at the first d <= 0, every prefix held
// down by what a z-drop of the reference in an earlier row would still return -- and, for a matrix of bwa_fill_scmat's form, up to
// three one-gap hops from its peak (bsw_hop_bound below).  seed[i] = L, or -1 for a pair that fails the
// validation (L >= h0 >= 0 otherwise): bsw_hist and bsw_scatter read it instead of validating again.  One thread per pair reads both
// sequences; the pass issues no atomics, and beside the DP kernels of another slice its grid is kSeedGridBeside.
// (seeded == 0, a six-field call: validation only, L = h0; no sequence is read)
// Where it runs: a call's only sort, and slice 0's, have the GPU to themselves and make L inside bsw_hist<true> -- no launch of
// its own, which a batch of 100 000 pairs cannot hide -- while slice 1's sort runs beside slice 0's DP kernels, where the scan
// wants another grid than the histogram's atomics: bsw_seed, then bsw_hist<false>.
__device__ __forceinline__ void bsw_seed_mat(const BswConst &c, int *s_mat) {      // the 25 scores, for per-lane look-ups; the caller syncs
    if (threadIdx.x < 25) {
        const int t = threadIdx.x / 5, q = threadIdx.x % 5;
        s_mat[threadIdx.x] = (int)((q < 4 ? c.row_lo[t] >> (8 * q) : c.row_hi[t]) & 0xffu) - 128;
    }
}
// ---- the hop bound (header comment: "L with hops") --------------------------------------------
// The segments behind a hop are scanned by COUNTS, sixteen bases per trip from one 16-byte load per sequence, with no walk from
// base to base: the lanes of a wave hold different pairs, and a walk costs every lane what it costs the slowest.  e marks the
// bytes that do not score a match (the codes differ, or one is 4 or above: an N), nb the Ns among them; a chunk's mismatches and
// Ns are two population counts.  Nothing is read further than three bytes past either sequence's end: a chunk that would reach
// further is read in dwords, each only where it holds a base, and the bytes behind the segment's end are masked out.
struct BswHopSeg { int pk, kp, dk, mk; };      // the peak's worth (0: none), its step (1-based), d and mn there
__device__ __forceinline__ uint32_t bsw_nz_bytes(uint32_t y) { return (((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u; }   // bit 7 of every non-zero byte
// the next min(16, left) bases from t and q (left >= 1): e / nb per dword, bytes behind `left` cleared
__device__ __forceinline__ void bsw_hop_load(const uint8_t *t, const uint8_t *q, int left, uint32_t e[4], uint32_t nb[4]) {
    uint32_t tw[4], qw[4];
    if (left >= 13) {
        __builtin_memcpy(tw, t, 16);
        __builtin_memcpy(qw, q, 16);
    } else {
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const bool in = 4 * b < left;
            tw[b] = in ? load_u32_unaligned(t + 4 * b) : 0u;
            qw[b] = in ? load_u32_unaligned(q + 4 * b) : 0u;
        }
    }
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int vb = left - 4 * b;
        const uint32_t m = vb >= 4 ? ~0u : vb <= 0 ? 0u : (1u << (8 * vb)) - 1u;
        nb[b] = (tw[b] | qw[b]) & 0xfcfcfcfcu & m;
        e[b] = ((tw[b] ^ qw[b]) & m) | nb[b];
    }
}
// one chunk's rule (tools/gen/bsw_exit_model.c, hop_scan): cnt bases with nm mismatches and nn Ns behind state (d, mn); false and
// nothing changed when the chunk's lowest possible prefix is not positive
__device__ __forceinline__ bool bsw_hop_step(const BswConst &c, int cnt, int nm, int nn, int end, int &d, int &mn, BswHopSeg &s) {
    const int dm = c.hop_mm < 0 ? -c.hop_mm : 0, dn = c.hop_n < 0 ? -c.hop_n : 0;
    const int low = d - nm * dm - nn * dn;
    if (low <= 0) return false;
    d += cnt * c.hop_a - nm * (c.hop_a - c.hop_mm) - nn * (c.hop_a - c.hop_n);
    mn = low < mn ? low : mn;
    int v = d;
    if (c.zdrop > 0 && d - mn > c.zdrop) v = c.zdrop + 1 + mn;
    if (v > s.pk) { s.pk = v; s.kp = end; s.dk = d; s.mk = mn; }
    return true;
}
// t, q: the segment's first bases; n: the bases the shorter of the two still has (may be <= 0); d > 0, mn <= d
__device__ __forceinline__ BswHopSeg bsw_hop_scan(const BswConst &c, const uint8_t *t, const uint8_t *q, int n, int d, int mn) {
    BswHopSeg s; s.pk = 0; s.kp = 0; s.dk = d; s.mk = mn;
    uint32_t e[4], nb[4];
    bool live = true;
#pragma unroll 1
    for (int k = 0; k < n && live; k += 16) {
        bsw_hop_load(t + k, q + k, n - k, e, nb);
        const int cnt = n - k < 16 ? n - k : 16;
        int ne = 0, nn = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) ne += __popc(bsw_nz_bytes(e[b]));
        if ((nb[0] | nb[1] | nb[2] | nb[3]) != 0u) {
#pragma unroll
            for (int b = 0; b < 4; b++) nn += __popc(bsw_nz_bytes(nb[b]));
        }
        live = bsw_hop_step(c, cnt, ne - nn, nn, k + cnt, d, mn, s);
        if (c.zdrop > 0 && s.pk == c.zdrop + 1 + mn) live = false;    // the cap is reached: no later step can be worth more
    }
    // behind the peak's chunk: the next sixteen bases in steps of four, then the run of matches in front of the next marked byte
    const int base = s.kp, left = n - base < 16 ? n - base : 16;
    if (left >= 1) {
        bsw_hop_load(t + base, q + base, left, e, nb);
        d = s.dk; mn = s.mk;
        live = true;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int cnt = left - 4 * b < 4 ? left - 4 * b : 4;
            if (live && cnt > 0) {
                const int nn = __popc(bsw_nz_bytes(nb[b]));
                live = bsw_hop_step(c, cnt, __popc(bsw_nz_bytes(e[b])) - nn, nn, base + 4 * b + cnt, d, mn, s);
            }
        }
        const int o = s.kp - base;                          // 0, 4, 8, 12 -- or `left`, the end of the window
        if (o < left) {
            const uint32_t eo = o == 0 ? e[0] : o == 4 ? e[1] : o == 8 ? e[2] : e[3];
            const int cnt = left - o < 4 ? left - o : 4;
            int lead = eo ? __builtin_ctz(bsw_nz_bytes(eo)) >> 3 : 4;
            lead = lead < cnt ? lead : cnt;
            const int d2 = s.dk + lead * c.hop_a;
            int v = d2;
            if (c.zdrop > 0 && d2 - s.mk > c.zdrop) v = c.zdrop + 1 + s.mk;
            if (lead > 0 && v > s.pk) { s.pk = v; s.kp += lead; s.dk = d2; }
        }
    }
    return s;
}

// L of one pair from the main diagonal's scan (L, its peak step kp, the minimum mk up to there): at most kHops times the one
// candidate of nine around the current segment's peak whose first chunk ends highest (header comment; tools/gen/bsw_exit_model.c,
// hop_bound, is the same rule).
constexpr int kHops = 3, kHopEvents = 4;
__device__ __forceinline__ int bsw_hop_bound(const BswConst &c, const uint8_t *t, int tl, const uint8_t *q, int ql, int L, int kp, int mk) {
    int si = 0, sj = 0, dk = L;
    // the band gate |i - j| <= w of the pair's clamped w: dist <= lim with lim = max(1, (int)(x / e + 1.)) holds iff dist <= 1 or
    // x >= (dist - 1) * e -- no division
    const int xi = ql * c.max_sc + c.end_bonus - c.o_ins, xd = ql * c.max_sc + c.end_bonus - c.o_del;
    const int dm = c.hop_mm < 0 ? -c.hop_mm : 0, dn = c.hop_n < 0 ? -c.hop_n : 0;
#pragma unroll 1
    for (int hop = 0; hop < kHops; hop++) {
        if (c.zdrop > 0 && L - mk > c.zdrop) break;         // the peak is held down by the cap (dk == L otherwise): no candidate's cap is higher
        int bestv = 0, bi = 0, bj = 0, bd = 0, dd = dk;
#pragma unroll 1
        for (int back = 0; back <= 8; back += 4) {
            const int cs = kp - back;                       // the start's step in its segment: (c) at least one diagonal step in
            if (cs < 1) break;
            if (back) {                                     // d at step cs: take back the scores of steps cs + 1 .. cs + 4
                const uint32_t tw = load_u32_unaligned(t + si + cs), qw = load_u32_unaligned(q + sj + cs);
                const uint32_t nb = (tw | qw) & 0xfcfcfcfcu, e = (tw ^ qw) | nb;
                dd -= 4 * c.hop_a + __popc(bsw_nz_bytes(e)) * (c.hop_mm - c.hop_a) + __popc(bsw_nz_bytes(nb)) * (c.hop_n - c.hop_mm);
            }
            const int ci = si + cs, cj = sj + cs;
#pragma unroll 1
            for (int g = 0; g < 3; g++) {                   // 1 or 2 reference bases deleted, 1 query base inserted
                const int ni = g < 2 ? ci + g + 1 : ci, nj = g < 2 ? cj : cj + 1;
                const int nd = g < 2 ? dd - c.o_del - (g + 1) * c.e_del : dd - c.o_ins - c.e_ins;
                const int dist = ni > nj ? ni - nj : nj - ni;
                const bool band = dist <= c.w && (dist <= 1 || (xi >= (dist - 1) * c.e_ins && xd >= (dist - 1) * c.e_del));
                int left = tl - ni < ql - nj ? tl - ni : ql - nj;
                if (nd <= 0 || !band || left < 1) continue; // (a) a positive value, (b) inside the band
                left = left < 16 ? left : 16;
                uint32_t e[4], nb[4];
                bsw_hop_load(t + ni, q + nj, left, e, nb);
                int ne = 0, nn = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) { ne += __popc(bsw_nz_bytes(e[b])); nn += __popc(bsw_nz_bytes(nb[b])); }
                if (ne > kHopEvents || nd - (ne - nn) * dm - nn * dn <= 0) continue;
                const int val = nd + left * c.hop_a - (ne - nn) * (c.hop_a - c.hop_mm) - nn * (c.hop_a - c.hop_n);
                if (val > bestv) { bestv = val; bi = ni; bj = nj; bd = nd; }
            }
        }
        if (bestv == 0) break;
        const BswHopSeg s = bsw_hop_scan(c, t + bi, q + bj, tl - bi < ql - bj ? tl - bi : ql - bj, bd, mk < bd ? mk : bd);
        if (s.pk <= L) break;
        L = s.pk; si = bi; sj = bj; kp = s.kp; dk = s.dk; mk = s.mk;
    }
    return L;
}

__device__ __forceinline__ int bsw_seed_of(const BswIO &io, const BswConst &c, const int *s_mat, int seeded, int64_t i) {
    {
        const int ql = io.len2[i], tl = io.len1[i], h = io.h0[i];
        const int64_t ro = io.ref_off[i], qo = io.qry_off[i];
        const bool ok = ql >= 1 && ql <= GAB_BSW_MAX_QLEN && tl >= 1 && tl <= GAB_BSW_MAX_TLEN && h >= 0 &&
                        h <= (1 << 29) && ro >= io.ref_lo && qo >= io.qry_lo &&
                        ro + tl + 3 <= io.ref_bytes && qo + ql + 3 <= io.qry_bytes &&   // (the kernels read dwords from the sequence's own start)
                        ro + tl <= io.ref_hi && qo + ql <= io.qry_hi;
        if (!ok) return -1;
        if (!seeded) return h;                              // (wave-uniform)
        const uint8_t *const t = io.ref + ro, *const q = io.qry + qo;
        const int n = ql < tl ? ql : tl;
        int d = h, L = h, mn = h, kp = 0, mk = h;              // kp: the first step (1-based) worth L; mk: the minimum of d_0 .. d_kp
        bool live = h > 0;                                  // the scan goes on: no d <= 0 so far and bases left
        for (int k = 0; k < n && live; k += 16) {
            uint32_t tw[4], qw[4];
            if (k + 16 <= n + 3) {                          // one 16-byte load per sequence: a quarter of the cache-line requests
                __builtin_memcpy(tw, t + k, 16);
                __builtin_memcpy(qw, q + k, 16);
            } else {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const bool in = k + 4 * b < n;
                    tw[b] = in ? load_u32_unaligned(t + k + 4 * b) : 0u;
                    qw[b] = in ? load_u32_unaligned(q + k + 4 * b) : 0u;
                }
            }
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const uint32_t tc = (tw[b >> 2] >> (8 * (b & 3))) & 0xffu, qc = (qw[b >> 2] >> (8 * (b & 3))) & 0xffu;
                const int nd = d + s_mat[(tc < 4u ? tc : 4u) * 5u + (qc < 4u ? qc : 4u)];
                live = live && k + b < n && nd > 0;
                if (live) {
                    d = nd;
                    int v = d;
                    if (c.zdrop > 0 && d - mn > c.zdrop) v = c.zdrop + 1 + mn;
                    mn = d < mn ? d : mn;
                    if (v > L) { L = v; kp = k + b + 1; mk = mn; }
                }
            }
        }
        return c.hop && kp > 0 ? bsw_hop_bound(c, t, tl, q, ql, L, kp, mk) : L;
    }
}
__global__ __launch_bounds__(256) void bsw_seed(BswIO io, BswConst c, int seeded, int64_t lo, int64_t hi, int32_t *__restrict__ seed) {
    __shared__ int s_mat[25];
    bsw_seed_mat(c, s_mat);
    __syncthreads();
    int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < hi; i += stride) seed[i] = bsw_seed_of(io, c, s_mat, seeded, i);
}

// ---- pass 1: histogram -----------------------------------------------------------------------
// The value the histogram atomic returns is the pair's rank inside its bucket: it is kept, so that the scatter pass
// needs no second round of 10 M atomics (each pass was atomic-throughput bound at ~13 G/s).
// Pairs lo .. hi - 1 of the batch (one slice of it, or all): hist and st are the slice's own, rank is indexed by the pair.
// FUSED: the pass makes seed[i] itself (pass 0 above) instead of reading what bsw_seed wrote.
template <bool FUSED>
__global__ __launch_bounds__(256) void bsw_hist(BswIO io, BswConst c, int seeded, int64_t lo, int64_t hi, int32_t *seed,
                                                uint32_t *hist, uint32_t *rank, BswStats *st) {
    __shared__ int cls_h0[kNumClasses];      // largest h0 per query-length class among this workgroup's pairs
    __shared__ int s_mat[25];
    const int max_sc = c.max_sc;
    if (threadIdx.x < kNumClasses) cls_h0[threadIdx.x] = 0;
    if (FUSED) bsw_seed_mat(c, s_mat);
    __syncthreads();
    int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < hi; i += stride) {
        const int L = FUSED ? bsw_seed_of(io, c, s_mat, seeded, i) : seed[i];
        if (FUSED) seed[i] = L;            // (bsw_scatter and the records read it)
        if (L < 0) {                       // failed the validation of pass 0
            atomicAdd(&st->bad, 1);
            atomicMin((unsigned int *)&st->first_bad, (unsigned int)(i + 1 > 0x7fffffff ? 0x7fffffff : i + 1));
            rank[i] = ~0u;                 // (the scatter pass is already queued behind this one: it must not place this pair)
            continue;
        }
        const int ql = io.len2[i], h = io.h0[i];
        const int tl = seeded ? 0 : io.len1[i];             // (the seeded key does not read it)
        if (h > 0) atomicMax(&cls_h0[(ql - 1) / kClassStep], h);
        rank[i] = atomicAdd(&hist[bsw_hslot(bsw_key(ql, tl, h, L, max_sc, seeded))], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kNumClasses && cls_h0[threadIdx.x] > 0) atomicMax(&st->max_h0[threadIdx.x], cls_h0[threadIdx.x]);
}

// ---- pass 2: exclusive scan of the 65536 bins ----------------------------------------------
// Two launches of 64 workgroups: (a) every thread takes ONE bin -- the counters sit at scrambled slots, so a thread that
// walks 64 consecutive bins pays 128 scattered loads one after the other (a single workgroup doing that took 113 us,
// 9 % of a 100 000-pair batch) -- and the workgroup scans its 1024 bins; (b) adds the totals of the workgroups in front.
constexpr int kScanBlocks = kNumKeys / 1024;
static_assert(kScanBlocks == 64, "bsw_scan_b reduces the block totals with one wave");
__global__ __launch_bounds__(1024) void bsw_scan_a(const uint32_t *__restrict__ hist, uint32_t *__restrict__ start, uint32_t *__restrict__ sums) {
    __shared__ uint32_t wsum[16];
    const int t = threadIdx.x, key = blockIdx.x * 1024 + t, lane = t & 63, wv = t >> 6;
    const uint32_t v = hist[bsw_hslot(key)];
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < wv; k++) before += wsum[k];
    start[key] = before + inc - v;
    if (t == 1023) sums[blockIdx.x] = before + inc;
}
__global__ __launch_bounds__(1024) void bsw_scan_b(uint32_t *__restrict__ start, const uint32_t *__restrict__ sums, uint32_t *__restrict__ qstart) {
    __shared__ uint32_t s_off, s_total;
    const int t = threadIdx.x, key = blockIdx.x * 1024 + t;
    if (t < 64) {
        const uint32_t sv = sums[t];
        uint32_t mine = t < (int)blockIdx.x ? sv : 0, all = sv;
        for (int o = 32; o > 0; o >>= 1) { mine += __shfl_xor(mine, o); all += __shfl_xor(all, o); }
        if (t == 0) { s_off = mine; s_total = all; }
    }
    __syncthreads();
    const uint32_t run = start[key] + s_off;
    start[key] = run;
    if ((key % kTBuckets) == 0) qstart[key / kTBuckets] = run;
    if (key == kNumKeys - 1) { start[kNumKeys] = s_total; qstart[kQBuckets] = s_total; }
}

// ---- pass 3: scatter the pairs' descriptors into bucket order -------------------------------
// One 32-byte record per pair, written here from coalesced reads of the five input arrays and read coalesced by the DP
// kernels: the DP kernels used to gather the five fields through the permutation (five random 64-byte sectors per pair,
// 3.2 GB of the 7.6 GB the DP fetched per 10 M pairs against 2.1 GB of algorithmic bytes).
// (lens = len1 | len2 << 16: len1 <= GAB_BSW_MAX_TLEN < 2^15, len2 <= GAB_BSW_MAX_QLEN; L is bsw_seed's)
struct __attribute__((aligned(32))) BswRec { int64_t ref_off, qry_off; int32_t lens, h0, L; uint32_t id; };
static_assert(sizeof(BswRec) == 32 && GAB_BSW_MAX_TLEN < (1 << 16) && GAB_BSW_MAX_QLEN < (1 << 15), "BswRec packs both lengths into one word");

// (pairs lo .. hi - 1 as in bsw_hist; start counts from the slice's first record, recs is where the slice's records begin, and
// rec.id stays the pair's index in the whole batch)
__global__ __launch_bounds__(256) void bsw_scatter(BswIO io, int max_sc, int seeded, int64_t lo, int64_t hi, const int32_t *__restrict__ seed,
                                                   const uint32_t *__restrict__ start, const uint32_t *__restrict__ rank, BswRec *recs) {
    int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < hi; i += stride) {
        int ql = io.len2[i], tl = io.len1[i];
        if (rank[i] == ~0u) continue;      // failed bsw_seed's validation (the host returns GAB_EINVAL after this pass)
        BswRec r;
        r.ref_off = io.ref_off[i]; r.qry_off = io.qry_off[i]; r.lens = tl | ql << 16; r.h0 = io.h0[i]; r.L = seed[i]; r.id = (uint32_t)i;
        recs[start[bsw_key(ql, tl, r.h0, r.L, max_sc, seeded)] + rank[i]] = r;
    }
}

// ---- pass 4: the DP ------------------------------------------------------------------------

// WIDE = false: H and E packed as (E << 16) | H in one dword per column (both < 2^15).
// WIDE = true : H at lds[j*64+lane], E at lds[(qcap+1+j)*64+lane].
template <bool WIDE>
__global__ __launch_bounds__(64) void bsw_dp(BswIO io, BswConst c, const BswRec *__restrict__ recs,
                                            int64_t kbeg, int64_t kend, int qcap,
                                            int32_t *__restrict__ score_out,
                                            gab_bsw_result *__restrict__ result_out, BswStats *st) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const int64_t k = kbeg + (int64_t)(gridDim.x - 1 - blockIdx.x) * 64 + lane;   // heaviest waves (largest key) first
    const bool valid = k < kend;
    BswRec rec; rec.ref_off = rec.qry_off = 0; rec.lens = rec.h0 = rec.L = 0; rec.id = 0u;
    if (valid) rec = recs[k];
    const uint32_t id = rec.id;

    uint32_t *const H = lds + lane;                                   // [j*64]
    uint32_t *const E = lds + (size_t)(qcap + 1) * 64 + lane;         // WIDE only
    uint8_t *const QC = reinterpret_cast<uint8_t *>(lds + (size_t)(WIDE ? 2 : 1) * (qcap + 1) * 64) + lane * 4;
    // query code j of this lane: QC[(j >> 2) * 256 + (j & 3)]

    unsigned long long cells = 0;
    if (valid) {
        const int qlen = rec.lens >> 16, tlen = rec.lens & 0xffff, h0 = rec.h0;
        const uint8_t *q = io.qry + rec.qry_off;
        const uint8_t *t = io.ref + rec.ref_off;
        const int oe_del = c.o_del + c.e_del, oe_ins = c.o_ins + c.e_ins;
        const int e_del = c.e_del, e_ins = c.e_ins;

        for (int w4 = 0; w4 * 4 < qlen; w4++)
            *reinterpret_cast<uint32_t *>(QC + w4 * 256) = load_u32_unaligned(q + w4 * 4);

        // band clamp (bandedSWA.cpp:164-172)
        int w = c.w;
        {
            int lim = (int)((double)(qlen * c.max_sc + c.end_bonus - c.o_ins) / e_ins + 1.);
            lim = lim > 1 ? lim : 1; w = w < lim ? w : lim;
            lim = (int)((double)(qlen * c.max_sc + c.end_bonus - c.o_del) / e_del + 1.);
            lim = lim > 1 ? lim : 1; w = w < lim ? w : lim;
        }
        const bool score_only = result_out == nullptr;      // wave-uniform: the early exit and the two prunes of the header comment apply
        // the prunes need every cell that row 0's band clamp leaves behind to be zero, and a z-drop that rarely sends pairs back (header comment)
        bool prune = score_only && (qlen <= w + 1 || h0 - oe_ins - (w + 1) * e_ins <= 0) && (c.zdrop == 0 || c.zdrop >= 8 * c.max_sc);
        int best, best_i, best_j, g_i, gscore, max_off;
      for (;;) {                                            // second trip: a pair one of the guards sent back, prunes off
        // row -1 (bandedSWA.cpp:159-161); E starts at 0 everywhere
        {
            int prev = h0;
            for (int j = 0; j <= qlen; j++) {
                int v;
                if (j == 0) v = h0;
                else if (j == 1) v = h0 > oe_ins ? h0 - oe_ins : 0;
                else v = prev > e_ins ? prev - e_ins : 0;
                prev = v;
                H[j * 64] = (uint32_t)v;
                if (WIDE) E[j * 64] = 0u;
            }
        }
        best = h0; best_i = -1; best_j = -1; g_i = -1; gscore = -1; max_off = 0;
        int beg = 0, end = qlen;
        int stale_pot = 0;                                  // bound on what the cells the band clamp cut can still lead to
        bool dropped = false, abandon = false;              // a prune has dropped a live cell; one of the three guards fired
        // seeded prune (header comment): the prunes and two of the guards test against thr = max(best, Lm1); 0 leaves thr == best
        const bool seed_ok = prune && min(qlen, 2 * w + 1) > 9;      // (a band that can hold more than nine cells)
        const int Lm1 = seed_ok && (c.seed & 1) ? rec.L - 1 : 0;
        if (seed_ok && (c.seed & 2)) {                      // the prune of row -1: cell 0 stays
            const int thr = max(best, Lm1);
            int jl = qlen;
            for (; jl >= 1; jl--) {
                const int m = (int)H[jl * 64];              // (E = 0)
                if (m && m + c.max_sc * min(tlen, qlen - jl) > thr) break;
                H[jl * 64] = 0u;
            }
            end = jl + 2 < qlen ? jl + 2 : qlen;
            dropped = end < min(qlen, w + 1);               // the reference sweeps row 0 up to there
        }
        uint32_t tw = load_u32_unaligned(t);       // 4 reference bases, refreshed every 4 rows
        for (int i = 0; i < tlen; i++) {
            const int tc = (tw >> ((i & 3) * 8)) & 0xff;
            if ((i & 3) == 3 && i + 1 < tlen) tw = load_u32_unaligned(t + i + 1);
            // biased score bytes for this reference base (codes >= 4 are N)
            uint32_t rlo = c.row_lo[4], rhi = c.row_hi[4];
            rlo = tc == 0 ? c.row_lo[0] : rlo; rhi = tc == 0 ? c.row_hi[0] : rhi;
            rlo = tc == 1 ? c.row_lo[1] : rlo; rhi = tc == 1 ? c.row_hi[1] : rhi;
            rlo = tc == 2 ? c.row_lo[2] : rlo; rhi = tc == 2 ? c.row_hi[2] : rhi;
            rlo = tc == 3 ? c.row_lo[3] : rlo; rhi = tc == 3 ? c.row_hi[3] : rhi;

            if (beg < i - w) beg = i - w;
            if (end > i + w + 1) { end = i + w + 1; stale_pot = max(stale_pot, best + c.max_sc * (qlen - end)); }
            if (end > qlen) end = qlen;
            const int beg0 = beg, end0 = end;               // the band this row is swept with: either prune moves its edge by at most four cells
            int hleft = 0;
            if (beg == 0) { hleft = h0 - (c.o_del + e_del * (i + 1)); hleft = hleft > 0 ? hleft : 0; }
            int f = 0;
            uint32_t rowpk = 0;           // (row max << 16) | column, max over the row; ties -> later column
            int rowmax32 = 0, rowmax_j = -1;
            int j = beg;
            for (; j < end; j++) {
                int diag, e;
                if (WIDE) { diag = (int)H[j * 64]; e = (int)E[j * 64]; }
                else { uint32_t v = H[j * 64]; diag = (int)(v & 0xffffu); e = (int)(v >> 16); }
                uint32_t qc = QC[(j >> 2) * 256 + (j & 3)];
                qc = qc > 4u ? 4u : qc;
                int sc = (int)__builtin_amdgcn_perm(rhi, rlo, qc | 0x0c0c0c00u) - 128;
                int M = diag ? diag + sc : 0;
                int h = max(max(M, e), f);
                int t1 = M - oe_del; t1 = t1 > 0 ? t1 : 0;
                int en = e - e_del; en = en > t1 ? en : t1;
                if (WIDE) { H[j * 64] = (uint32_t)hleft; E[j * 64] = (uint32_t)en; }
                else H[j * 64] = (uint32_t)hleft | ((uint32_t)en << 16);
                hleft = h;
                if (WIDE) {
                    if (!(rowmax32 > h)) rowmax_j = j;
                    rowmax32 = h > rowmax32 ? h : rowmax32;
                } else {
                    uint32_t pk = ((uint32_t)h << 16) | (uint32_t)j;
                    rowpk = pk > rowpk ? pk : rowpk;
                }
                int t2 = M - oe_ins; t2 = t2 > 0 ? t2 : 0;
                f -= e_ins; f = f > t2 ? f : t2;
            }
            cells += (unsigned)(end > beg ? end - beg : 0);
            int rowmax;
            if (WIDE) rowmax = rowmax32;
            else { rowmax = (int)(rowpk >> 16); rowmax_j = end > beg ? (int)(rowpk & 0xffffu) : -1; }
            if (WIDE) { H[end * 64] = (uint32_t)hleft; E[end * 64] = 0u; }
            else H[end * 64] = (uint32_t)hleft;
            if (j == qlen) {
                if (!(gscore > hleft)) g_i = i;
                gscore = hleft > gscore ? hleft : gscore;
            }
            if (rowmax == 0) {                              // zero-row guard of the right prune (header comment, step 10)
                if (dropped && beg == 0) {
                    const int hb = h0 - c.o_del - e_del * (i + 1);              // this row's left edge: stored cell 0
                    abandon = hb > 0 && hb + c.max_sc * min(tlen - 1 - i, qlen) > max(best, Lm1);
                }
                break;
            }
            const int rows_left = tlen - 1 - i;
            bool try_exit = false;
            if (rowmax > best) {
                best = rowmax; best_i = i; best_j = rowmax_j;
                int off = rowmax_j - i; off = off < 0 ? -off : off;
                max_off = off > max_off ? off : max_off;
            } else {
                if (c.zdrop > 0) {
                    if (dropped && rowmax < best - c.zdrop) { abandon = true; break; }     // the reference's row maximum may differ here
                    int di = i - best_i, dj = rowmax_j - best_j;
                    if (di > dj) { if (best - rowmax - (di - dj) * e_del > c.zdrop) break; }
                    else { if (best - rowmax - (dj - di) * e_ins > c.zdrop) break; }
                }
                // the row maximum's own potential: while it exceeds best no exit is possible and the bound pass is skipped
                try_exit = score_only && rowmax + c.max_sc * min(rows_left, qlen - 1 - rowmax_j) <= best;
            }
            const int thr = max(best, Lm1);                 // (best is this row's already)
            // right-edge guard of the left prune (header comment, step 5)
            if (dropped && end < qlen && end != i + w + 1 && hleft > e_ins &&
                hleft - e_ins + c.max_sc * min(rows_left, qlen - end - 1) > thr) { abandon = true; break; }
            // trim all-zero cells from both band edges (bandedSWA.cpp:234-237)
            if (WIDE) {
                for (j = beg; j < end && H[j * 64] == 0u && E[j * 64] == 0u; j++) {}
                beg = j;
                for (j = end; j >= beg && H[j * 64] == 0u && E[j * 64] == 0u; j--) {}
            } else {
                for (j = beg; j < end && H[j * 64] == 0u; j++) {}
                beg = j;
                for (j = end; j >= beg && H[j * 64] == 0u; j--) {}
            }
            int jl = j;                                     // the last live stored cell (beg - 1: none)
            end = j + 2 < qlen ? j + 2 : qlen;
            if (prune && beg < end) {                       // left prune: cell beg is live here, the zero trim stopped at it
                bool go = true;
                if (beg == 0) {
                    const int hb = h0 - c.o_del - e_del * (i + 2);
                    go = hb <= 0 || hb + c.max_sc * min(rows_left, qlen) <= thr;
                }
                if (go) {
                    const int lcap = min(end, beg0 + 4);
                    for (j = beg; j < lcap; j++) {
                        const int m = WIDE ? max((int)H[j * 64], (int)E[j * 64]) : max((int)(H[j * 64] & 0xffffu), (int)(H[j * 64] >> 16));
                        if (m && m + c.max_sc * min(rows_left, qlen - j) > thr) break;
                    }
                    dropped = dropped || j > beg;
                    beg = j;
                }
            }
            if (prune && jl >= beg) {                       // right prune: cell jl is live here; dropped cells are zeroed (header comment)
                const int from = jl;
                for (; jl >= beg && jl > end0 - 4; jl--) {
                    const int m = WIDE ? max((int)H[jl * 64], (int)E[jl * 64]) : max((int)(H[jl * 64] & 0xffffu), (int)(H[jl * 64] >> 16));
                    if (m && m + c.max_sc * min(rows_left, qlen - jl) > thr) break;
                    H[jl * 64] = 0u;
                    if (WIDE) E[jl * 64] = 0u;
                }
                if (jl < from) { dropped = true; end = jl + 2 < qlen ? jl + 2 : qlen; }
            }
            if (try_exit) {
                int bound = stale_pot;
                if (beg == 0) {
                    const int hb = h0 - c.o_del - e_del * (i + 2);
                    if (hb > 0) bound = max(bound, hb + c.max_sc * min(rows_left, qlen));
                }
                for (j = beg; j <= end && bound <= best; j++) {
                    const int hd = WIDE ? (int)H[j * 64] : (int)(H[j * 64] & 0xffffu);
                    if (hd) bound = max(bound, hd + c.max_sc * min(rows_left, qlen - j));
                }
                if (bound <= best) break;
            }
        }
        if (!abandon) break;
        prune = false;
      }
        score_out[id] = best;
        if (result_out) {
            gab_bsw_result r;
            r.score = best; r.qle = best_j + 1; r.tle = best_i + 1;
            r.gtle = g_i + 1; r.gscore = gscore; r.max_off = max_off;
            result_out[id] = r;
        }
    }
    // one atomic per wave for the cell counter
    for (int o = 32; o > 0; o >>= 1) cells += __shfl_xor(cells, o);
    if (lane == 0 && cells) atomicAdd(&st->cells, cells);
}


// ---- pass 4b: the DP with 8-bit cells, two columns per step ---------------------------------------------------
// Used for a query-length class when max(h0) + qcap * max(mat) <= 255 (true for the whole 151-bp read workload):
// every H/E value then fits a byte, a column is a u16 (E << 8 | H) and TWO columns share one LDS dword, so the
// row needs half the LDS (7 waves per CU at 128 columns instead of 3) and the inner loop one LDS read and one
// LDS write per two cells.  Query codes are nibbles, two per byte.  The band may start or end in the middle of a
// dword: those single cells are handled with 16-bit LDS accesses so that cells outside the band keep their stale
// contents, which later rows may read when the band grows (bandedSWA.cpp:217,234-237).
//   lds layout: [ (qcap + 2) / 2 dwords of cells ][ ((qcap + 1) / 2 + 3) / 4 dwords of query nibbles ]  x 64 lanes
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ s16x2 pk_splat(int v) { s16x2 r; r.x = (short)v; r.y = (short)v; return r; }
// Packed 16-bit instructions the compiler does not form by itself: the x {0,1} product (as a C multiply it becomes
// compare + select per half), the u16 min, and the op_sel forms that route one half of a register to the other
// half of the result.  They are plain (non-volatile) asm so the scheduler may still move them.
// The packed max, min and saturating subtract ARE formed from the vector builtins, one instruction each, and are written that
// way: the compiler counts no wait state across an inline-asm statement and takes every asm result for a partial (dst_sel)
// write, so a chain of asm leaves got an s_nop wherever a reader followed within asm leaves only (profiles/bsw_row_edges.md).
__device__ __forceinline__ uint32_t pk_mul_lo(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
    return as_u32(__builtin_elementwise_max(as_s16x2(a), as_s16x2(b)));
}
__device__ __forceinline__ uint32_t pk_subsat_u16_k(uint32_t a, uint32_t k) {    // max(half - k, 0), unsigned halves
    return as_u32(__builtin_elementwise_sub_sat(as_u16x2(a), as_u16x2(k)));
}
__device__ __forceinline__ uint32_t pk_subsat_u16_v(uint32_t a, uint32_t b) {    // max(half of a - half of b, 0), unsigned halves
    return as_u32(__builtin_elementwise_sub_sat(as_u16x2(a), as_u16x2(b)));
}
__device__ __forceinline__ uint32_t and_or_b32(uint32_t a, uint32_t mask, uint32_t k) {   // (a & mask) | k, mask uniform
    uint32_t r; asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(mask), "v"(k)); return r;
}
__device__ __forceinline__ uint32_t pk_max_i16_0(uint32_t a) {
    uint32_t r; asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(a)); return r;
}
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    return as_u32(__builtin_elementwise_min(as_u16x2(a), as_u16x2(b)));
}
__device__ __forceinline__ uint32_t pk_min_u16_1(uint32_t a) {                    // min(half, 1) on both halves
    uint32_t r; asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(r) : "v"(a)); return r;
}
// Non-packed 16-bit / 32-bit instructions of the 2-cycle class (profiles/r02_valu_issue.md), all operands in VGPRs.  On gfx9
// a 16-bit VOP2 instruction reads the low halves of its sources and writes zero to the upper half of its destination.
__device__ __forceinline__ uint32_t max_i16_lo(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ uint32_t shr16(uint32_t a) {
    uint32_t r; asm("v_lshrrev_b32 %0, 16, %1" : "=v"(r) : "v"(a)); return r;
}
__device__ __forceinline__ uint32_t add_u32_v(uint32_t a, uint32_t b) {
    uint32_t r; asm("v_add_u32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
typedef __attribute__((address_space(3))) uint32_t bsw_lds_u32;       // 32-bit LDS pointers: one VGPR, so that inline assembly can bump them
typedef __attribute__((address_space(3))) const uint8_t bsw_lds_u8;
__device__ __forceinline__ uint32_t max_i16_hi_lo(uint32_t a, uint32_t b) {      // max(upper half of a, low half of b) -> low half, upper half zero
    uint32_t r; asm("v_max_i16_sdwa %0, %1, %2 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0" : "=v"(r) : "v"(a), "v"(b)); return r;
}
// The per-row products as 24-bit multiplies (v_mul_i32_i24 / v_mad_i32_i24, profiles/bsw_row_edges.md): both operands lie inside
// +-2^23 and the product inside 32 bits at every use -- max_sc <= 127, column counts <= qcap <= 256, row counts and |di - dj|
// <= GAB_BSW_MAX_TLEN + 256 < 2^16, gap penalties < 2^15.
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }
// The F step of the carry chain, max(t, f - e_ins), as one leaf per column: the subtraction's result has one reader, so the pair
// needs no register of its own and is one unit for the scheduler.  Neither instruction selects a part of its destination, so the
// second may read the first one's result in the next issue slot (no wait state between them).
__device__ __forceinline__ uint32_t f_step_lo(uint32_t t, uint32_t f, uint32_t e) {        // max(low half of t, f - e) -> low half
    uint32_t r; asm("v_sub_u16 %0, %2, %3\n\tv_max_i16 %0, %1, %0" : "=&v"(r) : "v"(t), "v"(f), "v"(e)); return r;
}
__device__ __forceinline__ uint32_t f_step_hi(uint32_t t, uint32_t f, uint32_t e) {        // max(upper half of t, f - e) -> low half
    uint32_t r;
    asm("v_sub_u16 %0, %2, %3\n\tv_max_i16_sdwa %0, %1, %0 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0"
        : "=&v"(r) : "v"(t), "v"(f), "v"(e));
    return r;
}
// The row-maximum key of a loop trip folded into the running key: max(key, max(a, b, c) << 16 | j), a, b and c in low halves.
__device__ __forceinline__ uint32_t rowkey_fold(uint32_t key, uint32_t a, uint32_t b, uint32_t c, uint32_t j) {
    uint32_t t;
    asm("v_max_i16 %1, %2, %3\n\tv_max_i16 %1, %1, %4\n\tv_lshl_or_b32 %1, %1, 16, %5\n\tv_max_u32 %0, %0, %1"
        : "+v"(key), "=&v"(t) : "v"(a), "v"(b), "v"(c), "v"(j));
    return key;
}
struct BswCellOut { int h, en, f; };
__device__ __forceinline__ BswCellOut bsw_cell(int diag, int e, int f, uint32_t qc, uint32_t rlo, uint32_t rhi, int oe_del,
                                               int e_del, int oe_ins, int e_ins) {
    const int sc = (int)__builtin_amdgcn_perm(rhi, rlo, qc | 0x0c0c0c00u) - 128;
    const int M = diag ? diag + sc : 0;
    BswCellOut o;
    o.h = max(max(M, e), f);
    o.en = max(max(M - oe_del, e - e_del), 0);
    o.f = max(max(M - oe_ins, f - e_ins), 0);
    return o;
}

// SYM: o_del + e_del == o_ins + e_ins (BWA-MEM's defaults): M - (o + e) is the same value for the E and the F source.
// MS1: no score above 1 (BWA-MEM's a = 1): for diag >= 1, M <= diag + 1 <= 2 diag, so "diag == 0 -> M = 0" is min(M, 2 diag).
// SO : score-only call (result_out == nullptr, known at the launch).  The score-only form carries no gscore / gtle / max_off and
//      writes no six-field record; the six-field form has no exit, no prune, no guard and no second pass.
// Per-row code behind the column sweep (both forms): the row maximum's column, z-drop, then ONE straight block for the band
// trimming -- the zero trim and, in the score-only form, both prunes are the same evaluation of the four-cell windows next to the
// two edges (a zero cell is a dropped cell; with `best` taken as 0 the prune's test IS the zero trim), so a lane whose prune is off
// or whose left edge may not move gets a zero operand instead of a branch.  Only the cell-by-cell loops of a zero trim that has
// run past its window, the predicated zeroing of a band that ends left of column 3, the zero-row guard and the exit's bound pass
// are divergent regions.
// The rest of the row tail is straight code (profiles/bsw_row_start.md): every flag is computed for every lane and joined with
// & and |; `best` and its row and column, the band clamp, the windows' one-cell moves and the next row's left-edge potential are
// selects or shift counts; the wave-uniform operands of that code (gap penalties, max_sc plain and packed, masks, packed steps)
// are per-lane copies made once per pair.
// NOT here, measured and taken out (same document): fetching the next row's first pair words behind the zeroing stores, in two
// forms -- both removed an LDS wait and both were slower -- and a row loop with one way out (the zero row and the last reference
// base as operands of `stop`), which cut scalar instructions and was no faster.
template <bool SYM, bool MS1, bool SO>
__global__ __launch_bounds__(64) void bsw_dp8(BswIO io, BswConst c, const BswRec *__restrict__ recs, int64_t kbeg,
                                              int64_t kend, int qcap, int32_t *__restrict__ score_out,
                                              gab_bsw_result *__restrict__ result_out, BswStats *st) {
    extern __shared__ uint32_t lds[];
    __shared__ __attribute__((aligned(8))) uint32_t row_tab[10];     // BswConst.row_lo / row_hi per reference base, for per-lane look-ups
    if (threadIdx.x < 5) { row_tab[2 * threadIdx.x] = c.row_lo[threadIdx.x]; row_tab[2 * threadIdx.x + 1] = c.row_hi[threadIdx.x]; }
    __syncthreads();
    const int lane = threadIdx.x;
    const int64_t k = kbeg + (int64_t)(gridDim.x - 1 - blockIdx.x) * 64 + lane;   // heaviest waves (largest key) first
    const bool valid = k < kend;
    BswRec rec; rec.ref_off = rec.qry_off = 0; rec.lens = rec.h0 = rec.L = 0; rec.id = 0u;
    if (valid) rec = recs[k];
    const uint32_t id = rec.id;
    const int ncell_dw = (qcap + 2) / 2;
    // cell j of this lane: 16 bits at byte address ((j >> 1) * 64 + lane) * 4 + (j & 1) * 2
    uint8_t *const CB = reinterpret_cast<uint8_t *>(lds + lane);
    uint32_t *const CW = lds + lane;                                   // pair p = columns 2p, 2p+1 at CW[p * 64]
    uint8_t *const QN = reinterpret_cast<uint8_t *>(lds + (size_t)ncell_dw * 64) + lane;   // nibble pair p at QN[p * 64]
#define CELL16(j) (*reinterpret_cast<uint16_t *>(CB + ((j) >> 1) * 256 + ((j) & 1) * 2))
#define QPAIR(p) (QN[(p) * 64])

    unsigned long long cells = 0;
    if (valid) {
        const int qlen = rec.lens >> 16, tlen = rec.lens & 0xffff, h0 = rec.h0;
        const uint8_t *q = io.qry + rec.qry_off;
        const uint8_t *t = io.ref + rec.ref_off;
        const int oe_del = c.o_del + c.e_del, oe_ins = c.o_ins + c.e_ins;
        const int e_del = c.e_del, e_ins = c.e_ins;

        // query -> nibbles (codes above 4 count as N), 8 bases -> 4 nibble bytes per trip.  The second dword is read only when
        // it holds a base (a sequence has three readable bytes behind it, not seven); the four stores stay inside the nibble
        // rows: pair 4 * ((qlen - 1) / 8) + 3 <= qcap / 2 - 1, qcap being a multiple of 16.
        for (int p0 = 0; p0 * 2 < qlen; p0 += 4) {
            const uint32_t s0 = load_u32_unaligned(q + p0 * 2);
            const uint32_t s1 = p0 * 2 + 4 < qlen ? load_u32_unaligned(q + p0 * 2 + 4) : 0u;
            // even bases in the low byte of each half, odd bases on top of them: a half is one nibble pair
            const uint32_t n0 = pk_min_u16(s0 & 0x00ff00ffu, 0x00040004u) | pk_min_u16((s0 >> 8) & 0x00ff00ffu, 0x00040004u) << 4;
            const uint32_t n1 = pk_min_u16(s1 & 0x00ff00ffu, 0x00040004u) | pk_min_u16((s1 >> 8) & 0x00ff00ffu, 0x00040004u) << 4;
            QPAIR(p0) = (uint8_t)n0; QPAIR(p0 + 1) = (uint8_t)(n0 >> 16);
            QPAIR(p0 + 2) = (uint8_t)n1; QPAIR(p0 + 3) = (uint8_t)(n1 >> 16);
        }
        int w = c.w;
        {
            int lim = (int)((double)(qlen * c.max_sc + c.end_bonus - c.o_ins) / e_ins + 1.);
            lim = lim > 1 ? lim : 1; w = w < lim ? w : lim;
            lim = (int)((double)(qlen * c.max_sc + c.end_bonus - c.o_del) / e_del + 1.);
            lim = lim > 1 ? lim : 1; w = w < lim ? w : lim;
        }
        // the prunes need every cell that row 0's band clamp leaves behind to be zero, and a z-drop that rarely sends pairs back (header comment)
        // per-lane copies of wave-uniform constants of the column sweep, made once per pair (they were seven v_mov_b32 per row):
        // the third VOP3 source of v_and_or_b32, and the operands of the 2-cycle instructions of the sweep (an SGPR or literal
        // source makes them 4-cycle instructions, r02_valu_issue.md), the pointer and column steps of a loop trip among them
        uint32_t k_selz = 0x0c000c00u, k_lo8 = 0x00ff00ffu, v_e_ins = (uint32_t)e_ins;
        uint32_t k_cstep = 512u, k_qstep = 128u, k_jstep = 4u;
        asm volatile("" : "+v"(k_selz), "+v"(k_lo8), "+v"(v_e_ins), "+v"(k_cstep), "+v"(k_qstep), "+v"(k_jstep));
        // ... and of the code behind the sweep (profiles/bsw_row_start.md): the gap penalties and max_sc as plain and as packed
        // operands, the masks and the packed steps of the window test.  As SGPRs or literals they were copied into VGPRs every
        // row (inline assembly takes VGPRs only) or made a 2-cycle instruction a 4-cycle one.
        int v_e_del = e_del, v_max_sc = c.max_sc, v_zdrop = c.zdrop;
        uint32_t k_m2 = as_u32(pk_splat(c.max_sc)), k_lo16 = 0x0000ffffu, k_two2 = 0x00020002u, k_hi1 = 0x00010000u, k_254 = 254u, k_256 = 256u;
        asm volatile("" : "+v"(v_e_del), "+v"(v_max_sc), "+v"(v_zdrop), "+v"(k_m2), "+v"(k_lo16), "+v"(k_two2), "+v"(k_hi1), "+v"(k_254), "+v"(k_256));
        bool prune = SO && (qlen <= w + 1 || h0 - oe_ins - (w + 1) * e_ins <= 0) && (c.zdrop == 0 || c.zdrop >= 8 * c.max_sc);
        int best, best_i, best_j, g_i, gscore, max_off;
      for (;;) {                                            // second trip: a pair one of the guards sent back, prunes off
        // row -1 (bandedSWA.cpp:159-161); E = 0.  Cell 0 is h0 and cell j >= 1 is max(h0 - oe_ins - (j - 1) * e_ins, 0): two cells
        // per dword store.  Pair word qlen / 2 ends on cell qlen + 1 when qlen is even -- inside the cell rows (qcap is even), and a
        // cell the sweep never reads as part of a band.
        // Seeded prune (header comment): the prunes and two of the guards test against thr = max(best, Lm1), 0 leaves thr == best;
        // and the prune of row -1: cell j >= 1 is stored only while it is live, value + max_sc * min(tlen, qlen - j) > thr0 -- both
        // terms fall from left to right, so the live cells are a prefix and jm1 ends on the last of them.  With that prune off
        // thr0 = -1 keeps every positive cell and `end` stays qlen.
        const bool seed_ok = SO && prune && min(qlen, 2 * w + 1) > 9;      // (a band that can hold more than nine cells)
        const int Lm1 = seed_ok && (c.seed & 1) ? rec.L - 1 : 0;
        const bool row_prune = seed_ok && (c.seed & 2);
        int jm1 = 0;
        {
            const int thr0 = row_prune ? max(h0, Lm1) : -1;
            int v = h0 - oe_ins;                            // cell 2p - 1
            int cl = qlen - 1;                              // columns left of cell 2p - 1
            const bool l1 = v > 0 && v + mul24(c.max_sc, min(tlen, cl)) > thr0;
            jm1 = l1 ? 1 : 0;
            CW[0] = (uint32_t)h0 | (uint32_t)(l1 ? v : 0) << 16;
            for (int p = 1; p <= (qlen >> 1); p++) {
                const int lo = v - e_ins;
                v = lo - e_ins;
                cl -= 2;
                const bool la = lo > 0 && lo + mul24(c.max_sc, min(tlen, cl + 1)) > thr0;
                const bool lb = v > 0 && v + mul24(c.max_sc, min(tlen, cl)) > thr0;
                jm1 = la ? 2 * p : jm1; jm1 = lb ? 2 * p + 1 : jm1;
                CW[p * 64] = (uint32_t)(la ? lo : 0) | (uint32_t)(lb ? v : 0) << 16;
            }
        }
        best = h0; best_i = -1; best_j = -1; g_i = -1; gscore = -1; max_off = 0;
        int beg = 0, end = row_prune && jm1 + 2 < qlen ? jm1 + 2 : qlen;
        int hrow = h0 - c.o_del - e_del;                    // row i's left edge h0 - o_del - e_del * (i + 1), carried from row to row
        int stale_pot = 0;                                  // bound on what the cells the band clamp cut can still lead to
        bool dropped = row_prune && end < min(qlen, w + 1); // a prune has dropped a live cell (row -1: the reference sweeps row 0 up to there)
        bool abandon = false;                               // one of the three guards fired
        uint32_t tw = load_u32_unaligned(t);
        for (int i = 0; i < tlen; i++, hrow -= e_del) {
            const int tc = (tw >> ((i & 3) * 8)) & 0xff;
            if ((i & 3) == 3 && i + 1 < tlen) tw = load_u32_unaligned(t + i + 1);
            // the packed score vector of this row's reference base: one 8-byte LDS read (five v_cmp + ten v_cndmask + the SGPR
            // moves they need were ~100 cycles per row)
            const uint2 rr = *reinterpret_cast<const uint2 *>(&row_tab[2 * (tc < 4 ? tc : 4)]);
            const uint32_t rlo = rr.x, rhi = rr.y;
            if (beg < i - w) beg = i - w;
            {                                               // the band clamp: both sides computed, a select keeps one
                const int ec = i + w + 1;
                const int sp = max(stale_pot, best + mul24(v_max_sc, qlen - ec));
                stale_pot = end > ec ? sp : stale_pot;
                end = min(min(end, ec), qlen);
            }
            int hleft = beg == 0 ? max(hrow, 0) : 0;
            int f = 0;
            uint32_t rowpk = 0;                   // (row max << 16) | column; ties -> later column
            int j = beg;
            // the two pair words the row can start with and their query codes: one LDS round trip for the row start
            uint32_t *cw = CW + (j >> 1) * 64;
            const uint8_t *qp = QN + (j >> 1) * 64;
            uint32_t v0 = cw[0], q0 = qp[0];
            {
                const uint32_t vn = cw[64], qn = qp[64];
                if ((j & 1) && j < end) {         // band starts on the upper half of a pair
                    const BswCellOut o = bsw_cell((int)((v0 >> 16) & 0xff), (int)(v0 >> 24), f, q0 >> 4, rlo, rhi, oe_del, e_del,
                                                  oe_ins, e_ins);
                    CELL16(j) = (uint16_t)(hleft | o.en << 8);
                    hleft = o.h; f = o.f;
                    rowpk = ((uint32_t)o.h << 16) | (uint32_t)j;
                    j++;
                    v0 = vn; q0 = qn; cw += 64; qp += 64;
                }
            }
            if (j + 1 < end) {
                // Two columns per step, the column-independent part in packed 16-bit lanes (lo = column j, hi = j+1):
                // M, E' and the F-source of both cells come from v_pk_* instructions; only the H / F carry chain
                // between the two cells is scalar.  The loop is unrolled by two pairs for the software pipeline (next pair's
                // LDS words in flight while this pair is computed); what keeps register copies out of it is said at the loop.
                const uint32_t k_oe_del = as_u32(pk_splat(oe_del)), k_e_del = as_u32(pk_splat(e_del));
                const uint32_t k_oe_ins = as_u32(pk_splat(oe_ins));
                const uint32_t k_bias = 0x00800080u, k_nib = 0x000f000fu;
                // carried between pairs, both in the LOW half of their register (high half zero):
                // HB = H of the previous column, FV = F entering the pair
                uint32_t HB = (uint32_t)hleft, FV = (uint32_t)f;
                // M is clamped at 0 (unsigned saturating subtract): H, E' and F all take a max with a non-negative
                // value, so the clamp changes none of them and lets E' / F-source use saturating subtracts too.
                // The column-to-column carry chain (H[j] -> F -> H[j+1] -> F) uses one half per instruction anyway: it runs in
                // the NON-packed 16-bit instructions (v_max_i16 / v_sub_u16 on the low halves), which issue every 2.6 cycles at
                // this occupancy instead of 4.2 (profiles/r02_valu_issue.md); the upper halves of ME and T are read through
                // src0_sel:WORD_1 of an SDWA v_max_i16 -- a 4-cycle op, but one instead of a shift and a max (profiles/bsw_row_sweep.md);
                // so do the plain 32-bit add of the two packed halves (no carry: both < 256) and the byte mask.
#define BSW_PAIR(V, QB, OUT, HJ)                                                                                \
    {                                                                                                             \
        const uint32_t d2 = (V) & k_lo8;                                         /* diag of both columns */      \
        const uint32_t e2 = __builtin_amdgcn_perm(0u, (V), 0x0c030c01u);         /* E of both columns */         \
        const uint32_t sel = and_or_b32((QB) * 0x1001u, k_nib, k_selz);          /* code j -> byte 0, j+1 -> 2 */\
        const uint32_t sc2 = __builtin_amdgcn_perm(rhi, rlo, sel);               /* biased scores per half */    \
        const uint32_t Mc = pk_subsat_u16_k(add_u32_v(d2, sc2), k_bias);                                         \
        const uint32_t M = MS1 ? pk_min_u16(Mc, add_u32_v(d2, d2)) : pk_mul_lo(Mc, pk_min_u16_1(d2));   /* diag == 0 -> M = 0 */ \
        const uint32_t Md = pk_subsat_u16_k(M, k_oe_del);                                                        \
        const uint32_t EN = pk_max_i16(Md, pk_subsat_u16_k(e2, k_e_del));                                        \
        const uint32_t T = SYM ? Md : pk_subsat_u16_k(M, k_oe_ins);                                              \
        const uint32_t ME = pk_max_i16(M, e2);                                                                   \
        const uint32_t HA = max_i16_lo(ME, FV);                                  /* H[j] */                      \
        const uint32_t FA = f_step_lo(T, FV, v_e_ins);                           /* F leaving column j */        \
        const uint32_t hprev = HB;                                                                               \
        HB = max_i16_hi_lo(ME, FA);                                           /* H[j+1] */                    \
        FV = f_step_hi(T, FA, v_e_ins);                                  /* F leaving column j+1 */      \
        /* byte 0 = H[j-1] (hprev), byte 1 = E'[j], byte 2 = H[j] (HA byte 0), byte 3 = E'[j+1] */               \
        (OUT) = (EN << 8) | __builtin_amdgcn_perm(HA, hprev, 0x0c040c00u);                                       \
        (HJ) = HA;                                                                                               \
    }
                // Row maximum: ONE key per loop trip, (largest H of the trip's four columns << 16) | first column, the max taken
                // in the 2-cycle v_max_i16.  Trips cover disjoint, increasing column ranges, so the key that wins names the
                // LAST group that holds the row maximum; which of its columns is the last one that holds it is read back from
                // the stored row after the sweep (behind CELL16(end) below).  The cells outside the loop keep exact keys.
                // The trip's three maxima, the key and its fold into rowpk are one leaf (rowkey_fold): no reader of an asm result
                // sits right behind it.  No register copies in the loop (the compiler put three into the plain form of it): the
                // pointers are bumped in place at the end of a trip by 2-cycle adds on VGPR constants, behind every LDS access
                // of the trip (the column by a plain add of such a constant, which the loop test may follow at once), and the loads of the two halves stay two ds_read_b32 (one LDS instruction more per trip):
                // merged into one two-word read they land in a register pair that the next trip's read overwrites.
                bsw_lds_u32 *cl = (bsw_lds_u32 *)cw;
                bsw_lds_u8 *ql = (bsw_lds_u8 *)qp;
                const int jlast = end - 3;
                while (j < jlast) {
                    const uint32_t v1 = cl[64], q1 = ql[64];
                    uint32_t h0j, h2j;
                    BSW_PAIR(v0, q0, cl[0], h0j)
                    const uint32_t m01 = max_i16_lo(h0j, HB);
                    asm volatile("" ::: "memory");                   // keeps the next load from merging with v1's above
                    v0 = cl[128]; q0 = ql[128];                      // pair index <= end / 2: inside the row allocation
                    BSW_PAIR(v1, q1, cl[64], h2j)
                    rowpk = rowkey_fold(rowpk, h2j, HB, m01, (uint32_t)j);
                    asm volatile("v_add_u32 %0, %0, %2\n\tv_add_u32 %1, %1, %3" : "+v"(cl), "+v"(ql) : "v"(k_cstep), "v"(k_qstep) : "memory");
                    j += (int)k_jstep;
                }
                if (j + 1 < end) {
                    const uint32_t v1 = cl[64], q1 = ql[64];         // the word a trailing single column lives in
                    uint32_t hj;
                    BSW_PAIR(v0, q0, cl[0], hj)
                    const uint32_t pa = (hj << 16) | (uint32_t)j, pb = (HB << 16) | (uint32_t)(j + 1);
                    rowpk = max(max(rowpk, pa), pb);
                    j += 2; v0 = v1; q0 = q1;
                }
                hleft = (int)HB; f = (int)FV;
#undef BSW_PAIR
            }
            if (j < end) {                        // band ends on the lower half of a pair: its word is already in v0
                const BswCellOut o = bsw_cell((int)(v0 & 0xff), (int)((v0 >> 8) & 0xff), f, q0 & 0xfu, rlo, rhi, oe_del, e_del,
                                              oe_ins, e_ins);
                CELL16(j) = (uint16_t)(hleft | o.en << 8);
                hleft = o.h; f = o.f;
                const uint32_t pk = ((uint32_t)o.h << 16) | (uint32_t)j;
                rowpk = pk > rowpk ? pk : rowpk;
                j++;
            }
            cells += (unsigned)(end > beg ? end - beg : 0);
            const int rowmax = (int)(rowpk >> 16);
            CELL16(end) = (uint16_t)hleft;        // eh[end].h = h1, eh[end].e = 0
            if constexpr (!SO) {
                if (j == qlen) {
                    if (!(gscore > hleft)) g_i = i;
                    gscore = hleft > gscore ? hleft : gscore;
                }
            }
            if (rowmax == 0) {                              // zero-row guard of the right prune (header comment, step 10)
                if constexpr (SO) {
                    if (dropped && beg == 0) {
                        // (hrow: this row's left edge, stored cell 0)
                        abandon = hrow > 0 && hrow + mul24(c.max_sc, min(tlen - 1 - i, qlen)) > max(best, Lm1);
                    }
                }
                break;
            }
            // One LDS round trip for what the rest of the row needs: the three pair words that hold the row maximum's
            // candidate columns and the six of the band trimming.  H(i, c) is the low byte of stored cell c + 1 and cell
            // `end` holds H(i, end - 1), so the candidates kj .. kj + 3 are cells kj + 1 .. kj + 4: pair words
            // (kj + 1) / 2 .. + 2, the last one at most qlen / 2 + 2 -- behind the cell rows come the query nibbles and
            // one spare row, so it is inside the launch's LDS (see lds8 at the launch), and a word past cell `end` is masked.
            const int kj = (int)(rowpk & k_lo16);
            const int pb = beg >> 1, pe = end >> 1;
            const uint32_t *const rw = CW + ((kj + 1) >> 1) * 64;
            const uint32_t r0 = rw[0], r1 = rw[64], r2 = rw[128];
            const uint32_t b0 = CW[pb * 64], b1 = CW[(pb + 1) * 64], b2 = CW[(pb + 2) * 64];
            const uint32_t e2 = CW[pe * 64], e1 = CW[(pe > 0 ? pe - 1 : 0) * 64], e0 = CW[(pe > 1 ? pe - 2 : 0) * 64];
            // rowmax_j = the LAST column c of [kj, min(kj + 3, end - 1)] with H(i, c) == rowmax.  For a loop trip's key that
            // is the reference's tie rule inside the group (a later group that reached the maximum would have won the key);
            // for an exact key column kj itself matches and no later column can: it would have made a larger key.
            int rowmax_j;
            {
                const uint32_t sh = (uint32_t)((kj + 1) & 1) << 4;
                const uint32_t c01 = __builtin_amdgcn_alignbit(r1, r0, sh), c23 = __builtin_amdgcn_alignbit(r2, r1, sh);
                const uint32_t rm2 = (uint32_t)rowmax << 16 | (uint32_t)rowmax;
                // 1 per 16-bit half whose H differs from the row maximum, gathered into bytes 0..3 = candidates 0..3
                const uint32_t ne = __builtin_amdgcn_perm(pk_min_u16_1((c23 ^ rm2) & 0x00ff00ffu), pk_min_u16_1((c01 ^ rm2) & 0x00ff00ffu),
                                                          0x06040200u);
                const int nv = end - kj < 4 ? end - kj : 4;                       // >= 1: rowmax > 0 comes from a cell of the band
                const uint32_t eq = (ne ^ 0x01010101u) & (0x01010101u >> (8 * (4 - nv)));
                rowmax_j = kj + ((31 - __builtin_clz(eq)) >> 3);
            }
            // What ends the pair's row loop in this row is gathered in `stop` and acted on once, behind the trimming (a lane that
            // stops trims its own band for nothing: the other lanes of the wave run that code anyway, and every access of it is
            // one that a row that goes on makes too).  Order as in the reference: the z-drop guard, the z-drop test, the right-edge
            // guard, and the exit's bound last.
            const int rows_left = tlen - 1 - i;
            const bool raised = rowmax > best;
            // Every flag below is computed for every lane and joined with & and |, and `best` and its row and column are selects:
            // a short-circuit form or an `if` around one to five instructions became an exec-mask region each, two scalar
            // instructions and the wait states in front of them for a lane mask that a v_cndmask takes as it is.
            const bool zd_on = c.zdrop > 0;                 // (wave-uniform; with zdrop == 0 neither z-drop flag can be set)
            const bool keeps = !raised;
            bool stop;
            {
                const int di = i - best_i, dj = rowmax_j - best_j, dd = di - dj;
                const int gap = mul24(dd > 0 ? dd : -dd, dd > 0 ? v_e_del : (int)v_e_ins);
                stop = zd_on & keeps & (best - rowmax - gap > v_zdrop);
                if constexpr (SO) {                         // z-drop guard: the reference's row maximum may differ here
                    abandon = zd_on & keeps & dropped & (rowmax < best - v_zdrop);
                    stop = stop | abandon;
                }
            }
            // the row maximum's own potential: while it exceeds best no exit is possible and the bound pass is skipped
            const bool try_exit = SO & keeps & (rowmax + mul24(v_max_sc, min(rows_left, qlen - 1 - rowmax_j)) <= best);
            best = max(best, rowmax); best_i = raised ? i : best_i; best_j = raised ? rowmax_j : best_j;
            if constexpr (!SO) {
                int off = rowmax_j - i; off = off < 0 ? -off : off;
                max_off = raised && off > max_off ? off : max_off;
            }
            const int thr = max(best, Lm1);                 // (best is this row's already; only the score-only form reads it)
            if constexpr (SO) {
                // right-edge guard of the left prune (header comment, step 5); a row that the z-drop test ends does not reach it
                const bool guard = !stop & dropped & (end < qlen) & (end != i + w + 1) & (hleft > e_ins) &
                                   (hleft - (int)v_e_ins + mul24(v_max_sc, min(rows_left, qlen - end - 1)) > thr);
                abandon = abandon | guard;
                stop = stop | guard;
            }
            // Band trimming (bandedSWA.cpp:234-237) and, in the score-only form, both prunes (header comment).  The four cells
            // next to either edge are fetched in ONE LDS round trip (whole pair words): x = cells beg0 .. beg0 + 3, y = cells
            // end0 - 3 .. end0.  A half outside [beg0, end0] or the query may hold anything: it can only shorten a count, and the
            // clamps below undo that.  rowmax > 0 puts a live cell into [beg0 + 1, end0], so both trims stop inside the band.
            // The next row's left edge, which the left prune and the exit's bound both test:
            int edge_pot = 0;
            {
                const int beg0 = beg, end0 = end;
                // x: cells 2pb .. 2pb+3, low half first, moved down one cell for an odd beg0; y: cells 2pe-2 .. 2pe+1 with cell
                // `end` on top, moved up one cell for an even end0.  The move is a shift count, not a branch.
                const uint32_t xs = (uint32_t)(beg0 & 1) << 4, ys = ((uint32_t)(end0 & 1) << 4) + 16u;
                const uint64_t x = (uint64_t)__builtin_amdgcn_alignbit(b2, b1, xs) << 32 | __builtin_amdgcn_alignbit(b1, b0, xs);
                const uint64_t y = (((uint64_t)e2 << 32 | e1) >> ys) << 32 | (uint32_t)(((uint64_t)e1 << 32 | e0) >> ys);
                const int lz = x ? __builtin_ctzll(x) >> 4 : 4, tz = y ? __builtin_clzll(y) >> 4 : 4;
                int base = min(beg0 + lz, end0);                           // the zero trim's left edge: the first live cell
                int lp = lz, tp = tz;                                      // cells either edge moves over, of its window
                if constexpr (SO) {
                    // The windows judged in packed 16-bit halves: m = max(H, E) <= 255 and max_sc * columns left <= 255.  A half is
                    // non-zero where its cell is live and its potential exceeds the lane's operand -- thr where the edge
                    // may be pruned; 0 where it may only be trimmed (prune off; or the left edge at column 0 in front of a live
                    // next-row edge, or at qlen), which leaves exactly the non-zero cells: lp == lz, tp == tz there.  A row
                    // whose zero trim runs past a window (lz == 4, tz == 4) has all four halves zero under either operand
                    // and prunes nothing on that side.
                    const int rq = min(rows_left, qlen);
                    const int hb = hrow - e_del;                           // the next row's left edge
                    const int hpot = hb + mul24(v_max_sc, rq);
                    edge_pot = hb > 0 ? hpot : 0;
                    const bool go = prune & (base < qlen) & ((base != 0) | (edge_pot <= thr));
                    const uint32_t r2 = (uint32_t)rq << 16 | (uint32_t)rq;             // (rq >= 0)
                    const uint32_t thr2 = (uint32_t)thr << 16 | (uint32_t)thr;
                    const uint32_t bestL = go ? thr2 : 0u, bestR = prune ? thr2 : 0u;
                    // columns left of the windows' first two cells, per half: (a, a - 1) = a * 0x10001 - 0x10000 for a >= 1
                    const uint32_t ca = (uint32_t)(qlen - beg0), cb = (uint32_t)(qlen - end0 + 3);
                    const uint32_t cl01 = (ca << 16 | ca) - k_hi1, cr01 = (cb << 16 | cb) - k_hi1;
#define BSW_STAY(W, CL, B2, OUT)                                                                                   \
    {                                                                                                             \
        const uint32_t m = pk_max_i16((W) & k_lo8, __builtin_amdgcn_perm(0u, (W), 0x0c030c01u));   /* max(H, E) per cell */ \
        (OUT) = pk_mul_lo(pk_subsat_u16_v(add_u32_v(m, pk_mul_lo(pk_min_u16((CL), r2), k_m2)), (B2)), pk_min_u16_1(m)); \
    }
                    uint32_t sll, slh, srl, srh;
                    BSW_STAY((uint32_t)x, cl01, bestL, sll)
                    BSW_STAY((uint32_t)(x >> 32), cl01 - k_two2, bestL, slh)
                    BSW_STAY((uint32_t)y, cr01, bestR, srl)
                    BSW_STAY((uint32_t)(y >> 32), cr01 - k_two2, bestR, srh)
#undef BSW_STAY
                    const uint64_t stl = (uint64_t)slh << 32 | sll, str = (uint64_t)srh << 32 | srl;
                    lp = stl ? __builtin_ctzll(stl) >> 4 : 4;
                    tp = str ? __builtin_clzll(str) >> 4 : 4;
                }
                int bl = beg0 + lp;
                if (__builtin_expect(lz == 4, 0)) {                        // the reference's cell-by-cell trim, behind the window
                    for (j = beg0 + 4; j < end0 && CELL16(j) == 0; j++) {}
                    base = bl = j < end0 ? j : end0;
                }
                j = end0 - tz;
                if (__builtin_expect(tz == 4, 0)) for (; j >= base && CELL16(j) == 0; j--) {}
                const int jlz = j > base - 1 ? j : base - 1;               // the zero trim's last live stored cell (base - 1: none)
                const int endz = jlz + 2 < qlen ? jlz + 2 : qlen;
                beg = bl < endz ? bl : endz;
                int jl = jlz;
                if constexpr (SO) {
                    dropped = dropped | (beg > base);                      // (cell `base` is live)
                    // Right edge: jn = where the prune stops, never left of beg - 1 and, with tz == 4, never left of jlz.  The
                    // dropped cells jn + 1 .. jlz lie in y's window and are set to zero with 16-bit stores (nothing waits for
                    // them; no word write-back: with end0 <= 3 the edge words are clamped duplicates).  With end0 >= 3 all four
                    // cells of the window are the lane's own, and the four stores are unconditional: every cell right of the new
                    // jl gets zero -- the dropped ones, and those the zero trim found zero already -- and the others get the value
                    // they hold.  Only a band that ends left of column 3 takes the predicated form.
                    int jn = end0 - tp;
                    jn = jn > beg - 1 ? jn : beg - 1;
                    dropped = dropped | (jn < jlz);
                    jl = jn < jlz ? jn : jlz;
                    if (__builtin_expect(end0 >= 3, 1)) {
                        const int nz = end0 - jl;                          // >= 0; cells of the window to clear, from the top
                        const uint64_t yz = nz >= 4 ? 0ull : y & (~0ull >> (16 * nz));
                        uint8_t *const a0 = CB + (end0 >> 1) * 256 + (end0 & 1) * 2;          // cell end0; cell end0 - 2 is 256 bytes below
                        const uint32_t d1 = (end0 & 1) ? 2u : k_254;                                  // cell end0 - 1 (and end0 - 3 below end0 - 2)
                        *reinterpret_cast<uint16_t *>(a0) = (uint16_t)(yz >> 48);
                        *reinterpret_cast<uint16_t *>(a0 - d1) = (uint16_t)(yz >> 32);
                        uint8_t *const a2 = a0 - k_256;
                        *reinterpret_cast<uint16_t *>(a2) = (uint16_t)(yz >> 16);
                        *reinterpret_cast<uint16_t *>(a2 - d1) = (uint16_t)yz;
                    } else if (jn < jlz) {
#pragma unroll
                        for (int k = 0; k < 3; k++) {                      // (end0 <= 2)
                            const int cj = end0 - k;                       // > jn >= -1
                            if (cj > jn && cj <= jlz) CELL16(cj) = 0;
                        }
                    }
                }
                end = jl + 2 < qlen ? jl + 2 : qlen;
            }
            {
                // (edge_pot and stale_pot are never negative)  The bound pass is the one divergent region here: a lane enters
                // it only when the cheap terms of the bound leave the exit open.
                int bound = max(stale_pot, beg == 0 ? edge_pot : 0);
                if (try_exit & !stop & (bound <= best)) {
                    // pot() of columns 2p (low half) and 2p + 1 (high half) of every pair word that holds a cell of [beg, end];
                    // the halves outside the band are masked to Hd = 0.  All halves stay below 2^15: Hd <= 255,
                    // max_sc * (columns left) <= max_sc * qcap <= 255.
                    const int pb = beg >> 1, pe = end >> 1;
                    const uint32_t r2 = as_u32(pk_splat(rows_left));
                    uint32_t cl2 = (uint32_t)(qlen - 2 * pb) | (uint32_t)(qlen - 2 * pb - 1) << 16;    // columns left, per half
                    uint32_t acc = 0;
                    for (int p = pb; p <= pe; p++, cl2 -= 0x00020002u) {
                        uint32_t d2 = CW[p * 64] & 0x00ff00ffu;
                        if (p == pb && (beg & 1)) d2 &= 0xffff0000u;
                        if (p == pe && !(end & 1)) d2 &= 0x0000ffffu;
                        const uint32_t gain = pk_mul_lo(pk_min_u16(cl2, r2), k_m2);
                        acc = pk_max_i16(acc, pk_mul_lo(add_u32_v(d2, gain), pk_min_u16_1(d2)));
                    }
                    bound = max(bound, max((int)(acc & 0xffffu), (int)(acc >> 16)));
                    stop = bound <= best;
                }
            }
            if (stop) break;
        }
        if (!SO || !abandon) break;
        prune = false;
      }
        score_out[id] = best;
        if constexpr (!SO) {
            gab_bsw_result r;
            r.score = best; r.qle = best_j + 1; r.tle = best_i + 1;
            r.gtle = g_i + 1; r.gscore = gscore; r.max_off = max_off;
            result_out[id] = r;
        }
    }
#undef CELL16
#undef QPAIR
    for (int o = 32; o > 0; o >>= 1) cells += __shfl_xor(cells, o);
    if (lane == 0 && cells) atomicAdd(&st->cells, cells);
}

// the eight instantiations of bsw_dp8
using BswDp8Fn = void (*)(BswIO, BswConst, const BswRec *, int64_t, int64_t, int, int32_t *, gab_bsw_result *, BswStats *);
template <bool SYM, bool MS1> BswDp8Fn bsw_dp8_pick(bool so) { return so ? bsw_dp8<SYM, MS1, true> : bsw_dp8<SYM, MS1, false>; }
BswDp8Fn bsw_dp8_kernel(bool sym, bool ms1, bool so) {
    return sym ? (ms1 ? bsw_dp8_pick<true, true>(so) : bsw_dp8_pick<true, false>(so))
               : (ms1 ? bsw_dp8_pick<false, true>(so) : bsw_dp8_pick<false, false>(so));
}

}  // namespace

// =============================================================================== host side
struct gab_bsw {
    gab_tuning tun = gab_tuning_loaded();      // experiment knobs, read when the handle is made
    gab_host_stream hs;     // private stream of the host-pointer entry point(s)
    int device = 0;
    gab_bsw_params prm;
    BswConst cst;
    gab_devbuf ws;          // hist | start | qstart | stats | records in bucket order | rank
    gab_devbuf io;          // staging for the host-pointer entry point
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // total begin, dp begin, dp end, total end
    // the per-class DP launches rotate over the caller's stream and these, so that the draining tail of one class
    // overlaps the next classes (fork / join with the events)
    static constexpr int kAux = 1;        // 3 measured equal to 1
    hipStream_t aux[kAux] = {nullptr};
    hipEvent_t fork = nullptr, join[kAux] = {nullptr};
    // a large batch is sorted in slices (bsw_run_device_impl): the sort of slice 1 runs on this stream beside slice 0's DP.
    // Made by the first sliced call, so that a handle that never sees a large batch opens no third queue.
    hipStream_t sort = nullptr;
    hipEvent_t sort_fork = nullptr, sort_join = nullptr;
    bool have_stats = false;
    int stat_slices = 1;            // slices of the last run: its cells are the sum of their counters
    uint32_t *h_qstart[kSlices] = {nullptr};   // pinned, kQBuckets + 1 per slice (one allocation)
    BswStats *h_stats[kSlices] = {nullptr};    // pinned, per slice (one allocation with h_init)
    BswStats *h_init = nullptr;     // pinned: what a slice's counters start from, written once
    bool out_of_order = false;      // gab_bsw_run: a batch's sequences did not lie in pair order (its sampled window was rejected by the device)
};

extern "C" int gab_bsw_create(const gab_bsw_params *p, int device, gab_bsw **out) {
    if (!p || !out) { gab_set_error("gab_bsw_create: NULL argument"); return GAB_EINVAL; }
    *out = nullptr;
    GAB_CHECK(p->e_del > 0 && p->e_ins > 0 && p->o_del >= 0 && p->o_ins >= 0,
              "gab_bsw_create: gap penalties must be o>=0, e>0 (got o_del=%d e_del=%d o_ins=%d e_ins=%d)",
              p->o_del, p->e_del, p->o_ins, p->e_ins);
    GAB_CHECK(p->w >= 0 && p->zdrop >= 0, "gab_bsw_create: w and zdrop must be >= 0");
    GAB_CHECK(p->o_del + p->e_del < 32768 && p->o_ins + p->e_ins < 32768 && p->end_bonus >= -32768 &&
              p->end_bonus < 32768, "gab_bsw_create: penalties out of 16-bit range");
    int rc = gab_check_device(device);
    if (rc) return rc;
    gab_device_guard g(device);
    gab_bsw *h = new (std::nothrow) gab_bsw();
    if (!h) { gab_set_error("out of host memory"); return GAB_ENOMEM; }
    h->device = device; h->prm = *p;
    BswConst &c = h->cst;
    c.o_del = p->o_del; c.e_del = p->e_del; c.o_ins = p->o_ins; c.e_ins = p->e_ins;
    c.zdrop = p->zdrop; c.end_bonus = p->end_bonus; c.w = p->w;
    int mx = 0;
    for (int k = 0; k < 25; k++) mx = p->mat[k] > mx ? p->mat[k] : mx;
    c.max_sc = mx;
    c.seed = 1 | (mx <= p->e_ins ? 2 : 0);
    c.hop_a = p->mat[0]; c.hop_mm = p->mat[1]; c.hop_n = p->mat[4];
    c.hop = c.hop_a > 0 && c.hop_mm <= c.hop_a && c.hop_n <= c.hop_a;
    for (int k = 0; k < 25; k++) c.hop = c.hop && p->mat[k] == (k / 5 == 4 || k % 5 == 4 ? c.hop_n : k / 5 == k % 5 ? c.hop_a : c.hop_mm);
    for (int t = 0; t < 5; t++) {
        uint32_t lo = 0;
        for (int q = 0; q < 4; q++) lo |= (uint32_t)(uint8_t)(p->mat[t * 5 + q] + 128) << (8 * q);
        c.row_lo[t] = lo;
        c.row_hi[t] = (uint32_t)(uint8_t)(p->mat[t * 5 + 4] + 128);
    }
    for (int k = 0; k < 4; k++)
        if (hipEventCreate(&h->ev[k]) != hipSuccess) { gab_set_error("hipEventCreate failed"); delete h; return GAB_EDEVICE; }
    bool aux_ok = hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < gab_bsw::kAux && aux_ok; k++)
        aux_ok = hipStreamCreateWithFlags(&h->aux[k], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&h->join[k], hipEventDisableTiming) == hipSuccess;
    if (!aux_ok) { gab_set_error("gab_bsw_create: stream / event creation failed"); delete h; return GAB_EDEVICE; }
    // the 256-base class needs more than the default 64 KiB of dynamic LDS
    if (hipFuncSetAttribute((const void *)bsw_dp<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void *)bsw_dp<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        gab_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"); delete h; return GAB_EDEVICE;
    }
    for (int k = 0; k < 8; k++)
        if (hipFuncSetAttribute((const void *)bsw_dp8_kernel(k & 4, k & 2, k & 1), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64) != hipSuccess) {
            gab_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"); delete h; return GAB_EDEVICE;
        }
    if (hipHostMalloc((void **)&h->h_qstart[0], sizeof(uint32_t) * (kQBuckets + 1) * kSlices) != hipSuccess ||
        hipHostMalloc((void **)&h->h_stats[0], sizeof(BswStats) * (kSlices + 1)) != hipSuccess) {
        gab_set_error("hipHostMalloc failed"); gab_bsw_destroy(h); return GAB_ENOMEM;
    }
    for (int k = 1; k < kSlices; k++) { h->h_qstart[k] = h->h_qstart[0] + (size_t)k * (kQBuckets + 1); h->h_stats[k] = h->h_stats[0] + k; }
    h->h_init = h->h_stats[0] + kSlices;
    memset(h->h_init, 0, sizeof(BswStats));
    h->h_init->first_bad = 0x7fffffff;      // (bsw_hist takes an atomicMin on it)
    *out = h;
    return GAB_OK;
}

extern "C" void gab_bsw_destroy(gab_bsw *h) {
    if (!h) return;
    gab_device_guard g(h->device);
    h->ws.release(); h->io.release(); h->hs.release();
    for (int k = 0; k < 4; k++) if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
    if (h->fork) (void)hipEventDestroy(h->fork);
    for (int k = 0; k < gab_bsw::kAux; k++) {
        if (h->join[k]) (void)hipEventDestroy(h->join[k]);
        if (h->aux[k]) (void)hipStreamDestroy(h->aux[k]);
    }
    if (h->sort_fork) (void)hipEventDestroy(h->sort_fork);
    if (h->sort_join) (void)hipEventDestroy(h->sort_join);
    if (h->sort) (void)hipStreamDestroy(h->sort);
    if (h->h_qstart[0]) (void)hipHostFree(h->h_qstart[0]);
    if (h->h_stats[0]) (void)hipHostFree(h->h_stats[0]);
    delete h;
}

// The sort workspace: per slice a block of hist | start | qstart | sums | stats (slice 1's sort writes its own while slice 0's DP
// adds to slice 0's cells), then the records of all n pairs in bucket order, slice after slice, then the n ranks and the n
// lower bounds of bsw_seed.
struct BswLayout {
    size_t o_start, o_qstart, o_sums, o_stats, blk;   // inside a slice's block (hist at 0); blk = the block's size
    size_t o_recs, o_rank, o_seed, total;
    explicit BswLayout(size_t n) {
        o_start = sizeof(uint32_t) * kNumKeys;
        o_qstart = o_start + sizeof(uint32_t) * (kNumKeys + 1);
        o_sums = o_qstart + sizeof(uint32_t) * (kQBuckets + 1);
        o_stats = (o_sums + sizeof(uint32_t) * kScanBlocks + 15) & ~(size_t)15;
        blk = (o_stats + sizeof(BswStats) + 255) & ~(size_t)255;
        o_recs = blk * kSlices;
        o_rank = o_recs + ((sizeof(BswRec) * n + 255) & ~(size_t)255);
        o_seed = o_rank + ((sizeof(uint32_t) * n + 255) & ~(size_t)255);
        total = o_seed + sizeof(int32_t) * n;
    }
};

static int bsw_run_device_impl(gab_bsw *h, const uint8_t *ref, int64_t ref_bytes, const int64_t *ref_off,
                               const uint8_t *qry, int64_t qry_bytes, const int64_t *qry_off,
                               const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                               int32_t *score_out, gab_bsw_result *result_out, void *stream_, int64_t ref_lo, int64_t qry_lo,
                               int64_t ref_hi, int64_t qry_hi);
extern "C" int gab_bsw_run_device(gab_bsw *h, const uint8_t *ref, int64_t ref_bytes, const int64_t *ref_off,
                                  const uint8_t *qry, int64_t qry_bytes, const int64_t *qry_off,
                                  const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                                  int32_t *score_out, gab_bsw_result *result_out, void *stream_) {
    if (h) gab_tuning_refresh(&h->tun);
    return bsw_run_device_impl(h, ref, ref_bytes, ref_off, qry, qry_bytes, qry_off, len1, len2, h0, n, score_out, result_out, stream_, 0, 0,
                               ref_bytes, qry_bytes);
}
static int bsw_run_device_impl(gab_bsw *h, const uint8_t *ref, int64_t ref_bytes, const int64_t *ref_off,
                               const uint8_t *qry, int64_t qry_bytes, const int64_t *qry_off,
                               const int32_t *len1, const int32_t *len2, const int32_t *h0, int64_t n,
                               int32_t *score_out, gab_bsw_result *result_out, void *stream_, int64_t ref_lo, int64_t qry_lo,
                               int64_t ref_hi, int64_t qry_hi) {
    GAB_CHECK(h, "gab_bsw_run_device: NULL handle");
    GAB_CHECK(n >= 0 && n < (1ll << 31), "gab_bsw_run_device: n=%lld out of range", (long long)n);
    h->have_stats = false;
    if (n == 0) return GAB_OK;
    GAB_CHECK(ref && ref_off && qry && qry_off && len1 && len2 && h0 && score_out,
              "gab_bsw_run_device: NULL buffer");
    gab_device_guard g(h->device);
    hipStream_t s = (hipStream_t)stream_;

    // A batch of at least slice_min pairs is cut into slice 0, pairs 0 .. slice0 - 1, and slice 1, the rest.  Each slice is
    // sorted by itself into its own part of the records and gets its own class launches; see the launch comment below.
    const int64_t slice0 = h->tun.bsw_slice[0] > 0 ? h->tun.bsw_slice[0] : result_out ? kSlice0Full : kSlice0;
    const int64_t slice_min = std::max<int64_t>(h->tun.bsw_slice[1] > 0 ? h->tun.bsw_slice[1] : kSliceMin, slice0 + 1);
    const int nsl = n >= slice_min ? kSlices : 1;
    const int64_t cut[kSlices + 1] = {0, nsl > 1 ? slice0 : n, n};
    if (nsl > 1 && !h->sort) {
        if (hipStreamCreateWithFlags(&h->sort, hipStreamNonBlocking) != hipSuccess) { h->sort = nullptr; gab_set_error("gab_bsw_run_device: stream creation failed"); return GAB_EDEVICE; }
        if (!h->sort_fork) GAB_HIP(hipEventCreateWithFlags(&h->sort_fork, hipEventDisableTiming));
        if (!h->sort_join) GAB_HIP(hipEventCreateWithFlags(&h->sort_join, hipEventDisableTiming));
    }

    const BswLayout L((size_t)n);
    int rc = h->ws.reserve(L.total);
    if (rc) return rc;
    char *base = h->ws.as<char>();
    BswRec *d_recs = (BswRec *)(base + L.o_recs);             // the pairs' records in bucket order, slice after slice
    uint32_t *d_rank = (uint32_t *)(base + L.o_rank);
    int32_t *d_seed = (int32_t *)(base + L.o_seed);
    auto d_stats = [&](int k) { return (BswStats *)(base + L.blk * k + L.o_stats); };

    BswIO io{ref, ref_off, qry, qry_off, len1, len2, h0, ref_bytes, qry_bytes, n, ref_lo, qry_lo, ref_hi, qry_hi};
    // the sort of slice k on stream q; its class boundaries and statistics end up in the slice's host mirrors
    auto enqueue_sort = [&](int k, hipStream_t q) -> hipError_t {
        char *b = base + L.blk * k;
        uint32_t *d_hist = (uint32_t *)b, *d_start = (uint32_t *)(b + L.o_start), *d_qstart = (uint32_t *)(b + L.o_qstart);
        uint32_t *d_sums = (uint32_t *)(b + L.o_sums);
        const int64_t lo = cut[k], hi = cut[k + 1];
        hipError_t e = hipMemsetAsync(b, 0, L.blk, q);
        // first_bad uses atomicMin, so it starts at INT_MAX (set by a tiny H2D after the memset)
        if (e == hipSuccess) e = hipMemcpyAsync(d_stats(k), h->h_init, sizeof(BswStats), hipMemcpyHostToDevice, q);
        if (e != hipSuccess) return e;
        const int gmax = k > 0 ? kSortGridBeside : 1024;
        const int grid = (int)(gab_ceil_div(hi - lo, 256) < gmax ? gab_ceil_div(hi - lo, 256) : gmax);   // (one same-address atomicMax per wave)
        const int sgrid = (int)(gab_ceil_div(hi - lo, 256) < kSeedGridBeside ? gab_ceil_div(hi - lo, 256) : kSeedGridBeside);
        const int seeded = result_out == nullptr;      // score-only: L and the deficit key; six-field: validation and the key it had
        if (k > 0) {      // beside slice 0's DP kernels: the scan on a grid of its own
            hipLaunchKernelGGL(bsw_seed, dim3(sgrid), dim3(256), 0, q, io, h->cst, seeded, lo, hi, d_seed);
            hipLaunchKernelGGL(bsw_hist<false>, dim3(grid), dim3(256), 0, q, io, h->cst, seeded, lo, hi, d_seed, d_hist, d_rank, d_stats(k));
        } else {
            hipLaunchKernelGGL(bsw_hist<true>, dim3(grid), dim3(256), 0, q, io, h->cst, seeded, lo, hi, d_seed, d_hist, d_rank, d_stats(k));
        }
        hipLaunchKernelGGL(bsw_scan_a, dim3(kScanBlocks), dim3(1024), 0, q, d_hist, d_start, d_sums);
        hipLaunchKernelGGL(bsw_scan_b, dim3(kScanBlocks), dim3(1024), 0, q, d_start, (const uint32_t *)d_sums, d_qstart);
        hipLaunchKernelGGL(bsw_scatter, dim3(grid), dim3(256), 0, q, io, h->cst.max_sc, seeded, lo, hi, (const int32_t *)d_seed, d_start, d_rank, d_recs + lo);
        e = hipMemcpyAsync(h->h_qstart[k], d_qstart, sizeof(uint32_t) * (kQBuckets + 1), hipMemcpyDeviceToHost, q);
        if (e == hipSuccess) e = hipMemcpyAsync(h->h_stats[k], d_stats(k), sizeof(BswStats), hipMemcpyDeviceToHost, q);
        return e;
    };
    GAB_HIP(hipEventRecord(h->ev[0], s));
    GAB_HIP(enqueue_sort(0, s));
    GAB_HIP(hipStreamSynchronize(s));   // launch geometry of the DP depends on the class sizes
    const bool sym = h->cst.o_del + h->cst.e_del == h->cst.o_ins + h->cst.e_ins;
    const bool ms1 = h->cst.max_sc <= 1;

    // From here on kernels may be in flight on up to three streams, and those of the DP write the caller's outputs: an error
    // return waits for all of them first, so that nothing still writes score_out / result_out after the call has returned.
    hipStream_t s_main = s;
    auto join_all = [&]() {
        (void)hipStreamSynchronize(s_main);
        for (int k = 0; k < gab_bsw::kAux; k++) (void)hipStreamSynchronize(h->aux[k]);
        if (nsl > 1) (void)hipStreamSynchronize(h->sort);
    };
#define BSW_HIP_JOINED(call)                                                                                       \
    do {                                                                                                           \
        hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess) {                                                                                    \
            gab_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_));                    \
            join_all();                                                                                            \
            return e_ == hipErrorOutOfMemory ? GAB_ENOMEM : GAB_EDEVICE;                                           \
        }                                                                                                          \
    } while (0)
    // Launch order of a sliced call.  The sort of 10 M pairs takes 0.8 ms in which no DP kernel runs, and the DP cannot start
    // before the host has read the class sizes.  So only slice 0 is sorted with the GPU otherwise idle.  The sort of slice 1 goes
    // to a stream of its own just before slice 0's class launches, which go out as an unsliced call's do (longest class first,
    // alternating over the caller's stream and the aux stream); the host waits for the sort while the GPU works on slice 0,
    // and then enqueues slice 1's class launches over all three streams (below).  Slice 0 is sized so that its DP outlasts
    // that sort and no more, because its launches are small ones: see kSlice0.
    GAB_HIP(hipEventRecord(h->fork, s));
    for (int k = 0; k < gab_bsw::kAux; k++) GAB_HIP(hipStreamWaitEvent(h->aux[k], h->fork, 0));
    int nlaunch = 0;
    constexpr int kRing = gab_bsw::kAux + 2;
    hipStream_t ring[kRing] = {nsl > 1 ? h->sort : nullptr, s_main};
    for (int k = 0; k < gab_bsw::kAux; k++) ring[k + 2] = h->aux[k];
    for (int sl = 0; sl < nsl; sl++) {
    if (sl > 0) BSW_HIP_JOINED(hipStreamSynchronize(h->sort));      // (the GPU is busy with the DP of the slice before)
    const BswStats &hst = *h->h_stats[sl];
    const uint32_t *qstart = h->h_qstart[sl];
    if (hst.bad) {
        // (slice 0 is refused before any DP kernel runs and before slice 1 is looked at, so the count is slice 0's; a bad pair of
        // slice 1 is found with slice 0's DP in flight: none of slice 1's runs, and the outputs are unspecified)
        gab_set_error("gab_bsw_run_device: %d pair(s) violate the limits (first: pair %d): need 1<=len2<=%d, "
                      "1<=len1<=%d, 0<=h0, offsets inside the slabs with 3 more readable bytes behind every sequence",
                      hst.bad, hst.first_bad - 1, GAB_BSW_MAX_QLEN, GAB_BSW_MAX_TLEN);
        join_all();
        return GAB_EINVAL;
    }
    const bool last = sl + 1 == nsl;
    if (!last) {
        BSW_HIP_JOINED(hipEventRecord(h->sort_fork, s_main));
        BSW_HIP_JOINED(hipStreamWaitEvent(h->sort, h->sort_fork, 0));
        BSW_HIP_JOINED(enqueue_sort(sl + 1, h->sort));
    }
    if (sl == 0) BSW_HIP_JOINED(hipEventRecord(h->ev[1], s));
    int max_h0 = 0;
    for (int cls = 0; cls < kNumClasses; cls++) max_h0 = hst.max_h0[cls] > max_h0 ? hst.max_h0[cls] : max_h0;
    char slice_tag[16] = "";
    if (nsl > 1) snprintf(slice_tag, sizeof slice_tag, " slice %d", sl);
    // Small batches (fewer waves than fill the chip a few times over) go out as ONE launch sized for their longest query:
    // eight class launches of a couple of hundred waves each leave most CUs idle and pay eight launch latencies
    // (100 k pairs: 3.0 -> 1.x ms); the records are in key order, so the heaviest waves still start first.
    const bool one_launch = nsl == 1 && n <= (int64_t)64 * 8192;
    int top_cls = kNumClasses - 1;
    while (top_cls > 0 && qstart[(top_cls + 1) * kClassStep] <= qstart[top_cls * kClassStep]) top_cls--;
    // Slice 1's launches rotate over the sort stream, idle by now, the caller's and the aux stream.  The other two still hold
    // launches of slice 0, so the rotation is phased to give the idle stream the heaviest (pairs x qcap) of the first round's
    // launches: that one starts at once.  In a read set the longest class holds few pairs and the second one is the heavy one.
    int ring_phase = 0;
    if (sl > 0) {
        int64_t heaviest = 0;
        for (int cls = kNumClasses - 1, k = 0; cls >= 0 && k < kRing; cls--) {
            const int64_t w = ((int64_t)qstart[(cls + 1) * kClassStep] - (int64_t)qstart[cls * kClassStep]) * (cls + 1);
            if (w <= 0) continue;
            if (w > heaviest) { heaviest = w; ring_phase = k; }
            k++;
        }
        nlaunch = 0;
    }
    for (int cls = kNumClasses - 1; cls >= 0; cls--) {      // longest queries first: the tail of the step is made of short work
        int64_t kb = qstart[cls * kClassStep], ke = qstart[(cls + 1) * kClassStep];
        if (one_launch) { if (cls != top_cls) continue; kb = 0; }
        if (ke <= kb) continue;
        const int qcap = (cls + 1) * kClassStep;
        const int blocks = (int)gab_ceil_div(ke - kb, 64);
        s = (nlaunch % (gab_bsw::kAux + 1)) ? h->aux[nlaunch % (gab_bsw::kAux + 1) - 1] : s_main;
        if (sl > 0) s = ring[(nlaunch - ring_phase + kRing) % kRing];
        nlaunch++;
        // every H / E value of the launch is at most h0 + qlen * max_sc (max_sc >= 0: bsw_create starts its max at 0):
        // 8-bit cells when that fits a byte, 16-bit packed cells when it fits 15 bits, else 32-bit cells.  max_h0 is the
        // slice's own, so the two slices of a call may run different kernels for the same class
        const int64_t hmax = (int64_t)(one_launch ? max_h0 : hst.max_h0[cls]) + (int64_t)qcap * h->cst.max_sc;
        const bool wide = hmax > 32767;
        if (h->tun.bsw_trace)     // GAB_BSW_TRACE: which DP kernel each launch runs (a sliced call says which slice)
            fprintf(stderr, "[gab_bsw_dp %p] class %d qcap %d pairs %lld bits %d sym %d ms1 %d%s\n", (void *)h, cls, qcap,
                    (long long)(ke - kb), hmax <= 255 ? 8 : wide ? 32 : 16, (int)sym, (int)ms1, slice_tag);
        kb += cut[sl]; ke += cut[sl];      // (the slice's records start at record cut[sl])
        BswStats *const d_st = d_stats(sl);
        if (hmax <= 255 && h->cst.max_sc >= 0) {
            // qcap / 2 + 1 rows of cells, the nibble rows (at least one) and one spare row: the kernel reads up to pair word
            // qlen / 2 + 2 (row start, band trimming, the row maximum's candidates), which this layout holds for every qcap >= qlen
            const size_t lds8 = sizeof(uint32_t) * 64 * ((size_t)(qcap + 2) / 2 + ((size_t)(qcap + 1) / 2 + 3) / 4 + 1);
            auto kern = bsw_dp8_kernel(sym, ms1, result_out == nullptr);      // (score-only is a template argument of bsw_dp8)
            hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds8, s, io, h->cst, d_recs, kb, ke, qcap,
                               score_out, result_out, d_st);
            continue;
        }
        const size_t lds = sizeof(uint32_t) * 64 * ((size_t)(wide ? 2 : 1) * (qcap + 1) + (size_t)(qcap + 3) / 4);
        if (wide)
            hipLaunchKernelGGL(bsw_dp<true>, dim3(blocks), dim3(64), lds, s, io, h->cst, d_recs, kb, ke, qcap,
                               score_out, result_out, d_st);
        else
            hipLaunchKernelGGL(bsw_dp<false>, dim3(blocks), dim3(64), lds, s, io, h->cst, d_recs, kb, ke, qcap,
                               score_out, result_out, d_st);
    }
    s = s_main;
    BSW_HIP_JOINED(hipGetLastError());
    }      // (slices)
    if (nsl > 1) {
        BSW_HIP_JOINED(hipEventRecord(h->sort_join, h->sort));
        BSW_HIP_JOINED(hipStreamWaitEvent(s, h->sort_join, 0));
    }
    for (int k = 0; k < gab_bsw::kAux; k++) {
        BSW_HIP_JOINED(hipEventRecord(h->join[k], h->aux[k]));
        BSW_HIP_JOINED(hipStreamWaitEvent(s, h->join[k], 0));
    }
    BSW_HIP_JOINED(hipEventRecord(h->ev[2], s));
    for (int k = 0; k < nsl; k++) BSW_HIP_JOINED(hipMemcpyAsync(h->h_stats[k], d_stats(k), sizeof(BswStats), hipMemcpyDeviceToHost, s));
    BSW_HIP_JOINED(hipEventRecord(h->ev[3], s));
#undef BSW_HIP_JOINED
    h->stat_slices = nsl;
    h->have_stats = true;
    return GAB_OK;
}

extern "C" int gab_bsw_run(gab_bsw *h, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry,
                           const int64_t *qry_off, const int32_t *len1, const int32_t *len2,
                           const int32_t *h0, int64_t n, int32_t *score_out) {
    GAB_CHECK(h, "gab_bsw_run: NULL handle");
    GAB_CHECK(n >= 0 && n < (1ll << 31), "gab_bsw_run: n=%lld out of range", (long long)n);
    if (n == 0) return GAB_OK;
    GAB_CHECK(ref && ref_off && qry && qry_off && len1 && len2 && h0 && score_out, "gab_bsw_run: NULL buffer");
    gab_device_guard g(h->device);
    gab_tuning_refresh(&h->tun);
    const bool trace = h->tun.bsw_trace;      // GAB_BSW_TRACE, diagnosis: per-phase wall times of this call on stderr
    const double t_0 = gab_now_ms();
    // extent of the two slabs actually referenced: only [min, max) is staged, so a driver can hand a window
    // of a big input (absolute offsets) to each GPU without re-basing its offset arrays.  A scan of all n offsets here is
    // ~1 ms per million pairs of serial host work inside the caller's ROI, and the device validates every pair against the
    // staged window anyway (bsw_hist): the window is first taken from 66 pairs spread over the batch -- exact whenever the
    // sequences lie in pair order, as loadPairs lays them out (main_banded.cpp:164-206) -- and only a batch the device
    // rejects for it is scanned in full and staged again.
    int64_t rb = 0, qb = 0, ra = INT64_MAX, qa = INT64_MAX;
    auto take = [&](int64_t i) {
        int64_t r = ref_off[i] + len1[i], q = qry_off[i] + len2[i];
        rb = r > rb ? r : rb; qb = q > qb ? q : qb;
        ra = ref_off[i] < ra ? ref_off[i] : ra; qa = qry_off[i] < qa ? qry_off[i] : qa;
        return ref_off[i] >= 0 && qry_off[i] >= 0 && len1[i] >= 0 && len2[i] >= 0;
    };
    bool sampled = n > 4096 && !h->out_of_order && !h->tun.bsw_full_scan;      // (a batch of this handle was rejected for its sampled window: scan from then on)
    if (sampled) {
        bool ok = take(0);
        ok = take(n - 1) && ok;
        for (int k = 1; k <= 64; k++) ok = take((n - 1) * k / 65) && ok;
        // (a window the sample makes absurd -- negative fields, or more than 64 KB per pair -- is not worth a copy: scan)
        if (!ok || rb - ra > 65536 * n || qb - qa > 65536 * n) sampled = false;
    }
    if (!sampled) {
        rb = qb = 0; ra = qa = INT64_MAX;
        for (int64_t i = 0; i < n; i++)
            GAB_CHECK(take(i), "gab_bsw_run: negative offset/length at pair %lld", (long long)i);
    }
    ra &= ~(int64_t)255; qa &= ~(int64_t)255;          // keep the device alignment of the slab origin
    const size_t rpad = ((size_t)(rb - ra) + 3 + 255) & ~(size_t)255, qpad = ((size_t)(qb - qa) + 3 + 255) & ~(size_t)255;
    const size_t nn = (size_t)n;
    size_t o = 0;
    const size_t o_ref = o; o += rpad;
    const size_t o_qry = o; o += qpad;
    const size_t o_roff = o; o += 8 * nn;
    const size_t o_qoff = o; o += 8 * nn;
    const size_t o_l1 = o; o += 4 * nn;
    const size_t o_l2 = o; o += 4 * nn;
    const size_t o_h0 = o; o += 4 * nn;
    const size_t o_sc = o; o += 4 * nn;
    int rc = h->io.reserve(o);
    if (rc) return rc;
    char *b = h->io.as<char>();
    hipStream_t s = nullptr;
    if ((rc = h->hs.get(&s)) != GAB_OK) return rc;
    const double t_1 = gab_now_ms();
    {   // the copies of one chunk at a time per GPU (gab_core.hip: the workers of a GPU must not copy in lockstep)
        std::lock_guard<std::mutex> gate(gab_h2d_mutex(h->device));
        GAB_HIP(hipMemcpyAsync(b + o_ref, ref + ra, (size_t)(rb - ra), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_qry, qry + qa, (size_t)(qb - qa), hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_roff, ref_off, 8 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_qoff, qry_off, 8 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_l1, len1, 4 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_l2, len2, 4 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipMemcpyAsync(b + o_h0, h0, 4 * nn, hipMemcpyHostToDevice, s));
        GAB_HIP(hipStreamSynchronize(s));
    }
    double t_2 = 0;
    if (trace) { GAB_HIP(hipStreamSynchronize(s)); t_2 = gab_now_ms(); }
    // virtual slab origins: device address of byte 0 of the caller's slabs
    rc = bsw_run_device_impl(h, (const uint8_t *)(b + o_ref) - ra, ra + (int64_t)rpad, (const int64_t *)(b + o_roff),
                             (const uint8_t *)(b + o_qry) - qa, qa + (int64_t)qpad, (const int64_t *)(b + o_qoff),
                             (const int32_t *)(b + o_l1), (const int32_t *)(b + o_l2), (const int32_t *)(b + o_h0),
                             n, (int32_t *)(b + o_sc), nullptr, s, ra, qa, rb, qb);      // (rb / qb: a pair that ends in the window's padding was not copied)
    if (rc == GAB_EINVAL && sampled) {
        // a pair outside the sampled window (sequences not in pair order) -- or a really invalid one: the full scan tells
        h->out_of_order = true;
        return gab_bsw_run(h, ref, ref_off, qry, qry_off, len1, len2, h0, n, score_out);
    }
    if (rc) return rc;
    double t_3 = 0;
    if (trace) { GAB_HIP(hipStreamSynchronize(s)); t_3 = gab_now_ms(); }
    GAB_HIP(hipMemcpyAsync(score_out, b + o_sc, 4 * nn, hipMemcpyDeviceToHost, s));
    GAB_HIP(hipStreamSynchronize(s));
    if (trace)
        fprintf(stderr, "[gab_bsw_run %p] %lld pairs: host scan %.2f ms, H2D of %.1f MB %.2f ms, sort + DP %.2f ms, D2H %.2f ms\n", (void *)h,
                (long long)n, t_1 - t_0, (double)((rb - ra) + (qb - qa) + 28 * n) / 1e6, t_2 - t_1, t_3 - t_2, gab_now_ms() - t_3);
    return GAB_OK;
}

// Pre-size the handle's device buffers (staging of the host-pointer entry point + the sort workspace) for calls of up to
// max_pairs pairs / the given slab windows, so that the first gab_bsw_run inside a timed region does not pay for them (the
// reference allocates its per-thread F16_ / H16_ buffers in the BandedPairWiseSW constructor, bandedSWA.cpp:80-96).
extern "C" int gab_bsw_reserve(gab_bsw *h, int64_t max_pairs, int64_t max_ref_bytes, int64_t max_qry_bytes) {
    GAB_CHECK(h, "gab_bsw_reserve: NULL handle");
    GAB_CHECK(max_pairs >= 0 && max_pairs < (1ll << 31) && max_ref_bytes >= 0 && max_qry_bytes >= 0, "gab_bsw_reserve: size out of range");
    gab_device_guard g(h->device);
    const size_t nn = (size_t)max_pairs;
    int rc = h->io.reserve(std::max<size_t>((((size_t)max_ref_bytes + 3 + 511) & ~(size_t)255) + (((size_t)max_qry_bytes + 3 + 511) & ~(size_t)255) + 32 * nn + 1024,
                                            (size_t)4 << 20));      // (at least the 4 MB gab_warm_copy_engines moves)
    if (rc) return rc;
    rc = h->ws.reserve(BswLayout(nn).total);
    if (rc) return rc;
    hipStream_t s = nullptr;
    if ((rc = h->hs.get(&s)) != GAB_OK) return rc;
    // touch the memory and load the kernels' code objects once
    GAB_HIP(hipMemsetAsync(h->io.p, 0, h->io.cap, s));
    GAB_HIP(hipMemsetAsync(h->ws.p, 0, h->ws.cap, s));
    GAB_HIP(hipStreamSynchronize(s));
    if ((rc = gab_warm_copy_engines(s, h->io.p, h->io.cap)) != GAB_OK) return rc;
    // ... and one tiny batch through the whole path: the first launch of every kernel (code object, the runtime's per-kernel
    // bookkeeping, the auxiliary streams' queues) costs milliseconds once per process and handle -- not inside the caller's ROI
    // (the drop-in driver with the GPU parser: 55.7 ms for a step that takes 45)
    static const uint8_t seq[40] = {0, 1, 2, 3, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 0, 1, 2, 3, 3, 2, 1, 0, 0, 0, 0, 0};
    const int64_t ro[2] = {0, 4}, qo[2] = {2, 8};
    const int32_t l1[2] = {24, 20}, l2[2] = {20, 16}, h0[2] = {10, 0};
    int32_t sc[2];
    const bool had = h->have_stats;
    rc = gab_bsw_run(h, seq, ro, seq, qo, l1, l2, h0, 2, sc);
    h->have_stats = had;
    return rc;
}

extern "C" int gab_bsw_last_stats(gab_bsw *h, int64_t *cells, float *kernel_ms, float *total_ms) {
    GAB_CHECK(h, "gab_bsw_last_stats: NULL handle");
    GAB_CHECK(h->have_stats, "gab_bsw_last_stats: no completed run on this handle");
    gab_device_guard g(h->device);
    GAB_HIP(hipEventSynchronize(h->ev[3]));
    if (cells) {
        *cells = 0;
        for (int k = 0; k < h->stat_slices; k++) *cells += (int64_t)h->h_stats[k]->cells;
    }
    if (kernel_ms) GAB_HIP(hipEventElapsedTime(kernel_ms, h->ev[1], h->ev[2]));
    if (total_ms) GAB_HIP(hipEventElapsedTime(total_ms, h->ev[0], h->ev[3]));
    return GAB_OK;
}
