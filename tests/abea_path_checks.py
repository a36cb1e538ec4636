"""What the reference's align() computes from its path but does not return (abea/src/align.c:441-524), computed again from a path and
the read alone.  Independent of abea_model.align: no band, no trace, no score; only the pairs.

  end_event          the event of the last pair (the backtrack starts there)
  max_gap            the longest run of skips: consecutive pairs on one event whose k-mer goes up by one
  avg_log_emission   the float emission of every pair (log_normal_pdf, every operation rounded to float on its own), added in double
                     from the last pair to the first (align.c:462-465), divided by the number of pairs (align.c:515)
  flags              LOW_EMISSION: avg < -5.0; NOT_SPANNED: the first pair's k-mer is not 0 (the last pair's is the last k-mer by
                     construction); GAP: max_gap > 50

One move is not in the coordinates: the one that leaves the first pair.  When the first pair is on k-mer 0, the backtrack may leave
it by a skip into the trim column, which lengthens the run of skips at the front of the path by one.  For a first pair (0, 0) the
three scores of that cell are known without the band (the start cell, nothing above, the first trim cell; all three always inside
bands 0 to 2), so the move is computed here.  For a first pair (0, e > 0) it cannot be known from the pairs; then, and only when the
longer front run would be the longest, `admissible` holds both (max_gap, flags) values."""
import math

import numpy as np

import abea_model as M

F = np.float32


def emissions(seq, events, mean, stdv, log_stdv, scale, shift, path):
    """float32 emission of every pair of the path, each operation rounded on its own (log_probability_match_r9, log_normal_pdf)"""
    ranks = M.kmer_ranks(seq)[path[:, 0]]
    x = np.asarray(events, F)[path[:, 1]]
    gp_mean = F(scale) * np.asarray(mean, F)[ranks] + F(shift)
    with np.errstate(all="ignore"):
        a = (x - gp_mean) / np.asarray(stdv, F)[ranks]
        lp = (F(-0.918938) - np.asarray(log_stdv, F)[ranks]) + ((F(-0.5) * a) * a)
    assert lp.dtype == F
    return lp


def recompute(seq, events, mean, stdv, log_stdv, scale, shift, path):
    """path: (n, 2) of (ref_pos, read_pos) in read order, n >= 1 -> dict(end_event, max_gap, flags, avg_log_emission, admissible)"""
    path = np.asarray(path, np.int64).reshape(-1, 2)
    n_kmers, n_events = len(seq) - M.K + 1, np.size(events)
    assert len(path) >= 1 and path[-1, 0] == n_kmers - 1
    lp = emissions(seq, events, mean, stdv, log_stdv, scale, shift, path)
    total = 0.0
    for v in lp[::-1]:
        total += float(v)
    avg = total / float(len(path))

    skip = (np.diff(path[:, 1]) == 0) & (np.diff(path[:, 0]) == 1)       # the move from pair i + 1 back to pair i
    runs, run = [], 0
    for s in skip:
        run = run + 1 if s else 0
        runs.append(run)
    front = 0                                                           # the run of skips that ends at the first pair
    for s in skip:
        if not s:
            break
        front += 1
    gap = max(runs, default=0)
    gaps = [gap]
    if path[0, 0] == 0 and path[0, 1] == 0:
        events_per_kmer = n_events / n_kmers
        lp_stay = math.log(1 - 1 / (events_per_kmer + 1))
        lp_step = math.log(1.0 - math.exp(math.log(1e-10)) - math.exp(lp_stay))
        with np.errstate(all="ignore"):
            score_d = F((0.0 + lp_step) + float(lp[0]))                  # the start cell; the cell above is never filled
            score_l = F(float(F(math.log(0.01))) + math.log(1e-10))      # the first trim cell
        best = score_d
        best = score_l if score_l > best else best
        if best == score_l:                                              # (the stay's score is -inf or NaN: it never equals a larger score_l)
            gaps = [max(gap, front + 1)]
    elif path[0, 0] == 0 and front + 1 > gap:
        gaps.append(front + 1)

    def flags_of(g):
        return (M.LOW_EMISSION if avg < -5.0 else 0) | (M.NOT_SPANNED if path[0, 0] != 0 else 0) | (M.GAP if g > 50 else 0)
    return dict(end_event=int(path[-1, 1]), max_gap=gaps[0], flags=flags_of(gaps[0]), avg_log_emission=avg,
                admissible=[(g, flags_of(g)) for g in gaps])


def agrees(rec, chk):
    """a record (the model's or the library's) against the recomputation: equality on the four fields, avg_log_emission as equal
    doubles, max_gap and flags one of the admissible pairs"""
    return (int(rec["end_event"]) == chk["end_event"] and (int(rec["max_gap"]), int(rec["flags"])) in chk["admissible"]
            and np.float64(rec["avg_log_emission"]).tobytes() == np.float64(chk["avg_log_emission"]).tobytes()
            and int(rec["n_pairs"]) == (0 if int(rec["flags"]) else int(rec["path_len"])))
