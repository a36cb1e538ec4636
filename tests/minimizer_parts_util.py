"""helpers of the partitioned minimizer-index tests (not a test): tests/minimizer_model.py restricted to every key-space partition.

A partition owns the canonical k-mers whose hash falls to it (tests/kmer_parts_util.py: np_part_of, the numpy restatement of
gab_kmer_part_of).  Its own numbers are those of its keys alone; the ONE thing it shares with the others is the filter's threshold,
which comes from the totals of the whole input: repetitive_frequency(all minimizers, all distinct k-mers, rate)."""
import numpy as np

from tests import minimizer_model as mm
from tests.kmer_parts_util import np_part_of

OWN_FIELDS = ("minimizers", "distinct", "filtered_kmers", "filtered_entries", "selected_kmers", "index_entries")      # these add up
SLOTS = 8        # per 128-byte table line


def index_with_threshold(keys, gpos, kept, total_len, thr):
    """minimizer_model.index_of_entries with the threshold given instead of computed from these entries"""
    uniq, inv, cap = np.unique(keys, return_inverse=True, return_counts=True)
    gone = cap > thr
    keep = ~gone[inv] if keys.size else np.zeros(0, bool)
    order = np.lexsort((gpos[keep], keys[keep]))
    kmers = uniq[~gone]
    start = np.zeros(kmers.size + 1, np.int64)
    start[1:] = np.cumsum(cap[~gone])
    return {"reads_kept": kept, "total_len": total_len, "minimizers": int(keys.size), "distinct": int(uniq.size), "repetitive_frequency": thr,
            "filtered_kmers": int(gone.sum()), "filtered_entries": int(cap[gone].sum()), "selected_kmers": int(kmers.size),
            "index_entries": int(start[-1]), "kmers": kmers.astype(np.uint64), "start": start, "gpos": gpos[keep][order].astype(np.int64),
            "repetitive": uniq[gone].astype(np.uint64), "capacities": cap.astype(np.int64), "keys": uniq.astype(np.uint64)}


def restrict(found, rate, nparts, part_of=np_part_of):
    """the result of minimizer_model.entries() -> [m_0 .. m_{nparts-1}]: the model of every partition -- its nine fields (reads_kept,
    total_len and repetitive_frequency are the whole input's), `kmers`, `start`, `gpos`, `repetitive` as minimizer_model.build_index
    gives them, and its own `keys` with their `capacities`"""
    keys, gpos, kept, total_len = found
    thr = mm.repetitive_frequency(int(keys.size), int(np.unique(keys).size), rate)
    owner = part_of(keys, nparts) if keys.size else np.zeros(0, np.int64)
    return [index_with_threshold(keys[owner == p], gpos[owner == p], kept, total_len, thr) for p in range(nparts)]


def begin_fields(mp):
    """what phase 1 reports for the partition of model mp"""
    return dict({f: 0 for f in mm.FIELDS}, reads_kept=mp["reads_kept"], total_len=mp["total_len"], minimizers=mp["minimizers"], distinct=mp["distinct"])


def fields(mp):
    return {f: mp[f] for f in mm.FIELDS}


def sum_fields(parts):
    """the nine fields of the whole input from those of its partitions"""
    out = {f: parts[0][f] for f in ("reads_kept", "total_len", "repetitive_frequency")}
    out.update({f: sum(p[f] for p in parts) for f in OWN_FIELDS})
    return {f: out[f] for f in mm.FIELDS}


def merge(dumps):
    """[(kmers, start, gpos) of every partition] -> the one index: k-mers ascending, every list as it was, start recomputed"""
    kmers = np.concatenate([np.asarray(d[0], np.uint64) for d in dumps])
    lists = [np.asarray(d[2], np.int64)[d[1][i]:d[1][i + 1]] for d in dumps for i in range(len(d[0]))]
    assert np.unique(kmers).size == kmers.size, "two partitions hold the same k-mer"
    order = np.argsort(kmers, kind="stable")
    start = np.zeros(kmers.size + 1, np.int64)
    if kmers.size:
        start[1:] = np.cumsum([lists[i].size for i in order])
    gpos = np.concatenate([lists[i] for i in order]) if kmers.size else np.zeros(0, np.int64)
    return kmers[order], start, gpos.astype(np.int64)


def positions_of(reads, k, min_len):
    return int(sum(max(len(r) - k, 0) for r in reads if len(r) > min_len))


def first_table_room(positions, k, nparts):
    """keys the first capacity table of a partition is sized for (genarchbench_amd/csrc/kmer.hip: part_table_lines): the even share
    of min(positions, 4^k) keys, plus a quarter, plus 64 -- its slots are twice that, so a partition with no more keys than this
    leaves the table at most half full and its bounded inserts cannot give up"""
    keys = min(max(positions, 1), 4 ** k)
    share = (keys + nparts - 1) // nparts
    return share + share // 4 + 64


def first_table_slots(positions, k, nparts):
    """... and its slots: never more than the unpartitioned table, never fewer than 16 lines"""
    keys = min(max(positions, 1), 4 ** k)
    lines = lambda room: max(16, (2 * room + SLOTS - 1) // SLOTS)  # noqa: E731
    return min(lines(keys), lines(first_table_room(positions, k, nparts))) * SLOTS
