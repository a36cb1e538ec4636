"""Plain Python / numpy model of the minimizer index of the kmer-cnt benchmark (helper, not a test): what
VertexIndex::buildIndexMinimizers(1, window) computes (kmer-cnt/vertex_index.cpp:394-502) and what it prints.

1. reads as in tests/kmer_model.py: only reads LONGER than min_len, forward strand, positions 0 .. L - k - 1;
2. the sketch of one read is yieldMinimizers (kmer-cnt/kmer.h:206-262), written out below step by step with the same queue: the
   order key of a position is the splitmix64 finaliser (kmer-cnt/kmer.h:91-98) of its canonical k-mer; entries with a strictly
   greater key are popped from the back; when the front has left the window the expired fronts are popped AND THEN the front moves on
   to the last of a leading run of equal keys (the tie rule: `tie_rule=False` leaves that second loop out, which is what a
   text-book sliding-window minimum would do); after every step the front is emitted if it is not the last emitted position;
3. capacity(x) = emitted minimizers with canonical k-mer x; mean = (float)total / (unique + 1); repetitive_frequency =
   (size_t)(rate * mean) in C float arithmetic (filterFrequentKmers, kmer-cnt/vertex_index.cpp:178-217); keys with capacity >
   repetitive_frequency are removed;
4. kept read i of length L_i after S_i earlier bases owns the global positions [2 S_i, 2 S_i + L_i) forward and
   [2 S_i + L_i, 2 S_i + 2 L_i) reverse complement (kmer-cnt/sequence_container.cpp:359-370); a minimizer at p is entered at
   2 S_i + p when its forward k-mer is canonical (fw <= rc), at 2 S_i + L_i + (L_i - p - k) otherwise; every list ascending.
"""
import collections
import hashlib

import numpy as np

from tests import kmer_model

MAX_WINDOW = 255        # GAB_KMER_MAX_WINDOW (include/gab.h)


def hash64(x):
    """kmer-cnt/kmer.h:91-98 on a uint64 array"""
    with np.errstate(over="ignore"):
        z = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def strands(read, k):
    """bytes -> (forward k-mers, reverse-complement k-mers) at positions 0 .. L - k - 1, uint64"""
    codes = kmer_model._CODE[np.frombuffer(read, np.uint8)]
    assert not (codes == 255).any(), "the model takes ACGTacgt only"
    n = len(read) - k
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    c = codes.astype(np.uint64)
    fw = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | c[j:j + n]
        rc = rc | ((np.uint64(3) - c[j:j + n]) << np.uint64(2 * j))
    return fw, rc


def sketch_of_hashes(hashes, window, tie_rule=True):
    """the queue of yieldMinimizers over a list of order keys -> emitted positions"""
    if window < 1:
        raise ValueError("wrong minimizer length")
    n = len(hashes)
    if window == 1:
        return list(range(n))
    out = []
    q = collections.deque()         # (position, key)
    for p in range(n):
        h = hashes[p]
        while q and q[-1][1] > h:
            q.pop()
        q.append((p, h))
        if q[0][0] <= p - window:
            while q[0][0] <= p - window:
                q.popleft()
            if tie_rule:
                while len(q) >= 2 and q[0][1] == q[1][1]:
                    q.popleft()
        if not out or out[-1] != q[0][0]:
            out.append(q[0][0])
    return out


def sketch(read, k, window, tie_rule=True):
    """bytes -> int32 array of the minimizer positions of the read, ascending"""
    fw, rc = strands(read, k)
    return np.array(sketch_of_hashes(hash64(np.minimum(fw, rc)).tolist(), window, tie_rule), np.int32)


def sketch_reads(reads, k, window, min_len=5000, tie_rule=True):
    """what gab_kmer_sketch returns: (read_start int64 [n + 1], pos int32); a filtered or too-short read has an empty range"""
    lists = [sketch(r, k, window, tie_rule) if len(r) > min_len else np.zeros(0, np.int32) for r in reads]
    start = np.zeros(len(reads) + 1, np.int64)
    if reads:
        start[1:] = np.cumsum([x.size for x in lists])
    return start, (np.concatenate(lists) if lists else np.zeros(0, np.int32)).astype(np.int32)


def repetitive_frequency(total, unique, rate):
    """filterFrequentKmers' threshold with its C float operations"""
    mean = np.float32(total) / np.float32(unique + 1)
    return int(np.float32(rate) * mean)


def entries(reads, k, window, min_len=5000, tie_rule=True):
    """every emitted minimizer of the kept reads -> (canonical k-mers uint64, global positions int64), kept reads, their bases"""
    keys, gpos = [], []
    base = 0
    kept = 0
    for r in reads:
        if len(r) <= min_len:
            continue
        kept += 1
        L = len(r)
        fw, rc = strands(r, k)
        p = np.array(sketch_of_hashes(hash64(np.minimum(fw, rc)).tolist(), window, tie_rule), np.int64)
        if p.size:
            f, c = fw[p], rc[p]
            forward = f <= c
            keys.append(np.where(forward, f, c))
            gpos.append(np.where(forward, 2 * base + p, 2 * base + L + (L - p - k)))
        base += L
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)  # noqa: E731
    return cat(keys, np.uint64), cat(gpos, np.int64), kept, base


def build_index(reads, k, window, rate, min_len=5000, tie_rule=True):
    """-> dict: the nine fields of gab_kmer_index_result, `kmers` (ascending), `start` (nk + 1), `gpos` (each list ascending),
    `repetitive` (the removed k-mers, ascending)"""
    return index_of_entries(entries(reads, k, window, min_len, tie_rule), rate)


def index_of_entries(found, rate):
    """build_index from the result of entries(): the part that depends on the rate"""
    keys, gpos, kept, total_len = found
    uniq, inv, cap = np.unique(keys, return_inverse=True, return_counts=True)
    total, unique = int(keys.size), int(uniq.size)
    thr = repetitive_frequency(total, unique, rate)
    gone = cap > thr
    keep = ~gone[inv]
    order = np.lexsort((gpos[keep], keys[keep]))
    kmers = uniq[~gone]
    start = np.zeros(kmers.size + 1, np.int64)
    start[1:] = np.cumsum(cap[~gone])
    return {"reads_kept": kept, "total_len": total_len, "minimizers": total, "distinct": unique, "repetitive_frequency": thr,
            "filtered_kmers": int(gone.sum()), "filtered_entries": int(cap[gone].sum()), "selected_kmers": int(kmers.size),
            "index_entries": int(start[-1]), "kmers": kmers.astype(np.uint64), "start": start, "gpos": gpos[keep][order].astype(np.int64),
            "repetitive": uniq[gone].astype(np.uint64)}


FIELDS = ("reads_kept", "total_len", "minimizers", "distinct", "repetitive_frequency", "filtered_kmers", "filtered_entries",
          "selected_kmers", "index_entries")


def _g(x):
    return "%g" % float(x)


def printed(m):
    """the reference's debug lines, in its order, as (label, text): integers as they are, floats as its ostream writes them (%g of
    a float computed with the same float expressions, kmer-cnt/vertex_index.cpp:190-216, 494-500)"""
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = f32(m["minimizers"]) / f32(m["distinct"] + 1)
        rate = f32(m["filtered_entries"]) / f32(m["minimizers"])
        mean_kept = f32(m["index_entries"]) / f32(m["selected_kmers"])
        mini = f32(m["total_len"]) / f32(m["index_entries"])
    return {"mean_frequency": _g(mean), "repetitive_frequency": m["repetitive_frequency"], "filtered_entries": m["filtered_entries"],
            "filtered_rate": _g(rate), "selected_kmers": m["selected_kmers"], "index_entries": m["index_entries"],
            "mean_frequency_kept": _g(mean_kept), "minimizer_rate": _g(mini)}


def serialise(kmers, start, gpos):
    """k-mers ascending, each followed by its ascending global positions, as little-endian int64"""
    kmers = np.asarray(kmers).astype(np.int64); start = np.asarray(start, np.int64); gpos = np.asarray(gpos, np.int64)
    out = np.zeros(kmers.size + gpos.size, "<i8")
    at = start[:-1] + np.arange(kmers.size)
    is_key = np.zeros(out.size, bool)
    is_key[at] = True
    out[is_key] = kmers
    out[~is_key] = gpos
    return out.tobytes()


def digest(kmers, start, gpos):
    return hashlib.sha256(serialise(kmers, start, gpos)).hexdigest()
