"""Plain numpy model of the solid k-mer index of the kmer-cnt benchmark (helper, not a test): what
VertexIndex::buildIndexUnevenCoverage(globalMinFreq, selectRate, tandemFreq) computes (kmer-cnt/vertex_index.cpp:30-130, its
selector yieldFrequentKmers at kmer-cnt/vertex_index.cpp:321-363) and what it prints, with getFreq as the exact count.

Reads, positions, canonical form and global positions as in tests/kmer_model.py and tests/minimizer_model.py; c(x) = the exact
count of canonical k-mer x over the kept reads.  Per kept read with n = L - k > 0 positions and f[p] = c(k-mer at p):
1. cut = element of rank (size_t)(select_rate * (float)n) of f in descending order (float product, truncated; rank n - 1 where the
   product reaches n, which the reference does not survive);
2. positions with f[p] >= cut stay;
3. tandem_freq > 0: positions whose canonical k-mer occurs more than tandem_freq times in the read go;
4. positions with f[p] < min_freq go.
capacity(x) = selected positions with k-mer x.  The filter's mean runs over capacities >= min_freq; keys with capacity >
repetitive_frequency are removed; of the others those with c(x) <= repetitive_frequency get their positions, the rest an empty list.
"""
import numpy as np

from tests import kmer_model, minimizer_model

FIELDS = ("reads_kept", "total_len", "positions", "selected_positions", "candidates", "mean_total", "mean_unique", "repetitive_frequency",
          "filtered_kmers", "filtered_entries", "selected_kmers", "indexed_kmers", "index_entries")


def rank_of(select_rate, n):
    """(size_t)(selectRate * topKmers.size()) in C float arithmetic, held inside the array"""
    return min(int(np.float32(select_rate) * np.float32(n)), n - 1)


def select_read(keys, f, min_freq, select_rate, tandem):
    """canonical k-mers and their global counts at the positions of one read -> the selected positions, ascending (int64)"""
    n = keys.size
    if n == 0:
        return np.zeros(0, np.int64)
    cut = np.sort(f)[::-1][rank_of(select_rate, n)]
    keep = f >= cut
    if tandem > 0:
        _, inv, local = np.unique(keys, return_inverse=True, return_counts=True)
        keep &= local[inv] <= tandem
    keep &= f >= min_freq
    return np.flatnonzero(keep).astype(np.int64)


def counts_of(reads, k, min_len):
    """-> (sorted canonical k-mers, their exact counts int64) over the kept reads"""
    parts = [kmer_model.canonical_kmers(r, k) for r in reads if len(r) > min_len]
    allk = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    kmers, counts = np.unique(allk, return_counts=True)
    return kmers, counts.astype(np.int64)


def positions(reads, k, min_freq, select_rate, tandem, min_len=5000):
    """what gab_kmer_solid_positions returns: (read_start int64 [n + 1], pos int32)"""
    kmers, counts = counts_of(reads, k, min_len)
    lists = []
    for r in reads:
        if len(r) <= min_len or len(r) <= k:
            lists.append(np.zeros(0, np.int64))
            continue
        keys = kmer_model.canonical_kmers(r, k)
        lists.append(select_read(keys, counts[np.searchsorted(kmers, keys)], min_freq, select_rate, tandem))
    start = np.zeros(len(reads) + 1, np.int64)
    if reads:
        start[1:] = np.cumsum([x.size for x in lists])
    return start, (np.concatenate(lists) if lists else np.zeros(0, np.int64)).astype(np.int32)


def build_index(reads, k, min_freq, select_rate, tandem, rate, min_len=5000):
    """-> dict: the fields of gab_kmer_solid_result, `kmers` (the non-empty lists' keys, ascending), `start`, `gpos` (each list
    ascending), `empty` (kept keys with an empty list) and `repetitive` (removed keys), both ascending"""
    kmers, counts = counts_of(reads, k, min_len)
    keys, gpos = [], []
    base = kept = npos = 0
    for r in reads:
        if len(r) <= min_len:
            continue
        kept += 1
        L = len(r)
        fw, rc = minimizer_model.strands(r, k)
        canon = np.minimum(fw, rc)
        npos += canon.size
        p = select_read(canon, counts[np.searchsorted(kmers, canon)], min_freq, select_rate, tandem)
        if p.size:
            forward = fw[p] <= rc[p]
            keys.append(canon[p])
            gpos.append(np.where(forward, 2 * base + p, 2 * base + L + (L - p - k)))
        base += L
    keys = np.concatenate(keys).astype(np.uint64) if keys else np.zeros(0, np.uint64)
    gpos = np.concatenate(gpos).astype(np.int64) if gpos else np.zeros(0, np.int64)
    uniq, inv, cap = np.unique(keys, return_inverse=True, return_counts=True)
    glob = counts[np.searchsorted(kmers, uniq)] if uniq.size else np.zeros(0, np.int64)
    mean = cap >= min_freq
    total, unique = int(cap[mean].sum()), int(mean.sum())
    thr = minimizer_model.repetitive_frequency(total, unique, rate)
    gone = cap > thr
    empty = ~gone & (glob > thr)
    full = ~gone & ~empty
    take = full[inv]
    order = np.lexsort((gpos[take], keys[take]))
    start = np.zeros(int(full.sum()) + 1, np.int64)
    start[1:] = np.cumsum(cap[full])
    return {"reads_kept": kept, "total_len": base, "positions": npos, "selected_positions": int(keys.size), "candidates": int(uniq.size),
            "mean_total": total, "mean_unique": unique, "repetitive_frequency": thr, "filtered_kmers": int(gone.sum()),
            "filtered_entries": int(cap[gone].sum()), "selected_kmers": int((~gone).sum()), "indexed_kmers": int(full.sum()),
            "index_entries": int(start[-1]), "kmers": uniq[full].astype(np.uint64), "start": start, "gpos": gpos[take][order].astype(np.int64),
            "empty": uniq[empty].astype(np.uint64), "repetitive": uniq[gone].astype(np.uint64)}


def _g(x):
    """%g; 0 / 0 is the x86 default NaN, whose sign bit is set: the reference's ostream, like printf, writes "-nan" """
    return "-nan" if np.isnan(x) else "%g" % float(x)


def printed(m):
    """the reference's six debug lines, in its order (kmer-cnt/vertex_index.cpp:209-216, 126-129): integers as they are, floats as
    its ostream writes them (%g of a float computed with the same float expressions)"""
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = f32(m["mean_total"]) / f32(m["mean_unique"] + 1)
        rate = f32(m["filtered_entries"]) / f32(m["mean_total"])
        mean_kept = f32(m["index_entries"]) / f32(m["selected_kmers"])
    return {"mean_frequency": _g(mean), "repetitive_frequency": m["repetitive_frequency"], "filtered_entries": m["filtered_entries"],
            "filtered_rate": _g(rate), "selected_kmers": m["selected_kmers"], "index_entries": m["index_entries"],
            "mean_index_frequency": _g(mean_kept)}
