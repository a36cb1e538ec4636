"""numpy model of the kmer-cnt benchmark (helper, not a test): what KmerCounter::count(true) computes, COUNT_VERSION == 3
(kmer-cnt/vertex_index.cpp:787-860), with the quirks that decide the printed numbers.

1. file reading (kmer-cnt/sequence_container.cpp:159-328): FASTA / FASTQ, plain or gzip; a byte that is not one of ACGTacgt turns
   itself and the rest of its 32-base word of the record into T (unknown_to_t below says why: the reference's rand() replacement
   never runs on a 64-bit machine);
2. only reads LONGER than min_len are kept;
3. forward strand only, positions 0 .. L - k - 1: L - k k-mers, the last one of every read is never visited (kmer-cnt/kmer.h:177-198);
4. a k-mer is a 2k-bit number, first base most significant, A C G T = 0 1 2 3; canonical = min(itself, reverse complement);
5. one wrapping 8-bit counter per k-mer: Total k-mers = sum ceil(c / 256), Hash size = #(c >= 256).
"""
import gzip

import numpy as np

RUN = 64        # GAB_KMER_RUN (include/gab.h): a GPU lane's run of positions; merges are counted inside runs only

_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def canonical_kmers(read, k):
    """bytes (ACGTacgt only) -> uint64 canonical k-mers at positions 0 .. L - k - 1"""
    codes = _CODE[np.frombuffer(read, np.uint8)]
    assert not (codes == 255).any(), "the model takes ACGTacgt only (replace the other bytes first)"
    n = len(read) - k
    if n <= 0:
        return np.zeros(0, np.uint64)
    c = codes.astype(np.uint64)
    fw = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | c[j:j + n]
        rc = rc | ((np.uint64(3) - c[j:j + n]) << np.uint64(2 * j))
    return np.minimum(fw, rc)


def revcomp_value(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (~x & 3)
        x >>= 2
    return r


def model(reads, k, min_len=5000):
    """list of bytes -> dict: the six result fields, the sorted k-mers with their exact counts, and the merges of equal
    neighbouring keys inside runs of RUN positions (run boundaries at the multiples of RUN within a read)"""
    kept = [r for r in reads if len(r) > min_len]
    parts = [canonical_kmers(r, k) for r in kept]
    merged = 0
    for p in parts:
        if p.size > 1:
            same = p[1:] == p[:-1]
            same[RUN - 1::RUN] = False          # position i (= index i - 1 of `same`) starts a run when i % RUN == 0
            merged += int(same.sum())
    allk = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    kmers, counts = np.unique(allk, return_counts=True)
    counts = counts.astype(np.int64)
    return {"reads_kept": len(kept), "positions": int(allk.size), "distinct": int(kmers.size),
            "total_kmers": int(((counts + 255) // 256).sum()), "hash_size": int((counts >= 256).sum()),
            "max_count": int(counts.max()) if counts.size else 0, "kmers": kmers.astype(np.uint64), "counts": counts, "merged": merged}


FIELDS = ("reads_kept", "positions", "distinct", "total_kmers", "hash_size", "max_count")


def spectrum(counts, nbins):
    return np.bincount(np.minimum(counts, nbins - 1), minlength=nbins).astype(np.int64)


# ---- file reading -------------------------------------------------------------------------------------------------------------------
def _open(path):
    return gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")


def _is_fasta(path):
    base = path[:-3] if path.endswith(".gz") else path
    suffix = base.rsplit(".", 1)[-1]
    if suffix in ("fasta", "fa"):
        return True
    if suffix in ("fastq", "fq"):
        return False
    raise ValueError("Can't identify input file type: " + path)


def _valid(line):
    return _CODE[np.frombuffer(line, np.uint8)] != 255


def read_records_raw(path):
    """the records of one file as lists of sequence LINES (bytes), bytes not yet replaced"""
    recs = []
    with _open(path) as f:
        lines = [ln.rstrip(b"\r") for ln in f.read().split(b"\n")]
    if _is_fasta(path):
        cur = None
        for ln in lines:
            if not ln:
                continue
            if ln.startswith(b">"):
                cur = []
                recs.append(cur)
            else:
                cur.append(ln)
    else:
        state = 0
        for ln in lines:
            if ln and state == 1:
                recs.append([ln])
            state = (state + 1) % 4
    return recs


def unknown_to_t(read):
    """what the reference makes of a byte outside ACGTacgt.  validateSequence (kmer-cnt/sequence_container.cpp:318-328) means to
    replace it by "ACGT"[rand() % 4], but compares a size_t table entry of -1 with -1U: never equal where size_t has 64 bits (which
    kmer-cnt/kmer.h:14 asserts), so nothing is replaced and rand() is never called.  The 2-bit packing (kmer-cnt/sequence.h:54-69) then
    ORs the all-ones entry, shifted to the base's place, into the record's 32-base word: that base and every later base of the
    word read as T.  Positions count from the start of the record (its lines joined)."""
    bad = np.flatnonzero(~_valid(read))
    if not bad.size:
        return read
    b = np.frombuffer(read, np.uint8).copy()
    for i in bad:
        b[i:(i // 32 + 1) * 32] = ord("T")
    return b.tobytes()


def load_reads(paths):
    """every record of the files, in order, as the reference's containers hold them"""
    return [unknown_to_t(b"".join(lines)) for p in paths for lines in read_records_raw(p)]


def model_files(paths, k, min_len=5000):
    return model(load_reads(paths), k, min_len)
