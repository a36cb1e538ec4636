"""helpers of the key-space partition tests (not a test): a numpy restatement of the k-mer counter's hash, partition and table-line
arithmetic (genarchbench_amd/csrc/kmer.hip: kmer_hash, part_of, line_of), and tests/kmer_model.py restricted to one partition.

    h    = mix(key)                                  the 64-bit hash
    part = hi64(h * nparts)                          in [0, nparts)
    line = hi64((h * nparts mod 2^64) * nlines)      the fraction of the same product, uniform over [0, nlines) inside a partition
"""
import numpy as np

from tests import kmer_model

_U = np.uint64
SLOTS = 8        # per 128-byte table line


def np_hash(keys):
    with np.errstate(over="ignore"):
        h = np.asarray(keys, _U) * _U(0x9E3779B97F4A7C15)
        h ^= h >> _U(29)
        h = h * _U(0xBF58476D1CE4E5B9)
        return h ^ (h >> _U(32))


def np_umulhi(a, b):
    """high 64 bits of a * b for uint64 a and an integer 0 < b < 2^32: with a = ah 2^32 + al, (ah b + (al b >> 32)) >> 32 -- no
    term passes 2^64"""
    assert 0 < b < 1 << 32
    a = np.asarray(a, _U)
    ah, al = a >> _U(32), a & _U(0xFFFFFFFF)
    return (ah * _U(b) + ((al * _U(b)) >> _U(32))) >> _U(32)


def np_part_of(keys, nparts):
    return np_umulhi(np_hash(keys), nparts).astype(np.int64)


def np_line_of(keys, nparts, nlines):
    with np.errstate(over="ignore"):
        return np_umulhi(np_hash(keys) * _U(nparts), nlines).astype(np.int64)


def no_line_overfull(keys, nparts, nlines):
    """True when no table line is the home line of more than SLOTS of `keys`: then every insert ends in the first line it visits,
    whatever the order of the inserts, and `probes` is exactly the number of inserts"""
    if len(keys) == 0:
        return True
    return int(np.bincount(np_line_of(keys, nparts, nlines)).max()) <= SLOTS


def merged_keys(reads, k, min_len=5000):
    """the key of every position that kmer_model.model counts as merged into its predecessor (same rule, same run boundaries)"""
    out = []
    for r in reads:
        if len(r) <= min_len:
            continue
        p = kmer_model.canonical_kmers(r, k)
        if p.size > 1:
            same = p[1:] == p[:-1]
            same[kmer_model.RUN - 1::kmer_model.RUN] = False
            out.append(p[1:][same])
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def restrict(m, mk, nparts, part_of=np_part_of):
    """kmer_model.model's result m and merged_keys mk of one input -> [m_0 .. m_{nparts-1}], the model restricted to every
    partition: the six fields (reads_kept and positions are the whole call's), the sorted k-mers with their counts, the merges of
    keys the partition owns and its inserts (positions of its keys that were not merged)"""
    owner = part_of(m["kmers"], nparts)
    assert mk.size == m["merged"]
    merged = np.bincount(part_of(mk, nparts), minlength=nparts) if mk.size else np.zeros(nparts, np.int64)
    out = []
    for p in range(nparts):
        kmers, counts = m["kmers"][owner == p], m["counts"][owner == p]
        out.append({"reads_kept": m["reads_kept"], "positions": m["positions"], "distinct": int(kmers.size),
                    "total_kmers": int(((counts + 255) // 256).sum()), "hash_size": int((counts >= 256).sum()),
                    "max_count": int(counts.max()) if counts.size else 0, "kmers": kmers, "counts": counts, "merged": int(merged[p]),
                    "inserts": int(counts.sum()) - int(merged[p])})
    return out


def fields(m):
    return {f: m[f] for f in kmer_model.FIELDS}
