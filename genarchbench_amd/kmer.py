"""Host-side mirror of KmerCounter::count (kmer-cnt/vertex_index.cpp:787-860) over the C ABI, whole or in key-space partitions
(include/gab.h: gab_kmer_count_part), and of the minimizer index, VertexIndex::buildIndexMinimizers (kmer-cnt/vertex_index.cpp:394-502;
include/gab.h: gab_kmer_sketch, gab_kmer_index_minimizers), whole or in key-space partitions built in two phases
(gab_kmer_index_part_begin / gab_kmer_index_part_finish), and of the solid k-mer index, VertexIndex::buildIndexUnevenCoverage
(kmer-cnt/vertex_index.cpp:30-130; include/gab.h: gab_kmer_index_solid, gab_kmer_solid_positions)."""
import ctypes as C
import threading

import numpy as np

from ._lib import GabError, check, lib

RUN = 64        # GAB_KMER_RUN: positions per GPU lane (what last_stats()["merged"] is defined by)
MAX_K = 17      # GAB_KMER_MAX_K
MAX_PARTS = 64  # GAB_KMER_MAX_PARTS
MAX_WINDOW = 255    # GAB_KMER_MAX_WINDOW
ERANGE = -34    # GAB_ERANGE


class _Result(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("reads_kept", "positions", "distinct", "total_kmers", "hash_size", "max_count")]


class _IndexResult(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("reads_kept", "total_len", "minimizers", "distinct", "repetitive_frequency", "filtered_kmers",
                                         "filtered_entries", "selected_kmers", "index_entries")]


class _SolidResult(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("reads_kept", "total_len", "positions", "selected_positions", "candidates", "mean_total", "mean_unique",
                                         "repetitive_frequency", "filtered_kmers", "filtered_entries", "selected_kmers", "indexed_kmers", "index_entries")]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(seq, off, ln):
    """the five leading arguments of every *_device call, from torch tensors on the handle's GPU"""
    return (C.c_void_p(seq.data_ptr()), C.c_int64(seq.numel()), C.c_void_p(off.data_ptr()), C.c_void_p(ln.data_ptr()), C.c_int64(ln.numel()))


def pack_reads(reads):
    """list of bytes -> (seq uint8, off int64, len int32), reads back to back"""
    ln = np.array([len(r) for r in reads], np.int32)
    off = np.zeros(len(reads), np.int64)
    if len(reads) > 1:
        off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
    seq = np.frombuffer(b"".join(reads), np.uint8).copy() if len(reads) else np.zeros(0, np.uint8)
    return seq, off, ln


def part_of(kmers, nparts):
    """canonical k-mers (uint64 array) -> the partition of each, 0 .. nparts - 1 (int32 array); host arithmetic, no GPU"""
    kmers = np.ascontiguousarray(kmers, np.uint64)
    out = np.full(kmers.size, -12345, np.int32)
    check(lib().gab_kmer_parts_of(_p(kmers), C.c_int64(kmers.size), C.c_int(nparts), _p(out)))
    return out


def table_slots(positions, k, nparts):
    """table slots the first attempt of a partitioned count over `positions` k-mer positions allocates; no GPU"""
    fn = lib().gab_kmer_table_slots
    fn.restype = C.c_int64
    n = fn(C.c_int64(positions), C.c_int(k), C.c_int(nparts))
    if n < 0:
        check(int(n))
    return int(n)


def repetitive_frequency(minimizers, distinct, rate):
    """the filter's threshold, (size_t)(rate * ((float)minimizers / (distinct + 1))), as the library computes it; no GPU"""
    fn = lib().gab_kmer_repetitive_frequency
    fn.restype = C.c_int64
    n = fn(C.c_int64(minimizers), C.c_int64(distinct), C.c_float(rate))
    if n < 0:
        check(int(n))
    return int(n)


class KmerCounter:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().gab_kmer_create(C.c_int(device), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().gab_kmer_destroy(self._h)
            self._h = None

    __del__ = close

    def reserve(self, max_reads, max_seq_bytes):
        check(lib().gab_kmer_reserve(self._h, C.c_int64(max_reads), C.c_int64(max_seq_bytes)))

    @staticmethod
    def _dict(res):
        return {f: getattr(res, f) for f, _ in _Result._fields_}

    @staticmethod
    def _packed(reads):
        seq, off, ln = reads if isinstance(reads, tuple) else pack_reads(reads)
        return np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(ln, np.int32)

    def count(self, reads, k, min_len=5000):
        """reads: list of bytes, or a packed (seq, off, len) triple of numpy arrays -> the six result fields; only reads LONGER than
        min_len are counted"""
        return self.count_part(reads, k, 0, 1, min_len)

    def count_device(self, seq, off, ln, k, min_len=5000, stream=0):
        """torch tensors on the handle's GPU: uint8 / int64 / int32"""
        return self.count_part_device(seq, off, ln, k, 0, 1, min_len, stream)

    def reserve_part(self, max_reads, max_seq_bytes, nparts):
        check(lib().gab_kmer_reserve_part(self._h, C.c_int64(max_reads), C.c_int64(max_seq_bytes), C.c_int(nparts)))

    def count_part(self, reads, k, part, nparts, min_len=5000):
        """count() for partition `part` of `nparts` of the key space: reads_kept and positions are the whole call's, the other four
        fields the partition's, and the handle then holds the partition (spectrum, query, dump, last_stats)"""
        seq, off, ln = self._packed(reads)
        res = _Result(*([-12345] * 6))
        check(lib().gab_kmer_count_part(self._h, _p(seq), _p(off), _p(ln), C.c_int64(ln.size), C.c_int(k), C.c_int32(min_len), C.c_int(part),
                                        C.c_int(nparts), C.byref(res)))
        return self._dict(res)

    def count_part_device(self, seq, off, ln, k, part, nparts, min_len=5000, stream=0):
        """torch tensors on the handle's GPU: uint8 / int64 / int32"""
        res = _Result(*([-12345] * 6))
        check(lib().gab_kmer_count_part_device(self._h, *_dev(seq, off, ln), C.c_int(k), C.c_int32(min_len), C.c_int(part), C.c_int(nparts), C.byref(res),
                                               C.c_void_p(stream)))
        return self._dict(res)

    def _last_part(self, fn):
        part = C.c_int(-1); nparts = C.c_int(-1); slots = C.c_int64(-1); retried = C.c_int(-1)
        check(fn(self._h, C.byref(part), C.byref(nparts), C.byref(slots), C.byref(retried)))
        return {"part": part.value, "nparts": nparts.value, "table_slots": slots.value, "retried": retried.value}

    def last_part(self):
        """what the last count ran as: its partition, the slots of the table it ended in, whether its first table filled up and it ran again"""
        return self._last_part(lib().gab_kmer_last_part)

    def spectrum(self, nbins):
        hist = np.full(nbins, -12345, np.int64)
        check(lib().gab_kmer_spectrum(self._h, _p(hist), C.c_int32(nbins)))
        return hist

    def query(self, kmers):
        kmers = np.ascontiguousarray(kmers, np.uint64)
        out = np.full(kmers.size, 0xDEADBEEF, np.uint32)
        check(lib().gab_kmer_query(self._h, _p(kmers), C.c_int64(kmers.size), _p(out)))
        return out

    def dump(self, capacity=None):
        """-> (k-mers uint64 ascending, counts uint32); capacity: room offered on the first try (grown once when it is too little)"""
        n = C.c_int64(-1)
        cap = 0 if capacity is None else int(capacity)
        while True:
            kmers = np.full(cap, 0xDEADBEEFDEADBEEF, np.uint64); counts = np.full(cap, 0xDEADBEEF, np.uint32)
            rc = lib().gab_kmer_dump(self._h, _p(kmers), _p(counts), C.c_int64(cap), C.byref(n))
            if rc == -34 and n.value > cap:      # GAB_ERANGE: the needed size came back
                cap = n.value
                continue
            check(rc)
            return kmers[:n.value], counts[:n.value]

    def dump_into(self, kmers, counts):
        """one raw call: (return code, needed size)"""
        n = C.c_int64(-1)
        rc = lib().gab_kmer_dump(self._h, _p(kmers), _p(counts), C.c_int64(kmers.size), C.byref(n))
        return rc, n.value

    def last_stats(self):
        pr = C.c_int64(0); mg = C.c_int64(0); kms = C.c_float(0); tms = C.c_float(0)
        check(lib().gab_kmer_last_stats(self._h, C.byref(pr), C.byref(mg), C.byref(kms), C.byref(tms)))
        a = C.c_float(0); b = C.c_float(0); c = C.c_float(0)
        check(lib().gab_kmer_last_phases(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"probes": pr.value, "merged": mg.value, "kernel_ms": kms.value, "total_ms": tms.value,
                "pack_ms": a.value, "count_ms": b.value, "reduce_ms": c.value}

    # ---- minimizer mode -------------------------------------------------------------------------------------------------------------
    def sketch_into(self, reads, k, window, read_start, pos, min_len=5000):
        """one raw gab_kmer_sketch into the caller's arrays: (return code, needed size)"""
        seq, off, ln = self._packed(reads)
        n = C.c_int64(-1)
        rc = lib().gab_kmer_sketch(self._h, _p(seq), _p(off), _p(ln), C.c_int64(ln.size), C.c_int(k), C.c_int(window), C.c_int32(min_len), _p(read_start),
                                   _p(pos), C.c_int64(pos.size), C.byref(n))
        return rc, n.value

    def sketch(self, reads, k, window, min_len=5000, capacity=None):
        """-> (read_start int64 [n + 1], pos int32): the minimizer positions of read i are pos[read_start[i]:read_start[i + 1]], ascending;
        a filtered or too-short read has an empty range.  capacity: room offered on the first try (grown once when it is too little);
        by default twice the 2 / (window + 1) of the k-mer positions that random sequence gives, and never more than all of them"""
        packed = self._packed(reads)
        positions = int(np.maximum(packed[2].astype(np.int64) - k, 0).sum())
        cap = min(positions, 4 * positions // (max(window, 1) + 1)) + 64 if capacity is None else int(capacity)
        while True:
            start = np.full(packed[2].size + 1, -12345, np.int64); pos = np.full(cap, -12345, np.int32)
            rc, n = self.sketch_into(packed, k, window, start, pos, min_len)
            if rc == ERANGE and n > cap:
                cap = n
                continue
            check(rc)
            return start, pos[:n]

    def sketch_device(self, seq, off, ln, k, window, read_start, pos, min_len=5000, stream=0):
        """torch tensors on the handle's GPU: seq uint8, off int64, ln int32; outputs read_start int64 [n + 1] and pos int32 [capacity]
        -> (return code, needed size); ERANGE when pos is too small (nothing written)"""
        n = C.c_int64(-1)
        rc = lib().gab_kmer_sketch_device(self._h, *_dev(seq, off, ln), C.c_int(k), C.c_int(window), C.c_int32(min_len), C.c_void_p(read_start.data_ptr()),
                                          C.c_void_p(pos.data_ptr()), C.c_int64(pos.numel()), C.byref(n), C.c_void_p(stream))
        if rc != ERANGE:
            check(rc)
        return rc, n.value

    @staticmethod
    def _index_dict(res):
        return {f: getattr(res, f) for f, _ in _IndexResult._fields_}

    def index_minimizers(self, reads, k, window, rate=100.0, min_len=5000):
        """builds the minimizer index into the handle (it replaces the count table) -> the nine fields of gab_kmer_index_result"""
        seq, off, ln = self._packed(reads)
        res = _IndexResult(*([-12345] * 9))
        check(lib().gab_kmer_index_minimizers(self._h, _p(seq), _p(off), _p(ln), C.c_int64(ln.size), C.c_int(k), C.c_int(window), C.c_int32(min_len),
                                              C.c_float(rate), C.byref(res)))
        return self._index_dict(res)

    def index_minimizers_device(self, seq, off, ln, k, window, rate=100.0, min_len=5000, stream=0):
        """torch tensors on the handle's GPU: uint8 / int64 / int32"""
        res = _IndexResult(*([-12345] * 9))
        check(lib().gab_kmer_index_minimizers_device(self._h, *_dev(seq, off, ln), C.c_int(k), C.c_int(window), C.c_int32(min_len), C.c_float(rate),
                                                     C.byref(res), C.c_void_p(stream)))
        return self._index_dict(res)

    def index_part_begin(self, reads, k, window, part, nparts, min_len=5000):
        """phase 1 of partition `part` of `nparts` of the minimizer index: sketches all reads, counts the capacities of the k-mers the
        partition owns -> the nine fields, of which reads_kept and total_len are the whole call's, minimizers and distinct the
        partition's own and the rest 0.  The handle is then pending until index_part_finish"""
        seq, off, ln = self._packed(reads)
        res = _IndexResult(*([-12345] * 9))
        check(lib().gab_kmer_index_part_begin(self._h, _p(seq), _p(off), _p(ln), C.c_int64(ln.size), C.c_int(k), C.c_int(window), C.c_int32(min_len),
                                              C.c_int(part), C.c_int(nparts), C.byref(res)))
        return self._index_dict(res)

    def index_part_begin_device(self, seq, off, ln, k, window, part, nparts, min_len=5000, stream=0):
        """torch tensors on the handle's GPU: uint8 / int64 / int32; `ln` must stay alive and unchanged until index_part_finish"""
        res = _IndexResult(*([-12345] * 9))
        check(lib().gab_kmer_index_part_begin_device(self._h, *_dev(seq, off, ln), C.c_int(k), C.c_int(window), C.c_int32(min_len), C.c_int(part),
                                                     C.c_int(nparts), C.byref(res), C.c_void_p(stream)))
        return self._index_dict(res)

    def index_part_finish(self, minimizers, distinct, rate=100.0):
        """phase 2: minimizers / distinct are the sums of phase 1 over ALL partitions -> the nine fields: repetitive_frequency is the
        global threshold, every other count the partition's own.  The handle then holds the partition's index (index_dump,
        index_lookup, index_last_phases, index_last_part)"""
        res = _IndexResult(*([-12345] * 9))
        check(lib().gab_kmer_index_part_finish(self._h, C.c_int64(minimizers), C.c_int64(distinct), C.c_float(rate), C.byref(res)))
        return self._index_dict(res)

    def index_last_part(self):
        """what the last index build ran as: its partition, the slots of the capacity table it ended in, whether the first one filled up"""
        return self._last_part(lib().gab_kmer_index_last_part)

    def index_dump_into(self, kmers, start, gpos):
        """one raw gab_kmer_index_dump: (return code, needed k-mers, needed entries); start needs kmers.size + 1 of room"""
        nk = C.c_int64(-1); ne = C.c_int64(-1)
        assert start.size >= kmers.size + 1
        rc = lib().gab_kmer_index_dump(self._h, _p(kmers), _p(start), _p(gpos), C.c_int64(kmers.size), C.c_int64(gpos.size), C.byref(nk), C.byref(ne))
        return rc, nk.value, ne.value

    def index_dump(self):
        """-> (k-mers uint64 ascending, start int64 [nk + 1], gpos int64): the list of kmers[i] is gpos[start[i]:start[i + 1]], ascending"""
        nk, ne = 0, 0
        while True:
            kmers = np.full(nk, 0xDEADBEEFDEADBEEF, np.uint64); start = np.full(nk + 1, -12345, np.int64); gpos = np.full(ne, -12345, np.int64)
            rc, need_k, need_e = self.index_dump_into(kmers, start, gpos)
            if rc == ERANGE and (need_k > nk or need_e > ne):
                nk, ne = need_k, need_e
                continue
            check(rc)
            return kmers[:need_k], start[:need_k + 1], gpos[:need_e]

    def index_lookup(self, kmers):
        """-> (first int64, count int32, repetitive uint8) per k-mer (canonicalised first): its list is index_dump()'s
        gpos[first:first + count]; absent: count 0, first -1; removed as repetitive: count 0, first -1, repetitive 1"""
        kmers = np.ascontiguousarray(kmers, np.uint64)
        first = np.full(kmers.size, -12345, np.int64); count = np.full(kmers.size, -12345, np.int32); rep = np.full(kmers.size, 77, np.uint8)
        check(lib().gab_kmer_index_lookup(self._h, _p(kmers), C.c_int64(kmers.size), _p(first), _p(count), _p(rep)))
        return first, count, rep

    def index_last_phases(self):
        a = C.c_float(0); b = C.c_float(0); c = C.c_float(0); d = C.c_float(0)
        check(lib().gab_kmer_index_last_phases(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"sketch_ms": a.value, "count_ms": b.value, "fill_ms": c.value, "sort_ms": d.value}

    # ---- solid k-mer index ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _solid_dict(res):
        return {f: getattr(res, f) for f, _ in _SolidResult._fields_}

    @staticmethod
    def _solid_rule(k, min_len, min_freq, select_rate, tandem_freq):
        return C.c_int(k), C.c_int32(min_len), C.c_int(min_freq), C.c_float(select_rate), C.c_int(tandem_freq)

    def index_solid(self, reads, k, min_freq=2, select_rate=0.4, tandem_freq=100, rate=100.0, min_len=5000):
        """counts, then builds the solid k-mer index into the handle (it replaces a count or an index there) -> the thirteen fields of
        gab_kmer_solid_result; index_dump / index_lookup then read it"""
        seq, off, ln = self._packed(reads)
        res = _SolidResult(*([-12345] * 13))
        check(lib().gab_kmer_index_solid(self._h, _p(seq), _p(off), _p(ln), C.c_int64(ln.size), *self._solid_rule(k, min_len, min_freq, select_rate, tandem_freq),
                                         C.c_float(rate), C.byref(res)))
        return self._solid_dict(res)

    def index_solid_device(self, seq, off, ln, k, min_freq=2, select_rate=0.4, tandem_freq=100, rate=100.0, min_len=5000, stream=0):
        """torch tensors on the handle's GPU: uint8 / int64 / int32"""
        res = _SolidResult(*([-12345] * 13))
        check(lib().gab_kmer_index_solid_device(self._h, *_dev(seq, off, ln), *self._solid_rule(k, min_len, min_freq, select_rate, tandem_freq), C.c_float(rate),
                                                C.byref(res), C.c_void_p(stream)))
        return self._solid_dict(res)

    def solid_positions_into(self, reads, k, read_start, pos, min_freq=2, select_rate=0.4, tandem_freq=100, min_len=5000):
        """one raw gab_kmer_solid_positions into the caller's arrays: (return code, needed size)"""
        seq, off, ln = self._packed(reads)
        n = C.c_int64(-1)
        rc = lib().gab_kmer_solid_positions(self._h, _p(seq), _p(off), _p(ln), C.c_int64(ln.size), *self._solid_rule(k, min_len, min_freq, select_rate, tandem_freq),
                                            _p(read_start), _p(pos), C.c_int64(pos.size), C.byref(n))
        return rc, n.value

    def solid_positions(self, reads, k, min_freq=2, select_rate=0.4, tandem_freq=100, min_len=5000, capacity=None):
        """-> (read_start int64 [n + 1], pos int32): the selected positions of read i are pos[read_start[i]:read_start[i + 1]], ascending.
        capacity: room offered on the first try (grown once when it is too little); by default the select_rate share of the positions"""
        packed = self._packed(reads)
        positions = int(np.maximum(packed[2].astype(np.int64) - k, 0).sum())
        cap = int(positions * min(1.0, select_rate + 0.1)) + 64 if capacity is None else int(capacity)
        while True:
            start = np.full(packed[2].size + 1, -12345, np.int64); pos = np.full(cap, -12345, np.int32)
            rc, n = self.solid_positions_into(packed, k, start, pos, min_freq, select_rate, tandem_freq, min_len)
            if rc == ERANGE and n > cap:
                cap = n
                continue
            check(rc)
            return start, pos[:n]

    def solid_positions_device(self, seq, off, ln, k, read_start, pos, min_freq=2, select_rate=0.4, tandem_freq=100, min_len=5000, stream=0):
        """torch tensors on the handle's GPU; outputs read_start int64 [n + 1] and pos int32 [capacity] -> (return code, needed size)"""
        n = C.c_int64(-1)
        rc = lib().gab_kmer_solid_positions_device(self._h, *_dev(seq, off, ln), *self._solid_rule(k, min_len, min_freq, select_rate, tandem_freq),
                                                   C.c_void_p(read_start.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_int64(pos.numel()), C.byref(n),
                                                   C.c_void_p(stream))
        if rc != ERANGE:
            check(rc)
        return rc, n.value

    def solid_last_phases(self):
        v = [C.c_float(0) for _ in range(5)]
        check(lib().gab_kmer_solid_last_phases(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("count_ms", "select_ms", "capacity_ms", "fill_ms", "sort_ms"), (x.value for x in v)))

    def solid_last_stats(self):
        """tested_positions: positions that took the multiplicity test; fallback_reads: reads whose test outgrew the on-chip table"""
        a = C.c_int64(-1); b = C.c_int64(-1)
        check(lib().gab_kmer_solid_last_stats(self._h, C.byref(a), C.byref(b)))
        return {"tested_positions": a.value, "fallback_reads": b.value}


class KmerCounterSet:
    """One count over several GPUs without a merge: handle i, on devices[i], counts partition i of len(devices) of the key space.
    Every handle walks all reads; no handle needs anything from another.  A device may appear more than once (several partitions on
    one card, one after the other or side by side).  index_minimizers builds the minimizer index the same way, in two rounds around
    the sum of the partitions' minimizers and distinct k-mers."""

    def __init__(self, devices):
        devices = list(devices)
        if not 1 <= len(devices) <= MAX_PARTS:
            raise ValueError(f"KmerCounterSet: {len(devices)} devices, supported 1..{MAX_PARTS}")
        self.parts = []
        try:
            for d in devices:
                self.parts.append(KmerCounter(d))
        except Exception:
            self.close()
            raise

    def close(self):
        for kc in self.parts:
            kc.close()
        self.parts = []

    def reserve(self, max_reads, max_seq_bytes):
        for kc in self.parts:
            kc.reserve_part(max_reads, max_seq_bytes, len(self.parts))

    def count(self, reads, k, min_len=5000):
        """every partition at once, one host thread per handle -> the six fields of the whole input"""
        packed = KmerCounter._packed(reads)
        n = len(self.parts)
        out = self._each(lambda i: self.parts[i].count_part(packed, k, i, n, min_len))
        both = {f: out[0][f] for f in ("reads_kept", "positions")}
        both.update({f: sum(r[f] for r in out) for f in ("distinct", "total_kmers", "hash_size")})
        both["max_count"] = max(r["max_count"] for r in out)
        return both

    def spectrum(self, nbins):
        return sum(kc.spectrum(nbins) for kc in self.parts)

    def query(self, kmers):
        """a k-mer is counted by one partition and 0 in every other: the sum is its count"""
        kmers = np.ascontiguousarray(kmers, np.uint64)
        out = np.zeros(kmers.size, np.uint32)
        for kc in self.parts:
            out += kc.query(kmers)
        return out

    def dump(self):
        """-> (k-mers uint64 ascending, counts uint32): the partitions' sorted lists, merged"""
        lists = [kc.dump() for kc in self.parts]
        kmers = np.concatenate([d[0] for d in lists]); counts = np.concatenate([d[1] for d in lists])
        order = np.argsort(kmers, kind="stable")      # (the lists are disjoint and sorted: a merge, done by numpy's run-aware sort)
        return kmers[order], counts[order]

    def last_stats(self):
        """one row per partition: last_stats() and last_part() of its handle"""
        return [dict(kc.last_stats(), **kc.last_part()) for kc in self.parts]

    def _each(self, call):
        """call(i) for every handle at once, one host thread per handle -> the list of results; the first exception is raised here"""
        n = len(self.parts)
        out = [None] * n

        def run(i):
            try:
                out[i] = call(i)
            except Exception as e:      # (handed to the caller's thread below)
                out[i] = e
        threads = [threading.Thread(target=run, args=(i,)) for i in range(1, n)]
        for t in threads:
            t.start()
        run(0)
        for t in threads:
            t.join()
        for r in out:
            if isinstance(r, Exception):
                raise r
        return out

    # ---- minimizer mode: the index in key-space partitions, built in two phases ------------------------------------------------------
    def index_minimizers(self, reads, k, window, rate=100.0, min_len=5000):
        """two rounds of one host thread per handle: every partition sketches all reads and counts its own capacities; the sums of
        their minimizers and distinct k-mers give the one threshold every partition then filters with -> the nine fields of the whole
        input"""
        packed = KmerCounter._packed(reads)
        n = len(self.parts)
        begun = self._each(lambda i: self.parts[i].index_part_begin(packed, k, window, i, n, min_len))
        minimizers = sum(r["minimizers"] for r in begun); distinct = sum(r["distinct"] for r in begun)
        out = self._each(lambda i: self.parts[i].index_part_finish(minimizers, distinct, rate))
        both = {f: out[0][f] for f in ("reads_kept", "total_len", "repetitive_frequency")}
        both.update({f: sum(r[f] for r in out) for f in ("minimizers", "distinct", "filtered_kmers", "filtered_entries", "selected_kmers", "index_entries")})
        return {f: both[f] for f, _ in _IndexResult._fields_}

    def index_dump(self):
        """-> (k-mers uint64 ascending, start int64 [nk + 1], gpos int64): the partitions' dumps merged by k-mer, start recomputed"""
        dumps = [kc.index_dump() for kc in self.parts]
        kmers = np.concatenate([d[0] for d in dumps])
        lens = np.concatenate([np.diff(d[1]) for d in dumps])
        base = np.cumsum([0] + [d[2].size for d in dumps])[:-1]
        first = np.concatenate([d[1][:-1] + b for d, b in zip(dumps, base)])      # where every list starts in the concatenated gpos
        gpos = np.concatenate([d[2] for d in dumps])
        order = np.argsort(kmers, kind="stable")      # (disjoint sorted lists: a merge)
        kmers, lens, first = kmers[order], lens[order], first[order]
        start = np.zeros(kmers.size + 1, np.int64)
        start[1:] = np.cumsum(lens)
        take = np.repeat(first - start[:-1], lens) + np.arange(int(start[-1]), dtype=np.int64)
        return kmers, start, gpos[take]

    def index_lookup(self, kmers):
        """-> (first, count, repetitive) as KmerCounter.index_lookup: count and repetitive come from the partition that owns the k-mer,
        first is the start of its list in index_dump()'s merged gpos"""
        kmers = np.ascontiguousarray(kmers, np.uint64)
        first = np.full(kmers.size, -1, np.int64); count = np.zeros(kmers.size, np.int32); rep = np.zeros(kmers.size, np.uint8)
        keys = []
        for kc in self.parts:
            f, c, r = kc.index_lookup(kmers)      # (another partition's k-mer: -1, 0, 0)
            count += c; rep |= r
            hit = np.flatnonzero(f >= 0)
            if hit.size:      # (the canonical k-mer of every hit: list starts are strictly ascending, a kept k-mer has an entry)
                own_kmers, own_start, _ = kc.index_dump()
                keys.append((hit, own_kmers[np.searchsorted(own_start, f[hit])]))
        if keys:
            merged, start, _ = self.index_dump()
            for hit, canon in keys:
                first[hit] = start[np.searchsorted(merged, canon)]
        return first, count, rep

    def index_last_phases(self):
        """one row per partition: index_last_phases() and index_last_part() of its handle"""
        return [dict(kc.index_last_phases(), **kc.index_last_part()) for kc in self.parts]


__all__ = ["KmerCounter", "KmerCounterSet", "GabError", "pack_reads", "part_of", "table_slots", "repetitive_frequency", "RUN", "MAX_K", "MAX_PARTS", "MAX_WINDOW"]
