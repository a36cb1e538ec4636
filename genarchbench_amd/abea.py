"""Host-side mirror of the adaptive banded event alignment, align() (abea/src/align.c:169-548), over the C ABI
(include/gab.h: gab_abea_align, gab_abea_align_device): the loop of align_db over its reads (abea/src/f5c.c:1367-1394) as one call."""
import ctypes as C

import numpy as np

from ._lib import check, lib

K = 6             # GAB_ABEA_K
BANDWIDTH = 100   # GAB_ABEA_BANDWIDTH
NKMER = 4096      # GAB_ABEA_NKMER
LOW_EMISSION, NOT_SPANNED, GAP, NO_END = 1, 2, 4, 8      # gab_abea_read.flags

PAIR = np.dtype([("ref_pos", np.int32), ("read_pos", np.int32)])
READ = np.dtype([("n_pairs", np.int32), ("path_len", np.int32), ("end_event", np.int32), ("max_gap", np.int32), ("flags", np.uint32),
                 ("pad", np.int32), ("avg_log_emission", np.float64), ("fills", np.int64)])      # gab_abea_read, 40 bytes
assert PAIR.itemsize == 8 and READ.itemsize == 40


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_reads(reads):
    """list of (bases bytes, event means, scale, shift) -> the packed arrays of align(): seq, seq_off, seq_len, events, event_off,
    n_events, scale, shift, pair_off (n_events + n_kmers pairs of room per read, back to back)"""
    seq_len = np.array([len(r[0]) for r in reads], np.int32)
    n_events = np.array([len(r[1]) for r in reads], np.int32)
    seq_off = np.zeros(len(reads), np.int64); event_off = np.zeros(len(reads), np.int64); pair_off = np.zeros(len(reads), np.int64)
    if len(reads) > 1:
        seq_off[1:] = np.cumsum(seq_len[:-1], dtype=np.int64)
        event_off[1:] = np.cumsum(n_events[:-1], dtype=np.int64)
        pair_off[1:] = np.cumsum((n_events.astype(np.int64) + seq_len - K + 1)[:-1])
    seq = np.frombuffer(b"".join(bytes(r[0]) for r in reads), np.uint8).copy() if reads else np.zeros(0, np.uint8)
    events = np.concatenate([np.asarray(r[1], np.float32) for r in reads]) if reads else np.zeros(0, np.float32)
    scale = np.array([r[2] for r in reads], np.float32); shift = np.array([r[3] for r in reads], np.float32)
    return seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pair_off


def pair_room(seq_len, n_events):
    """pairs of room a read needs at its pair_off: n_events + n_kmers"""
    return np.asarray(n_events, np.int64) + np.asarray(seq_len, np.int64) - K + 1


class EventAligner:
    """one pore model (4096 k-mer entries: level_mean, level_stdv, optionally level_log_stdv) on one GPU"""

    def __init__(self, level_mean, level_stdv, level_log_stdv=None, device=0):
        self._h = C.c_void_p()
        mean = np.ascontiguousarray(level_mean, np.float32); stdv = np.ascontiguousarray(level_stdv, np.float32)
        if mean.size != NKMER or stdv.size != NKMER or (level_log_stdv is not None and np.size(level_log_stdv) != NKMER):
            raise ValueError(f"the pore model has {NKMER} entries")
        lstd = None if level_log_stdv is None else np.ascontiguousarray(level_log_stdv, np.float32)
        check(lib().gab_abea_create(C.c_int(device), _p(mean), _p(stdv), _p(lstd) if lstd is not None else None, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().gab_abea_destroy(self._h)
            self._h = None

    __del__ = close

    def reserve(self, max_reads, max_bases, max_events):
        check(lib().gab_abea_reserve(self._h, C.c_int64(max_reads), C.c_int64(max_bases), C.c_int64(max_events)))

    def align(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pair_off=None):
        """numpy arrays (pack_reads gives them) -> (pairs, pair_off, records): pairs a PAIR array in which read i's path is
        pairs[pair_off[i] : pair_off[i] + records[i]["path_len"]], records a READ array"""
        seq = np.ascontiguousarray(seq, np.uint8); events = np.ascontiguousarray(events, np.float32)
        seq_off = np.ascontiguousarray(seq_off, np.int64); event_off = np.ascontiguousarray(event_off, np.int64)
        seq_len = np.ascontiguousarray(seq_len, np.int32); n_events = np.ascontiguousarray(n_events, np.int32)
        scale = np.ascontiguousarray(scale, np.float32); shift = np.ascontiguousarray(shift, np.float32)
        n = seq_len.size
        room = pair_room(seq_len, n_events)
        if pair_off is None:
            pair_off = np.zeros(n, np.int64)
            if n > 1:
                pair_off[1:] = np.cumsum(room[:-1])
        pair_off = np.ascontiguousarray(pair_off, np.int64)
        total = int((pair_off + np.maximum(room, 0)).max()) if n else 0
        pairs = np.full(max(total, 0), -1, np.int32).repeat(2).view(PAIR)
        res = np.zeros(n, READ)
        check(lib().gab_abea_align(self._h, _p(seq), _p(seq_off), _p(seq_len), _p(events), _p(event_off), _p(n_events), _p(scale), _p(shift),
                                   C.c_int64(n), _p(pairs), _p(pair_off), _p(res)))
        return pairs, pair_off, res

    def align_reads(self, reads):
        """list of (bases, event means, scale, shift) -> (pairs, pair_off, records)"""
        return self.align(*pack_reads(reads))

    def align_device(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, res, stream=0):
        """torch tensors on the handle's GPU: uint8, int64, int32, float32, int64, int32, float32, float32; pairs an int32 tensor of
        shape (room, 2) and res a uint8 tensor of 40 bytes per read, both filled in place (complete when the call returns)"""
        n = seq_len.numel()
        if pairs.numel() % 2 or res.numel() * res.element_size() < n * READ.itemsize:
            raise ValueError("pairs holds (ref_pos, read_pos) int32 pairs, res 40 bytes per read")
        check(lib().gab_abea_align_device(
            self._h, C.c_void_p(seq.data_ptr()), C.c_int64(seq.numel()), C.c_void_p(seq_off.data_ptr()), C.c_void_p(seq_len.data_ptr()),
            C.c_void_p(events.data_ptr()), C.c_int64(events.numel()), C.c_void_p(event_off.data_ptr()), C.c_void_p(n_events.data_ptr()),
            C.c_void_p(scale.data_ptr()), C.c_void_p(shift.data_ptr()), C.c_int64(n), C.c_void_p(pairs.data_ptr()), C.c_int64(pairs.numel() // 2),
            C.c_void_p(pair_off.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(stream)))

    def last_stats(self):
        """cells filled, bands swept, launches, and the device time of the DP kernels and of all kernels (ms) of the last call"""
        cells = C.c_int64(-1); bands = C.c_int64(-1); launches = C.c_int64(-1); kms = C.c_float(-1); tms = C.c_float(-1)
        check(lib().gab_abea_last_stats(self._h, C.byref(cells), C.byref(bands), C.byref(launches), C.byref(kms), C.byref(tms)))
        return {"cells": cells.value, "bands": bands.value, "launches": launches.value, "kernel_ms": kms.value, "total_ms": tms.value}
