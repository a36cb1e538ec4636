"""Host-side mirror of the dbg section of include/gab.h: the de Bruijn graphs of Platypus' local assembly, one per assembly region
(dbg/src/debruijn.cpp: loadReferenceIntoGraph :1291-1317, loadBAMDataIntoGraph :1399-1414), and the region planner (the batch loop
of main, :1576-1592, with setWindowPointers, dbg/src/common.cpp:161-194)."""
import ctypes as C

import numpy as np

from ._lib import GabError, check, lib

MAX_K = 16                      # GAB_DBG_MAX_K
MAX_OCCURRENCES = 1 << 24       # GAB_DBG_MAX_OCCURRENCES
REGION_SIZE = 1500              # GAB_DBG_REGION_SIZE
ERANGE = -34                    # GAB_ERANGE
NODE = np.dtype([("src_read", "<i4"), ("src_off", "<i4"), ("colours", "<i4"), ("position", "<i4"), ("weight", "<i8"), ("n_edges", "<i4"),
                 ("edge_to", "<i4", 4), ("pad", "<i4"), ("edge_weight", "<i8", 4)])                  # gab_dbg_node
REGION = np.dtype([("start", "<i4"), ("ref_start", "<i4"), ("ref_len", "<i4"), ("pad", "<i4"), ("read_begin", "<i8"), ("read_end", "<i8")])    # gab_dbg_region
INPUTS = ("ref", "ref_off", "ref_len", "ref_start", "seq", "qual", "read_off", "read_len", "read_flag", "read_begin", "read_end")
_DTYPES = dict(ref=np.uint8, ref_off=np.int64, ref_len=np.int32, ref_start=np.int32, seq=np.uint8, qual=np.uint8, read_off=np.int64, read_len=np.int32,
               read_flag=np.int32, read_begin=np.int64, read_end=np.int64)


class _Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("min_qual", C.c_int32)]


class _Stats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("regions", "occurrences", "passed", "nodes", "edges", "probes")] + [("kernel_ms", C.c_float), ("total_ms", C.c_float)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_regions(regions, reads):
    """regions: [(ref bytes, ref_start, read_begin, read_end)], reads: [(seq bytes, qual bytes, flag)] -> the dict of arrays that build() takes:
    the reference slices and the reads back to back"""
    def slab(parts):
        ln = np.array([len(x) for x in parts], np.int32)
        off = np.zeros(len(parts), np.int64)
        if len(parts) > 1:
            off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
        return (np.frombuffer(b"".join(parts), np.uint8).copy() if len(parts) else np.zeros(0, np.uint8)), off, ln
    ref, ref_off, ref_len = slab([bytes(r[0]) for r in regions])
    seq, read_off, read_len = slab([bytes(r[0]) for r in reads])
    qual, _, qlen = slab([bytes(r[1]) for r in reads])
    assert np.array_equal(qlen, read_len), "a read has as many qualities as bases"
    return dict(ref=ref, ref_off=ref_off, ref_len=ref_len, ref_start=np.array([r[1] for r in regions], np.int32), seq=seq, qual=qual, read_off=read_off,
                read_len=read_len, read_flag=np.array([r[2] for r in reads], np.int32), read_begin=np.array([r[2] for r in regions], np.int64),
                read_end=np.array([r[3] for r in regions], np.int64))


def room(packed, k=15, per_region=False):
    """the nodes the regions can have at most, from lengths alone; no GPU"""
    a = {f: np.ascontiguousarray(packed[f], _DTYPES[f]) for f in ("ref_len", "read_len", "read_flag", "read_begin", "read_end")}
    each = np.zeros(a["ref_len"].size, np.int64)
    n = lib().gab_dbg_room(_p(a["ref_len"]), _p(a["read_len"]), _p(a["read_flag"]), _p(a["read_begin"]), _p(a["read_end"]), a["read_len"].size, a["ref_len"].size, k, _p(each))
    if n < 0:
        check(int(n))
    return (int(n), each) if per_region else int(n)


def plan_regions(beg, end, pos, read_end, contig_len):
    """the reference's assembly regions of [beg, end): a REGION array (start, ref_start, ref_len, read_begin, read_end); no GPU"""
    pos = np.ascontiguousarray(pos, np.int32); read_end = np.ascontiguousarray(read_end, np.int32)
    need = C.c_int64(0)
    rc = lib().gab_dbg_plan_regions(beg, end, _p(pos), _p(read_end), pos.size, contig_len, None, 0, C.byref(need))
    if rc not in (0, ERANGE):
        check(rc)
    out = np.zeros(need.value, REGION)
    check(lib().gab_dbg_plan_regions(beg, end, _p(pos), _p(read_end), pos.size, contig_len, _p(out), out.size, C.byref(need)))
    return out


def format_region(ref, ref_start, reads, records):
    """the reference's verbose line of one region (dbg/src/debruijn.cpp:1458-1465) from its records: "%d %d " of ref_start twice, then per
    node the rest of the region's reference or of the read from the node's first occurrence on.  reads: the call's [(seq, ...)] or [seq]"""
    parts = [b"%d %d " % (ref_start, ref_start)]
    for rec in records:
        r = int(rec["src_read"])
        src = ref if r < 0 else (reads[r] if isinstance(reads[r], (bytes, bytearray)) else reads[r][0])
        parts.append(bytes(src[int(rec["src_off"]):]))
    return b"".join(parts) + b"\n"


class GraphBuilder:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().gab_dbg_create(device, C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            lib().gab_dbg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, max_regions, max_reads, max_occurrences):
        check(lib().gab_dbg_reserve(self._h, max_regions, max_reads, max_occurrences))

    def build(self, packed, k=15, min_qual=20, capacity=None):
        """packed: pack_regions()'s dict (host arrays) -> (node_off int64[n_regions + 1], records NODE[nodes]).  capacity None: the library is
        asked for the need first (one extra call) -- pass room(packed, k) to do it in one"""
        a = {f: np.ascontiguousarray(packed[f], _DTYPES[f]) for f in INPUTS}
        nr, nd = a["ref_len"].size, a["read_len"].size
        params = _Params(k, min_qual)
        node_off = np.zeros(nr + 1, np.int64)
        nout = C.c_int64(0)

        def call(nodes):
            return lib().gab_dbg_build(self._h, C.byref(params), _p(a["ref"]), _p(a["ref_off"]), _p(a["ref_len"]), _p(a["ref_start"]), _p(a["seq"]), _p(a["qual"]),
                                       _p(a["read_off"]), _p(a["read_len"]), _p(a["read_flag"]), nd, _p(a["read_begin"]), _p(a["read_end"]), nr, _p(node_off),
                                       _p(nodes), nodes.size, C.byref(nout))
        nodes = np.zeros(0 if capacity is None else capacity, NODE)
        rc = call(nodes)
        if rc == ERANGE and capacity is None:
            nodes = np.zeros(nout.value, NODE)
            rc = call(nodes)
        self.needed = nout.value
        check(rc)
        return node_off, nodes[:nout.value]

    def build_device(self, inputs, node_off, nodes, k=15, min_qual=20, stream=0):
        """inputs: {name: torch tensor on the handle's GPU} for the names of INPUTS; node_off (int64, n_regions + 1) and nodes (uint8, 80 bytes a
        record, or any tensor of that many bytes) are torch tensors the records are written into -> the number of nodes"""
        t = inputs
        nr, nd = t["ref_len"].numel(), t["read_len"].numel()
        params = _Params(k, min_qual)
        nout = C.c_int64(0)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        capacity = nodes.numel() * nodes.element_size() // NODE.itemsize
        rc = lib().gab_dbg_build_device(self._h, C.byref(params), ptr(t["ref"]), t["ref"].numel(), ptr(t["ref_off"]), ptr(t["ref_len"]), ptr(t["ref_start"]), ptr(t["seq"]),
                                        ptr(t["qual"]), t["seq"].numel(), ptr(t["read_off"]), ptr(t["read_len"]), ptr(t["read_flag"]), nd, ptr(t["read_begin"]),
                                        ptr(t["read_end"]), nr, ptr(node_off), ptr(nodes), capacity, C.byref(nout), C.c_void_p(stream))
        self.needed = nout.value
        check(rc)
        return nout.value

    def last_stats(self):
        s = _Stats()
        check(lib().gab_dbg_last_stats(self._h, C.byref(s)))
        out = {f: getattr(s, f) for f, _ in _Stats._fields_}
        ph = [C.c_float(0) for _ in range(3)]
        check(lib().gab_dbg_last_phases(self._h, *[C.byref(x) for x in ph]))
        out.update(insert_ms=ph[0].value, number_ms=ph[1].value, emit_ms=ph[2].value)
        return out


__all__ = ["GraphBuilder", "GabError", "NODE", "REGION", "pack_regions", "plan_regions", "format_region", "room"]
