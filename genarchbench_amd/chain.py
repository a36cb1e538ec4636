"""Host-side mirror of host_chain_kernel (chain/src/host_kernel.h:6, fast-chain/src/host_kernel.h:6)."""
import ctypes as C

import numpy as np

from ._lib import check, lib

CHAIN, FASTCHAIN = 0, 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_pair(host):
    hs, hp = host
    for a in (hs, hp):
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous and a.flags.writeable):
            raise TypeError("host=(score, parent): writable C-contiguous int32 numpy arrays")
    return hs, hp


def _lock(arrays):
    """page-lock every array (gab_host_register) -- a view's whole base array, each base once -> what to hand to _unlock"""
    locked = []
    for a in arrays:
        while isinstance(a.base, np.ndarray):
            a = a.base
        if a.nbytes and a.ctypes.data not in locked:
            check(lib().gab_host_register(C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)))
            locked.append(a.ctypes.data)
    return locked


def _unlock(locked):
    for addr in locked:
        lib().gab_host_unregister(C.c_void_p(addr))


class ChainEngine:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().gab_chain_create(C.c_int(device), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().gab_chain_destroy(self._h)
            self._h = None

    __del__ = close

    def host_chain_kernel(self, batch, mode=CHAIN, pinned=False, host=None):
        """batch: tools.gabgen.ChainBatch-like (hdr records, call_off, x, y) -> (scores, parents).
        pinned: page-lock the four arrays for the call, as the drivers do with their slabs (gab_host_register);
        host: the caller's own (score, parent) int32 arrays to fill, of the arrays' extent (the largest call_off + n); views are
        page-locked with their whole base array"""
        if host is None:
            score = np.full(batch.nanchors, -777, np.int32); parent = np.full(batch.nanchors, -777, np.int32)
        else:
            score, parent = _host_pair(host)
        locked = _lock((batch.x, batch.y, score, parent)) if pinned else []
        try:
            check(lib().gab_chain_run(self._h, C.c_int(mode), _p(batch.x), _p(batch.y), _p(batch.call_off),
                                      _p(batch.hdr), C.c_int64(batch.ncalls), _p(score), _p(parent)))
        finally:
            _unlock(locked)
        return score, parent

    def run_device(self, mode, x, y, call_off, hdr, score, parent, stream=0):
        """x, y, score, parent: torch CUDA tensors; call_off, hdr: numpy (host) call table"""
        check(lib().gab_chain_run_device(self._h, C.c_int(mode), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                         _p(call_off), _p(hdr), C.c_int64(len(hdr)),
                                         C.c_void_p(score.data_ptr()), C.c_void_p(parent.data_ptr()),
                                         C.c_void_p(stream)))

    def run_device_through(self, mode, x, y, call_off, hdr, score, parent, pinned=True, stream=0, host=None):
        """run_device + the results in host arrays as well (gab_chain_run_device_through): returns (score, parent) numpy arrays;
        pinned: page-lock them for the call, so that the DP kernel writes them through while it runs;
        host: the caller's own (score, parent) int32 arrays instead of fresh ones; views (a window with canaries on both sides) are
        page-locked with their whole base array"""
        if host is None:
            n = int(score.numel())
            hs = np.full(n, -777, np.int32); hp = np.full(n, -777, np.int32)
        else:
            hs, hp = _host_pair(host)
        locked = _lock((hs, hp)) if pinned else []
        try:
            check(lib().gab_chain_run_device_through(self._h, C.c_int(mode), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                                     _p(call_off), _p(hdr), C.c_int64(len(hdr)), C.c_void_p(score.data_ptr()),
                                                     C.c_void_p(parent.data_ptr()), _p(hs), _p(hp), C.c_void_p(stream)))
        finally:
            _unlock(locked)
        return hs, hp

    def last_stats(self):
        ev = C.c_int64(0); ms = C.c_float(0)
        check(lib().gab_chain_last_stats(self._h, C.byref(ev), C.byref(ms)))
        return {"evals": ev.value, "kernel_ms": ms.value}

    def last_through(self):
        """how the host arrays of the last run_device / run_device_through call were filled (gab_chain_last_through): 0 not asked for,
        1 written through by the kernels, 2 copied at the end: not page-locked, 3 copied at the end: a launch that does not write through
        took part, 4 written through and copied after all: the table form handed a call back"""
        route = C.c_int(-1)
        check(lib().gab_chain_last_through(self._h, C.byref(route)))
        return route.value

    def last_split(self, ncalls):
        """which kernel form took each call of the last run_device / run_device_through call (gab_chain_last_split; host_chain_kernel too
        below its big-batch paths): (form, counters) -- form[c] 0 empty, 1 throughput, 2 latency, 3 table, 4 table: not eligible,
        5 table: handed back, 6 legacy-only launch; counters {no_room, rescans, helpers, groups_needed}"""
        form = np.full(ncalls, 255, np.uint8); ct = (C.c_int64 * 4)()
        check(lib().gab_chain_last_split(self._h, C.c_int64(ncalls), _p(form), ct))
        return form, dict(zip(("no_room", "rescans", "helpers", "groups_needed"), (int(v) for v in ct)))
