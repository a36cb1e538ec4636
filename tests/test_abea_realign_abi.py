"""The C ABI of gab_abea_realign without a GPU: the symbols, the trace shape, and no quiet fall-back."""
import ctypes as C

import genarchbench_amd as g

import abea_realign_model as M

SYMBOLS = ("gab_abea_realign", "gab_abea_realign_device", "gab_abea_realign_last_stats", "gab_abea_realign_stage_ms", "gab_abea_realign_shape")


def test_the_symbols_are_exported():
    lib = g.lib()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_the_shape_needs_no_gpu_and_is_the_models():
    from genarchbench_amd import abea
    rows = C.c_int32(0)
    assert g.lib().gab_abea_realign_shape(C.byref(rows)) == 0 and rows.value == M.ROWS == abea.realign_shape()
    assert g.lib().gab_abea_realign_shape(None) == 0
    assert abea.EALN.itemsize == 12 and abea.REALIGN.itemsize == 24
    assert (abea.REALIGN_SKIPPED, abea.REALIGN_NO_PAIRS, abea.REALIGN_NO_EVENT, abea.REALIGN_STRAND) == (M.SKIPPED, M.NO_PAIRS, M.NO_EVENT, M.STRAND)
    assert abea.CIGAR_OPS == M.OPS and abea.realign_room([10, 7], M.encode_cigar([("M", 5), ("N", 3), ("M", 2), ("M", 9)]), [0, 3], [3, 1]).tolist() == [20, 7]


def test_without_a_gpu_the_entry_points_say_so():
    lib = g.lib()
    none = [None] * 16
    host = lib.gab_abea_realign(None, *none, C.c_int32(-1), C.c_int32(-1), C.c_int64(1), None, None, None)
    dev = lib.gab_abea_realign_device(None, None, C.c_int64(0), None, None, None, None, None, C.c_int64(0), None, None, None, None, C.c_int64(0), None, None,
                                      None, C.c_int64(0), None, None, C.c_int32(-1), C.c_int32(-1), C.c_int64(1), None, C.c_int64(0), None, None, None)
    stats = lib.gab_abea_realign_last_stats(None, None, None, None, None, None, None, None)
    want = -19 if lib.gab_device_count() <= 0 else -22      # GAB_ENODEV: no quiet fall-back; with a GPU a NULL handle is GAB_EINVAL
    assert (host, dev, stats) == (want, want, want)
    assert lib.gab_last_error()
