"""The C ABI of gab_abea_meth without a GPU: the symbols, the records, the two host helpers bit for bit, the room rule's numbers,
and no quiet fall-back."""
import ctypes as C

import numpy as np

import genarchbench_amd as g

import abea_meth_model as M
import abea_realign_model as R
from test_abea_meth_model import load_meth_fixture

SYMBOLS = ("gab_abea_set_cpg_model", "gab_abea_meth", "gab_abea_meth_device", "gab_abea_meth_groups", "gab_abea_meth_logsum", "gab_abea_meth_shape",
           "gab_abea_meth_last_stats", "gab_abea_meth_stage_ms")


def test_the_symbols_are_exported():
    lib = g.lib()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_the_records_the_flags_and_the_shape_are_the_models():
    from genarchbench_amd import abea
    assert abea.SITE.itemsize == 32 and abea.METH.itemsize == 40 and abea.METH.fields["cells"][1] == 32
    assert abea.SITE.names == ("start_position", "end_position", "n_cpg", "first_cpg", "event_start", "event_stop", "ll_unmethylated", "ll_methylated")
    assert tuple(n for n in abea.METH.names if n != "pad") == M.COUNTERS
    assert (abea.METH_SKIPPED, abea.METH_NO_EVENT, abea.METH_STRAND, abea.METH_TRANSITIONS) == (M.SKIPPED, M.NO_EVENT, M.STRAND, M.TRANSITIONS)
    assert abea.NKMER_CPG == M.NKMER5 and abea.LOGSUM_TBL == M.LOGSUM_TBL
    v = C.c_int32(0); w = C.c_int32(0)
    assert g.lib().gab_abea_meth_shape(C.byref(v), C.byref(w)) == 0 and (v.value, w.value) == (M.BLOCKS_PER_LANE, M.ONE_BLOCK_KMERS) == abea.meth_shape()
    assert g.lib().gab_abea_meth_shape(None, None) == 0


def test_the_logsum_table_needs_no_gpu_and_is_the_references():
    from genarchbench_amd import abea
    assert abea.meth_logsum().tobytes() == M.TABLE.tobytes()
    assert g.lib().gab_abea_meth_logsum(None) == -22


def test_the_groups_need_no_gpu_and_are_the_models():
    """gab_abea_meth_groups = the room rule's number, on every fixture read and case, and where the preparation makes or unmakes a CpG"""
    from genarchbench_amd import abea
    _, _, reads, cases, _ = load_meth_fixture()
    refs = [r["ref"] for r in reads.values()] + [c["ref"] for c in cases.values()] + [b"", b"C", b"CG", b"cg", b"yk", b"CR", b"NG", b"CGACG" + b"T" * 8 + b"CG", b"CGACG" + b"T" * 9 + b"CG"]
    ref_len = np.array([len(r) for r in refs], np.int32)
    ref_off = np.concatenate([[0], np.cumsum(ref_len)[:-1]]).astype(np.int64)
    got = abea.meth_room(np.frombuffer(b"".join(refs), np.uint8), ref_off, ref_len)
    want = [len(M.cpg_groups(R.prepare_ref(r))) for r in refs]
    assert got.tolist() == want and want[-9:] == [0, 0, 1, 1, 1, 0, 0, 1, 2]
    assert abea.meth_room(np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int32)).size == 0
    lib = g.lib()
    assert lib.gab_abea_meth_groups(None, None, None, C.c_int64(1), None) == -22 and lib.gab_abea_meth_groups(None, None, None, C.c_int64(-1), None) == -22


def test_methylation_rows_print_the_references_lines():
    from genarchbench_amd import abea
    _, cpg, reads, _, exp = load_meth_fixture()
    for i, lines in exp["lines"].items():
        r = reads[int(i)]
        sites = np.zeros(len(lines), abea.SITE)
        for s, w in zip(sites, exp["reads"][i]["sites"]):
            for k, f in enumerate(("start_position", "end_position", "n_cpg", "first_cpg", "event_start", "event_stop")):
                s[f] = w[k]
        sites["ll_unmethylated"] = np.array([w[6] for w in exp["reads"][i]["sites"]], np.uint32).view(np.float32)
        sites["ll_methylated"] = np.array([w[7] for w in exp["reads"][i]["sites"]], np.uint32).view(np.float32)
        assert abea.methylation_rows("contig", "read", r["ref"], r["ref_pos"], sites) == lines


def test_without_a_gpu_the_entry_points_say_so():
    lib = g.lib()
    none = [None] * 16
    host = lib.gab_abea_meth(None, *none, C.c_int64(1), None, None, None)
    dev = lib.gab_abea_meth_device(None, None, C.c_int64(0), None, None, None, None, None, C.c_int64(0), None, None, None, None, C.c_int64(0), None, None,
                                   None, C.c_int64(0), None, None, C.c_int64(1), None, C.c_int64(0), None, None, None)
    model = lib.gab_abea_set_cpg_model(None, None, None, None)
    stats = lib.gab_abea_meth_last_stats(None, None, None, None, None, None, None, None)
    stage = lib.gab_abea_meth_stage_ms(None, None, None)
    want = -19 if lib.gab_device_count() <= 0 else -22      # GAB_ENODEV: no quiet fall-back; with a GPU a NULL handle is GAB_EINVAL
    assert (host, dev, model, stats, stage) == (want,) * 5
    assert lib.gab_last_error()
