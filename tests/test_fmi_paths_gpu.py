"""GPU: which route of genarchbench_amd/csrc/fmi.hip every read, list and phase takes (gab_fmi_last_paths) against the CPU model of
the routes (oracle.pyoracle.fmi_paths), one run per row of tests/fmi_path_cases.py; the records and the device's own read_off
(gab_fmi_seed_device) against the oracle, field by field; ext_calls and cp_occ_records against oracle and model.

The rows and what each must reach are in tests/fmi_path_cases.py; tests/test_fmi_paths_model.py asserts on the CPU that they do."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from tests import fmi_path_cases as cases
from tests.test_fmi_paths_model import model_of, oracle_of

pytestmark = pytest.mark.gpu

KNOBS = ("GAB_FMI_WIDE", "GAB_FMI_WIDE_CAP", "GAB_FMI_LDS_ENTRIES", "GAB_FMI_WIDE_LISTS", "GAB_FMI_KMER_DEPTH", "GAB_FMI_BATCH",
         "GAB_FMI_SCRATCH_MB", "GAB_FMI_WAVES")


def run_device(case, monkeypatch):
    """one gab_fmi_seed_device call on a fresh handle made under the row's knobs (a handle reads them when it is made)
    -> (records, read_off as the device wrote them, last_stats, last_paths)"""
    import torch
    from genarchbench_amd.fmi import FMI_search, SMEM_DTYPE
    idx, reads = cases.load(case.input)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    f = FMI_search(arrays=(idx.ref_seq_len, idx.count, idx.cp_occ, idx.sentinel_index))
    try:
        dev = torch.device("cuda:0")
        enc = torch.from_numpy(np.ascontiguousarray(reads.enc)).to(dev); ln = torch.from_numpy(reads.len).to(dev)
        d_out, d_off, n = f.seed_device(enc, ln, case.msl, stream=torch.cuda.current_stream().cuda_stream)
        hip = C.CDLL("libamdhip64.so")
        host = np.zeros(max(n, 1) * 40, np.uint8)
        if n:
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(d_out), C.c_size_t(n * 40), C.c_int(2)) == 0
        off = np.zeros(reads.n + 1, np.int64)
        assert hip.hipMemcpy(off.ctypes.data_as(C.c_void_p), C.c_void_p(d_off), C.c_size_t(8 * (reads.n + 1)), C.c_int(2)) == 0
        return host[:n * 40].view(SMEM_DTYPE), off, f.last_stats(), f.last_paths()
    finally:
        f.close()


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_routes(case, monkeypatch):
    w, woff, calls = oracle_of(case.input, case.msl)
    want, extra = model_of(case)
    got, goff, st, paths = run_device(case, monkeypatch)
    print(f"\n{case.name}: {paths} cp_occ_records={st['cp_occ_records']} kernel_ms={st['kernel_ms']:.3f}")
    # 1. the records and the read_off the device wrote
    np.testing.assert_array_equal(goff, woff)
    assert len(got) == len(w)
    for fld in ("rid", "m", "n", "k", "l", "s"):
        np.testing.assert_array_equal(got[fld], w[fld], err_msg=fld)
    # 2. extensions and SMEMs
    assert st["ext_calls"] == calls and st["smems"] == len(w)
    assert paths["index_ext"] + paths["table_ext"] == calls
    if not case.weak:
        # 3. + 4. every route counter, and the CP_OCC records the index extensions fetched
        assert paths == want
        assert st["cp_occ_records"] == extra["cp_occ_records"]
        return
    # the queues ran full: who got a place depends on timing
    cap = int(case.env["GAB_FMI_WIDE_CAP"])
    assert paths["wide_items"] <= cap and paths["reruns"] in ((0, 1) if case.weak == 1 else (1,))
    if paths["reruns"] == 0:
        assert paths["wide_cands"] <= cap and paths["wide_min"] == want["wide_min"]
        assert paths["positions"] + paths["wide_cands"] == want["positions"] + want["wide_cands"]
    else:                                    # the batch again, every phase with its own lane: the run without hand-over
        alone, alone_x = model_of(case, wide_min=0)
        assert paths == dict(alone, reruns=1)
        assert st["cp_occ_records"] == alone_x["cp_occ_records"]


def test_last_paths_needs_a_run_and_survives_reserve(monkeypatch):
    """GAB_EINVAL before the first run; gab_fmi_reserve (an empty batch through the whole path) leaves the answer as it leaves
    last_stats"""
    from genarchbench_amd._lib import GabError
    from genarchbench_amd.fmi import FMI_search
    case = next(c for c in cases.CASES if c.name == "stride_255")
    idx, reads = cases.load(case.input)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    f = FMI_search(arrays=(idx.ref_seq_len, idx.count, idx.cp_occ, idx.sentinel_index))
    with pytest.raises(GabError) as e:
        f.last_paths()
    assert e.value.code == -22
    f.reserve(500, 151)
    with pytest.raises(GabError):
        f.last_paths()
    f.seed(reads, case.msl)
    before, stats = f.last_paths(), f.last_stats()
    assert before == model_of(case)[0]
    f.reserve(500, 151)
    assert f.last_paths() == before and f.last_stats()["ext_calls"] == stats["ext_calls"]
    f.close()


def test_clone_takes_the_hand_over_from_its_source_and_the_ring_from_its_own_environment(monkeypatch):
    """gab_fmi_clone: the scratch budget, batch, waves, hand-over threshold and queue places are the SOURCE handle's, whatever the
    environment says when the clone is made; ring entries, list format and debug are read from that environment"""
    from genarchbench_amd.fmi import FMI_search
    idx, reads = cases.load("nested")
    w, woff, _ = oracle_of("nested", 19)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GAB_FMI_WIDE", "4"); monkeypatch.setenv("GAB_FMI_BATCH", "1024")
    owner = FMI_search(arrays=(idx.ref_seq_len, idx.count, idx.cp_occ, idx.sentinel_index))
    try:
        monkeypatch.setenv("GAB_FMI_WIDE", "0"); monkeypatch.setenv("GAB_FMI_LDS_ENTRIES", "4")
        clone = owner.clone()
        try:
            got, goff = clone.seed(reads, 19)
            paths = clone.last_paths()
        finally:
            clone.close()
    finally:
        owner.close()
    print(f"\nclone: {paths}")
    assert paths["wide_min"] == 4 and paths["wide_items"] > 0      # the source's GAB_FMI_WIDE=4, not the environment's 0
    assert paths["lds_entries"] == 4                               # the clone's own environment
    np.testing.assert_array_equal(goff, woff)
    assert len(got) == len(w)
    for fld in ("rid", "m", "n", "k", "l", "s"):
        np.testing.assert_array_equal(got[fld], w[fld], err_msg=fld)
