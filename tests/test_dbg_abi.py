"""CPU: the dbg entry points that need no device -- gab_dbg_room and gab_dbg_plan_regions against tests/dbg_model.py, argument checks,
and GAB_ENODEV from gab_dbg_create where there is no GPU (no quiet fall-back)."""
import ctypes as C

import numpy as np
import pytest

from tests import dbg_cases as dc
from tests import dbg_model as M

EINVAL, ERANGE, ENODEV = -22, -34, -19


@pytest.fixture(scope="module")
def lib():
    import genarchbench_amd
    return genarchbench_amd.lib()


def test_create_without_a_device(lib):
    from genarchbench_amd import dbg
    if lib.gab_device_count() > 0:
        h = dbg.GraphBuilder(0)
        h.close()
        return
    with pytest.raises(dbg.GabError) as e:
        dbg.GraphBuilder(0)
    assert e.value.code == ENODEV


def test_null_handle_and_arguments(lib):
    want = EINVAL
    assert lib.gab_dbg_build(None, *([None] * 10), 0, None, None, 0, None, None, 0, None) == want
    assert lib.gab_dbg_build_device(None, None, None, 0, *([None] * 5), 0, None, None, None, 0, None, None, 0, None, None, 0, None, None) == want
    assert lib.gab_dbg_last_stats(None, None) == want and lib.gab_dbg_last_phases(None, None, None, None) == want
    assert lib.gab_dbg_reserve(None, 1, 1, 1) == want
    assert lib.gab_dbg_create(0, None) == want
    assert b"NULL handle" in lib.gab_last_error() or b"NULL" in lib.gab_last_error()
    lib.gab_dbg_destroy(None)


def test_room_is_the_models(lib):
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    packed = dbg.pack_regions(regions, reads)
    for k in (1, 15, 16):
        total, each = dbg.room(packed, k, per_region=True)
        want = M.room(regions, reads, k)
        assert np.array_equal(each, want) and total == int(want.sum())
    # the bound holds and is met: a region of all-distinct k-mers has exactly that many nodes
    off, recs, _ = dc.fixture_model()
    assert (np.diff(off) <= M.room(regions, reads, doc["k"])).all()
    k, _, regs, rds = dc.constructed()["all_distinct_255"]
    assert len(M.build_region(b"", 0, rds, k)) == M.room([(b"", 0, 0, 1)], rds, k)[0]
    with pytest.raises(dbg.GabError) as e:
        dbg.room(packed, 17)
    assert e.value.code == EINVAL
    bad = dict(packed, read_end=packed["read_end"] + len(reads))
    with pytest.raises(dbg.GabError) as e:
        dbg.room(bad, 15)
    assert e.value.code == EINVAL and "region 0" in str(e.value)


def test_pack_regions_round_trip():
    from genarchbench_amd import dbg
    _, regions, reads, _ = dc.fixture()
    p = dbg.pack_regions(regions, reads)
    for i in (0, 5, len(regions) - 1):
        assert p["ref"][p["ref_off"][i]:p["ref_off"][i] + p["ref_len"][i]].tobytes() == regions[i][0]
        assert (p["ref_start"][i], p["read_begin"][i], p["read_end"][i]) == regions[i][1:]
    j = 17
    assert p["seq"][p["read_off"][j]:p["read_off"][j] + p["read_len"][j]].tobytes() == reads[j][0] and p["read_flag"][j] == reads[j][2]
    assert p["qual"][p["read_off"][j]:p["read_off"][j] + p["read_len"][j]].tobytes() == reads[j][1]


def _plan(beg, end, pos, rend, contig):
    from genarchbench_amd import dbg
    got = dbg.plan_regions(beg, end, pos, rend, contig)
    return np.stack([got[f] for f in ("start", "ref_start", "ref_len", "read_begin", "read_end")], 1).astype(np.int64).reshape(-1, 5)


def test_plan_regions_is_the_models(lib):
    _, _, _, z = dc.fixture()
    n = len(z["contig"])
    assert np.array_equal(_plan(0, n, z["read_pos"], z["read_end"], n), z["plan"])
    rng = np.random.default_rng(3)
    for trial in range(20):
        n_reads = int(rng.integers(0, 400))
        pos = np.sort(rng.integers(0, 20000, n_reads)).astype(np.int32)
        rend = (pos + rng.integers(0, 151, n_reads)).astype(np.int32)
        beg = int(rng.integers(0, 9000)); end = beg + int(rng.integers(0, 9000)); contig = int(rng.choice([end, end + 700, end + 5000, max(0, end - 300)]))
        assert np.array_equal(_plan(beg, end, pos, rend, contig), M.plan_regions(beg, end, pos.tolist(), rend.tolist(), contig)), trial
    # no reads, an empty interval, a window of one base
    assert np.array_equal(_plan(100, 2000, [], [], 10000), M.plan_regions(100, 2000, [], [], 10000))
    assert len(_plan(500, 500, [1], [2], 1000)) == 0
    assert np.array_equal(_plan(0, 1, [0, 0, 1], [1, 5, 9], 50), M.plan_regions(0, 1, [0, 0, 1], [1, 5, 9], 50))


def test_plan_regions_capacity_and_errors(lib):
    from genarchbench_amd import dbg
    pos = np.array([5, 900, 1800], np.int32); rend = pos + 100
    need = C.c_int64(-1)
    out = np.frombuffer(bytes([0x5A]) * 32 * 4, dbg.REGION).copy()
    rc = lib.gab_dbg_plan_regions(0, 3000, pos.ctypes.data_as(C.c_void_p), rend.ctypes.data_as(C.c_void_p), 3, 5000, out.ctypes.data_as(C.c_void_p), 3, C.byref(need))
    assert rc == ERANGE and need.value == 4 and out.tobytes() == bytes([0x5A]) * 128, "too little room: the need, and nothing written"
    rc = lib.gab_dbg_plan_regions(0, 3000, pos.ctypes.data_as(C.c_void_p), rend.ctypes.data_as(C.c_void_p), 3, 5000, out.ctypes.data_as(C.c_void_p), 4, C.byref(need))
    assert rc == 0 and need.value == 4 and out["start"].tolist() == [0, 750, 1500, 2250] and (out["pad"] == 0).all()
    for bad_pos, bad_end in (([5, 4], [9, 9]), ([5, 6], [9, 5])):        # not ascending; a read that ends before it starts
        with pytest.raises(dbg.GabError) as e:
            dbg.plan_regions(0, 3000, bad_pos, bad_end, 5000)
        assert e.value.code == EINVAL and "read 1" in str(e.value)
    with pytest.raises(dbg.GabError):
        dbg.plan_regions(10, 5, [], [], 100)
