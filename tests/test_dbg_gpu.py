"""GPU: gab_dbg_build / gab_dbg_build_device against the golden fixture of the compiled reference byte for byte, then the constructed
regions of tests/dbg_cases.py against tests/dbg_model.py.  Every compared value is an integer or a byte: no tolerance anywhere."""
import numpy as np
import pytest

from tests import dbg_cases as dc
from tests import dbg_model as M

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -22, -34


@pytest.fixture(scope="module")
def builder():
    from genarchbench_amd.dbg import GraphBuilder
    h = GraphBuilder(0)
    yield h
    h.close()


def on_device(builder, packed, k, min_qual, capacity, fill=0x5A):
    """build_device on tensors of the packed arrays -> (nodes returned, node_off, the whole record buffer as NODE records)"""
    import torch
    from genarchbench_amd import dbg
    dev = torch.device("cuda:0")
    t = {f: torch.from_numpy(np.ascontiguousarray(packed[f])).to(dev) for f in dbg.INPUTS}
    node_off = torch.full((len(packed["ref_len"]) + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    nodes = torch.full((capacity * dbg.NODE.itemsize,), fill, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    try:
        n = builder.build_device(t, node_off, nodes, k, min_qual, stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
        builder.seen = (node_off.cpu().numpy(), nodes.cpu().numpy().view(dbg.NODE))
    return (n,) + builder.seen


def check_case(builder, k, min_qual, regions, reads, device_too=True):
    from genarchbench_amd import dbg
    stats = {}
    want_off, want = M.build(regions, reads, k, min_qual, stats)
    packed = dbg.pack_regions(regions, reads)
    off, recs = builder.build(packed, k, min_qual)
    assert np.array_equal(off, want_off), (off.tolist(), want_off.tolist())
    assert recs.tobytes() == want.tobytes(), first_difference(recs, want)
    got = builder.last_stats()
    assert {f: got[f] for f in ("regions", "occurrences", "passed", "nodes", "edges")} == {f: stats[f] for f in ("regions", "occurrences", "passed", "nodes", "edges")}
    if device_too:
        n, doff, drecs = on_device(builder, packed, k, min_qual, len(want) + 3)
        assert n == len(want) and np.array_equal(doff, want_off) and drecs[:n].tobytes() == want.tobytes()
        assert drecs[n:].tobytes() == bytes([0x5A]) * 3 * dbg.NODE.itemsize, "the room behind the last record is written"
    return off, recs


def first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} records, the model has {len(want)}"
    i = int(np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[0])
    return f"record {i}: got {got[i]} want {want[i]}"


def test_golden_fixture_through_both_entry_points(builder):
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    want_off, want, stats = dc.fixture_model()
    packed = dbg.pack_regions(regions, reads)
    off, recs = builder.build(packed, doc["k"], doc["min_qual"], capacity=dbg.room(packed, doc["k"]))
    n, doff, drecs = on_device(builder, packed, doc["k"], doc["min_qual"], len(want))
    for name, o, r in (("host", off, recs), ("device", doff, drecs[:n])):
        assert np.array_equal(o, want_off), name
        for i, w in enumerate(doc["regions"]):
            assert dc.sha(r[o[i]:o[i + 1]]) == w["sha256"], f"{name} pointers, region {i}: {first_difference(r[o[i]:o[i + 1]], want[o[i]:o[i + 1]])}"
    for i, full in doc["full"].items():
        ref, start, _, _ = regions[int(i)]
        assert dbg.format_region(ref, start, reads, recs[off[int(i)]:off[int(i) + 1]]).decode() == full["line"]
    got = builder.last_stats()
    assert {f: got[f] for f in ("regions", "occurrences", "passed", "nodes", "edges")} == {f: stats[f] for f in ("regions", "occurrences", "passed", "nodes", "edges")}
    assert got["probes"] >= 2 * got["passed"] - 2 and got["kernel_ms"] > 0 and got["total_ms"] >= got["kernel_ms"] * 0.99


@pytest.mark.parametrize("params", [(1, 20), (16, 3), (7, 30)])
def test_golden_fixture_under_other_parameters(builder, params):
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    off, recs = builder.build(dbg.pack_regions(regions, reads), *params)
    for i, w in enumerate(doc["other_parameters"]["%d,%d" % params]):
        assert dc.sha(recs[off[i]:off[i + 1]]) == w, f"region {i}"


CASES = dc.constructed()


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed(builder, name):
    k, mq, regions, reads = CASES[name]
    off, recs = check_case(builder, k, mq, regions, reads)
    if name == "weight_above_2_24":
        assert len(recs) == 1 and recs["weight"][0] == 700 * 135 * 2 * 93 + 270 > 1 << 24 and recs["edge_weight"][0, 0] == 700 * 135 * 93 + 135
    if name == "homopolymer":
        assert np.diff(off)[1:].tolist() == [1, 1] and recs[off[2]]["weight"] == 2 * 93 and recs[off[2]]["edge_to"][0] == 0
    if name == "five_successors":
        assert recs["n_edges"].max() == 4


def test_more_regions_than_a_grid_dimension_of_16_bits(builder):
    k, mq, regions, reads = dc.many_regions()
    from genarchbench_amd import dbg
    shapes = [M.build_region(ref, start, reads[b:e], k, mq, b) for ref, start, b, e in regions[:3]]
    off, recs = builder.build(dbg.pack_regions(regions, reads), k, mq)
    sizes = np.array([len(s) for s in shapes])[np.arange(len(regions)) % 3]
    assert np.array_equal(np.diff(off), sizes)
    for i in (0, 1, 2, 65535, 65536, 65537, len(regions) - 1):
        assert recs[off[i]:off[i + 1]].tobytes() == shapes[i % 3].tobytes(), i
    want = np.concatenate([np.tile(np.concatenate(shapes), len(regions) // 3)] + [shapes[i] for i in range(len(regions) % 3)])
    assert recs.tobytes() == want.tobytes()


def test_same_bytes_twice_and_in_reverse_order(builder):
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    packed = dbg.pack_regions(regions, reads)
    off1, recs1 = builder.build(packed, doc["k"], doc["min_qual"])
    off2, recs2 = builder.build(packed, doc["k"], doc["min_qual"])
    assert np.array_equal(off1, off2) and recs1.tobytes() == recs2.tobytes()
    off3, recs3 = builder.build(dbg.pack_regions(regions[::-1], reads), doc["k"], doc["min_qual"])
    n = len(regions)
    for i in range(n):
        assert recs3[off3[n - 1 - i]:off3[n - i]].tobytes() == recs1[off1[i]:off1[i + 1]].tobytes(), i


def test_too_little_room_writes_nothing(builder):
    from genarchbench_amd import dbg
    doc, regions, reads, _ = dc.fixture()
    want_off, want, _ = dc.fixture_model()
    packed = dbg.pack_regions(regions, reads)
    with pytest.raises(dbg.GabError) as e:
        on_device(builder, packed, doc["k"], doc["min_qual"], len(want) - 1)
    assert e.value.code == ERANGE and builder.needed == len(want)
    node_off, nodes = builder.seen
    assert (node_off == 0x5A5A5A5A5A5A5A5A).all() and nodes.tobytes() == bytes([0x5A]) * (len(want) - 1) * dbg.NODE.itemsize
    with pytest.raises(dbg.GabError) as e:
        builder.build(packed, doc["k"], doc["min_qual"], capacity=len(want) - 1)
    assert e.value.code == ERANGE and builder.needed == len(want)
    off, recs = builder.build(packed, doc["k"], doc["min_qual"], capacity=len(want))        # exactly enough
    assert recs.tobytes() == want.tobytes()


def test_a_lower_case_byte_is_refused_and_names_the_region(builder):
    from genarchbench_amd import dbg
    _, regions, reads, _ = dc.fixture()
    want_off, want, _ = dc.fixture_model()
    regions = list(regions)
    ref = bytearray(regions[4][0]); ref[100] = ord("a")
    regions[4] = (bytes(ref),) + regions[4][1:]
    packed = dbg.pack_regions(regions, reads)
    with pytest.raises(dbg.GabError) as e:
        on_device(builder, packed, 15, 20, len(want))
    assert e.value.code == EINVAL and "region 4" in str(e.value)
    node_off, nodes = builder.seen
    assert (node_off == 0x5A5A5A5A5A5A5A5A).all() and nodes.tobytes() == bytes([0x5A]) * len(want) * dbg.NODE.itemsize, "a partial result"
    # ... in a read: the first region that holds the read is named
    _, regions, reads, _ = dc.fixture()
    reads = list(reads)
    j = regions[2][2] if regions[2][2] >= regions[1][3] else regions[1][3]        # a read of region 2 that region 1 does not have
    assert regions[2][2] <= j < regions[2][3]
    reads[j] = (reads[j][0][:-1] + b"c", reads[j][1], reads[j][2])
    with pytest.raises(dbg.GabError) as e:
        builder.build(dbg.pack_regions(regions, reads), 15, 20)
    assert e.value.code == EINVAL and "region 2" in str(e.value)


def test_argument_checks_with_a_device(builder):
    from genarchbench_amd import dbg
    _, regions, reads, _ = dc.fixture()
    packed = dbg.pack_regions(regions[:2], reads)
    for k in (0, 17):
        with pytest.raises(dbg.GabError) as e:
            builder.build(packed, k, 20)
        assert e.value.code == EINVAL
    bad = dict(packed, read_end=np.array([len(reads) + 1, 0], np.int64))
    with pytest.raises(dbg.GabError) as e:
        builder.build(bad, 15, 20)
    assert e.value.code == EINVAL
    bad = dict(packed, ref_off=packed["ref_off"] + len(packed["ref"]))
    with pytest.raises(dbg.GabError) as e:
        on_device(builder, bad, 15, 20, 10)
    assert e.value.code == EINVAL and "outside the slab" in str(e.value)
    off, recs = builder.build(dbg.pack_regions([], []), 15, 20)
    assert off.tolist() == [0] and len(recs) == 0
