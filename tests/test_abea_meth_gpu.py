"""abea's call-methylation on the GPU: gab_abea_meth and its device form, bit for bit against the reference's recorded results
(tests/golden/abea_meth_expected.json) on the fixture reads and the constructed cases, against the model (tests/abea_meth_model.py)
where the reference cannot run, and the input rules."""
import numpy as np
import pytest

import abea_meth_model as M
import abea_realign_model as R
from test_abea_meth_model import load_meth_fixture, model_of, model_of_cases
from test_abea_realign_gpu import read_of

pytestmark = pytest.mark.gpu
F = np.float32
GAB_EINVAL = -22


@pytest.fixture(scope="module")
def aligner():
    from genarchbench_amd.abea import EventAligner
    model, cpg, _, _, _ = load_meth_fixture()
    h = EventAligner(*model)
    h.set_cpg_model(*cpg)
    yield h
    h.close()


@pytest.fixture(scope="module")
def flat_aligner():
    from genarchbench_amd.abea import EventAligner
    h = EventAligner(*load_meth_fixture()[0])
    h.set_cpg_model(*M.FLAT_CPG)
    yield h
    h.close()


def bits_of(got, i):
    """read i of (sites, out_off, records) as the golden JSON holds a read"""
    s, off, res = got
    mine = s[off[i]:off[i] + res[i]["n_sites"]]
    rec = {k: int(res[i][k]) for k in M.COUNTERS}
    assert int(res[i]["pad"]) == 0
    return rec, [[int(x[f]) for f in ("start_position", "end_position", "n_cpg", "first_cpg", "event_start", "event_stop")] +
                 [int(np.array([x["ll_unmethylated"]], F).view(np.uint32)[0]), int(np.array([x["ll_methylated"]], F).view(np.uint32)[0])] for x in mine]


def check(got, i, want, name):
    rec, sites = bits_of(got, i)
    assert rec == {k: want[k] for k in M.COUNTERS}, f"{name}: {rec}"
    assert sites == want["sites"], f"{name}: sites, order and both floats bit for bit"
    assert [s[0] for s in sites] == sorted(s[0] for s in sites)


def want_of_model(sites, rec):
    return dict({k: int(rec[k]) for k in M.COUNTERS}, sites=M.site_bits(sites))


def device_form(aligner, reads, canary=0x5a, room=None, slack=2):
    """the same batch through gab_abea_meth_device -> (sites, out_off, records)"""
    import torch
    from genarchbench_amd import abea
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p = abea.pack_aligned_reads(reads)
    if room is None:
        room = abea.meth_room(p[0], p[1], p[2])
    out_off = off(room)
    total = int(np.sum(room))
    out = torch.full(((total + slack) * 32,), canary, dtype=torch.uint8, device="cuda")
    res = torch.full((len(reads) * 40,), canary, dtype=torch.uint8, device="cuda")
    try:
        aligner.call_methylation_device(up(p[0]), up(p[1]), up(p[2]), up(p[3]), up(p[4]), up(p[5].view(np.int32)), up(p[6]), up(p[7]), up(p[8]), up(p[9]), up(p[10]),
                                        up(p[11]), up(p[12].view(np.int32).reshape(-1, 2)), up(p[13]), up(p[14].view(np.uint8)), out, up(out_off), res)
    finally:
        device_form.last = (out.cpu().numpy(), res.cpu().numpy())
    o, r = device_form.last
    assert (o[total * 32:] == canary).all()              # nothing behind the last read's room
    sites = o[:total * 32].view(abea.SITE); recs = r.view(abea.METH)
    for i in range(len(reads)):                          # nor behind a read's own sites
        assert (o[(out_off[i] + recs[i]["n_sites"]) * 32:(out_off[i] + room[i]) * 32] == canary).all()
    return sites, out_off, recs


def test_the_golden_fixture_equals_the_reference(aligner):
    """every fixture read without an N operation through the host entry and through the device entry"""
    from genarchbench_amd import abea
    _, _, reads, _, exp = load_meth_fixture()
    idx = sorted(reads)
    batch = [read_of(reads[i]) for i in idx]
    got = aligner.call_methylation_reads(batch)
    st = aligner.meth_last_stats()
    for k, i in enumerate(idx):
        check(got, k, exp["reads"][str(i)], f"read {i}")
    res = got[2]
    assert st["reads"] == len(idx) and st["sites"] == int(res["n_sites"].sum()) == exp["counts"]["sites"] and st["groups"] == int(res["groups"].sum())
    assert st["cells"] == int(res["cells"].sum()) and st["rows"] == sum(abs(s[5] - s[4]) + 1 for i in idx for s in exp["reads"][str(i)]["sites"])
    assert 0 < st["kernel_ms"] <= st["total_ms"] * 1.001 and abs(st["prep_ms"] + st["score_ms"] - st["kernel_ms"]) < 1e-3
    dev = device_form(aligner, batch)
    for k, i in enumerate(idx):
        check(dev, k, exp["reads"][str(i)], f"read {i}, device form")
    for i, lines in exp["lines"].items():                # the printed lines of three reads
        k = idx.index(int(i)); r = reads[int(i)]
        mine = got[0][got[1][k]:got[1][k] + res[k]["n_sites"]]
        assert abea.methylation_rows("contig", "read", r["ref"], r["ref_pos"], mine) == lines


def test_the_constructed_cases(aligner, flat_aligner):
    """every case, the defined deviations among them, one read a call and all in one batch, host and device form, against the model"""
    _, _, _, cases, exp = load_meth_fixture()
    want = model_of_cases()
    plain = [n for n in cases if n not in M.FLAT_CASES]
    for n in cases:
        h = flat_aligner if n in M.FLAT_CASES else aligner
        w = want_of_model(*want[n])
        assert w == {k: v for k, v in exp["cases"][n].items() if k != "by_reference"}, n
        check(h.call_methylation_reads([read_of(cases[n])]), 0, w, n)
    batch = [read_of(cases[n]) for n in plain]
    for got, form in ((aligner.call_methylation_reads(batch), "host"), (device_form(aligner, batch), "device")):
        for k, n in enumerate(plain):
            check(got, k, want_of_model(*want[n]), f"{n}, one batch, {form} form")
    check(device_form(flat_aligner, [read_of(cases[n]) for n in M.FLAT_CASES]), 0, want_of_model(*want[M.FLAT_CASES[0]]), "flat, device form")


@pytest.mark.parametrize("part", range(5))
def test_every_kmer_count_of_a_group(aligner, part):
    """one group of every width from 16 to 216 k-mers (a fifth of them a case), built from the kernel's shape as the library reports it:
    every number of lanes in use, every position of the last k-mer among its lane's blocks, both paths and the change between them;
    forward and reverse reads alternate.  Against the model, which the golden script holds to the reference on a sample of widths."""
    from genarchbench_amd import abea
    model, cpg, _, _, _ = load_meth_fixture()
    bpl, one = abea.meth_shape()
    widths = M.all_widths(bpl, one)[part::5]
    cases = M.width_cases(model, widths)
    want = {n: want_of_model(*model_of(cpg, c)) for n, c in cases.items()}
    assert all(w["n_sites"] == 1 and w["cells"] == 2 * 13 * n for n, w in want.items())
    batch = [read_of(cases[n]) for n in widths]
    for got, form in ((aligner.call_methylation_reads(batch), "host"), (device_form(aligner, batch), "device")):
        for k, n in enumerate(widths):
            check(got, k, want[n], f"{n} k-mers, {form} form")


SCORE_WAVEFRONTS = 2048 * 4                              # `SCORE_BLOCKS` x `SCORE_WAVES` of abea_meth.hip: the persistent wavefronts that take items off one counter


def test_more_items_than_scoring_wavefronts_and_more_than_64_sites_a_read(aligner):
    """135 reads of 70 scored groups each, three distinct ones (one of them reverse) 45 times over in a seeded order: 9450 items for
    8192 wavefronts, so some wavefront takes a second item whatever the scheduling; and 70 sites in a read, so that the slot of a site
    is carried over from a step in which all 64 positions' worth of earlier sites were counted"""
    model, cpg, _, _, _ = load_meth_fixture()
    rng = np.random.default_rng(20251203)
    distinct, want = [], []
    for rev in (False, True, False):
        at = (30 + np.concatenate([[0], np.cumsum(rng.integers(20, 49, 69))])).tolist()      # isolated: more than ten bases apart, and scoreable
        read = M.bases_with_cpgs(rng, at[-1] + 40, at)
        c = R.case(rng, model, R.revcomp(read) if rev else read, rev=rev, per=1)
        w = want_of_model(*model_of(cpg, c))
        assert 2200 < len(read) <= 2500 and w["n_sites"] == w["groups"] == 70 and w["flags"] == 0 and w["cells"] == 70 * 2 * 21 * 16
        distinct.append(read_of(c)); want.append(w)
    order = np.random.default_rng(20251204).permutation(np.repeat(np.arange(3), 45))
    batch = [distinct[j] for j in order]
    assert len(batch) == 135 and 70 * len(batch) > SCORE_WAVEFRONTS + 1000
    for got, form in ((aligner.call_methylation_reads(batch), "host"), (device_form(aligner, batch), "device")):
        st = aligner.meth_last_stats()
        for k, j in enumerate(order):
            check(got, k, want[j], f"read {k} (a copy of read {j}), {form} form")
        assert st["reads"] == 135 and st["sites"] == int(got[2]["n_sites"].sum()) == 70 * 135 and st["groups"] == 70 * 135
        assert st["cells"] == int(got[2]["cells"].sum()) == 135 * want[0]["cells"] and st["rows"] == 135 * 70 * 21


def test_the_flank_table_grows_with_the_longest_read_of_a_call():
    """a fresh handle: a read of 120 events, then one of 6000 with a group on 401 rows, then the first again"""
    from genarchbench_amd.abea import EventAligner
    model, cpg, _, _, _ = load_meth_fixture()
    rng = np.random.default_rng(20251205)
    short = R.case(rng, model, M.bases_with_cpgs(rng, 125, [60]), per=1)
    cnt = np.ones(5620, np.int64); cnt[50:70] = 20
    long = R.case(rng, model, M.bases_with_cpgs(rng, 5625, [60, 3000, 5500]), counts=cnt, epb=4.0)
    want_short, want_long = want_of_model(*model_of(cpg, short)), want_of_model(*model_of(cpg, long))
    assert short["events"].size == 120 and long["events"].size == 6000 and want_short["n_sites"] == 1 and want_long["n_sites"] == 3
    assert want_long["sites"][0][5] - want_long["sites"][0][4] == 400
    h = EventAligner(*model)
    try:
        h.set_cpg_model(*cpg)
        for c, want, name in ((short, want_short, "120 events"), (long, want_long, "6000 events"), (short, want_short, "120 events again")):
            check(h.call_methylation_reads([read_of(c)]), 0, want, name)
            check(device_form(h, [read_of(c)]), 0, want, name + ", device form")
    finally:
        h.close()


def test_the_host_entry_with_slabs_that_do_not_start_at_0(aligner):
    """every slab with a junk prefix of an odd length, the reads in reverse order with gaps, two reads on the same reference bytes and
    events: byte for byte the result of the same reads packed from 0, and not a byte written outside a read's sites"""
    from genarchbench_amd import abea
    from test_abea_realign_launch_gpu import scattered_room, windowed
    _, _, _, cases, _ = load_meth_fixture()
    names = ["separation_11", "lower_case_and_iupac", "kmers_64_reverse", "no_cpg", "cigar_operations", "single_cpg", "separation_11"]
    want = model_of_cases()
    packed = abea.pack_aligned_reads([read_of(cases[n]) for n in names])
    plain = aligner.call_methylation(*packed)
    w = windowed(packed, (6, 0), 41)
    assert w[1][6] == w[1][0] and w[10][6] == w[10][0] and w[1].min() == 7 and w[6].min() == 3 and w[10].min() == 5 and w[13].min() == 9
    room = abea.meth_room(w[0], w[1], w[2])
    assert room.tolist() == [2, 3, 1, 0, 3, 1, 2]
    out_off, total = scattered_room(room, 42)
    out = (np.frombuffer(bytes([0xa5]) * 32 * total, abea.SITE).copy(), np.frombuffer(bytes([0xa5]) * 40 * (len(names) + 1), abea.METH).copy())
    got = aligner.call_methylation(*w, out_off=out_off, out=out)
    assert out[1][:len(names)].tobytes() == plain[2].tobytes() and out[1][len(names):].tobytes() == bytes([0xa5]) * 40
    written = np.zeros(total, bool)
    for i, n in enumerate(names):
        check(got, i, want_of_model(*want[n]), f"{n} (read {i})")
        k = int(plain[2][i]["n_sites"])
        assert out[0][out_off[i]:out_off[i] + k].tobytes() == plain[0][plain[1][i]:plain[1][i] + k].tobytes(), f"{n} (read {i})"
        written[out_off[i]:out_off[i] + k] = True
    assert out[0][~written].tobytes() == bytes([0xa5]) * 32 * int((~written).sum()) and written.sum() == 12


def test_repeatable_and_independent_of_the_batch_order(aligner):
    _, _, reads, cases, _ = load_meth_fixture()
    names = [n for n in cases if n not in M.FLAT_CASES]
    batch = [read_of(reads[i]) for i in sorted(reads)[:40]] + [read_of(cases[n]) for n in names]
    first = aligner.call_methylation_reads(batch)
    again = aligner.call_methylation_reads(batch)
    assert first[0].tobytes() == again[0].tobytes() and first[2].tobytes() == again[2].tobytes()
    perm = np.random.default_rng(7).permutation(len(batch))
    shuffled = aligner.call_methylation_reads([batch[j] for j in perm])
    for k, j in enumerate(perm):
        assert bits_of(shuffled, k) == bits_of(first, j), f"read {j} at place {k}"
    empty = aligner.call_methylation_reads([])
    assert empty[0].size == 0 and aligner.meth_last_stats()["reads"] == 0


def test_out_off_may_leave_gaps_and_any_order(aligner):
    from genarchbench_amd import abea
    _, _, _, cases, _ = load_meth_fixture()
    names = ["separation_11", "single_cpg", "lower_case_and_iupac"]
    want = model_of_cases()
    p = abea.pack_aligned_reads([read_of(cases[n]) for n in names])
    out_off = np.array([20, 0, 7], np.int64)             # rooms 2, 1, 3
    sites = np.zeros(25, abea.SITE); sites["n_cpg"] = -9
    got = aligner.call_methylation(*p, out_off=out_off, out=(sites, np.zeros(3, abea.METH)))
    for k, n in enumerate(names):
        check(got, k, want_of_model(*want[n]), n)
    used = {20, 21, 0, 7, 8, 9}
    assert all((sites[j]["n_cpg"] == -9) == (j not in used) for j in range(25))


def test_the_input_rules(aligner):
    """each broken rule is GAB_EINVAL naming the read, and the outputs stay as they were"""
    import genarchbench_amd as g
    from genarchbench_amd.abea import EventAligner
    model, _, _, cases, _ = load_meth_fixture()
    good = cases["separation_11"]

    def broken(**kw):
        c = dict(good); c.update(kw)
        return c

    def with_calib(**kw):
        return broken(calib=dict(good["calib"], **kw))
    ref_bad = bytearray(good["ref"]); ref_bad[5] = ord("!")
    ev_bad = good["events"].copy(); ev_bad[3] = np.nan
    map_bad = good["map"].copy(); map_bad[9] = (0, good["events"].size)
    rules = {"an N operation": broken(cigar=R.encode_cigar([("M", 60), ("N", 10), ("M", 70)])),
             "a P operation": broken(cigar=R.encode_cigar([("M", 60), ("P", 1), ("M", 80)])),
             "a CIGAR longer than the reference": broken(cigar=R.encode_cigar([("M", 141)]), seq_len=141, map=np.full((136, 2), -1, np.int32)),
             "a CIGAR longer than the read": broken(cigar=R.encode_cigar([("M", 100), ("I", 50)])),
             "a reference byte that is no base": broken(ref=bytes(ref_bad)),
             "an event mean that is no number": broken(events=ev_bad),
             "a map entry outside the events": broken(map=map_bad),
             "var of zero": with_calib(var=F(0.0)), "a scale that is no number": with_calib(scale=F(np.inf))}
    for why, c in rules.items():
        for form in ("host", "device"):
            batch = [read_of(good), read_of(c)]
            with pytest.raises(RuntimeError) as e:
                if form == "host":
                    from genarchbench_amd import abea
                    sites = np.zeros(8, abea.SITE); sites["n_cpg"] = -9; res = np.zeros(2, abea.METH); res["groups"] = -9
                    aligner.call_methylation(*abea.pack_aligned_reads(batch), out_off=np.array([0, 4], np.int64), out=(sites, res))
                else:
                    device_form(aligner, batch)
            assert "read 1" in str(e.value), f"{why}: {e.value}"
            if form == "host":
                assert (sites["n_cpg"] == -9).all() and (res["groups"] == -9).all(), why
            else:
                assert all((a == 0x5a).all() for a in device_form.last), why
    # less room than groups
    with pytest.raises(RuntimeError, match="room"):
        device_form(aligner, [read_of(good), read_of(good)], room=np.array([2, 1], np.int64), slack=0)
    assert all((a == 0x5a).all() for a in device_form.last)
    with pytest.raises(RuntimeError, match="room"):
        from genarchbench_amd import abea
        aligner.call_methylation(*abea.pack_aligned_reads([read_of(good), read_of(good)]), out_off=np.array([0, 1], np.int64), out=(np.zeros(8, abea.SITE), np.zeros(2, abea.METH)))
    # no CpG model yet
    h = EventAligner(*model)
    try:
        with pytest.raises(RuntimeError, match="gab_abea_set_cpg_model"):
            h.call_methylation_reads([read_of(good)])
    finally:
        h.close()
    assert g.lib().gab_last_error()
    check(aligner.call_methylation_reads([read_of(good)]), 0, want_of_model(*model_of_cases()["separation_11"]), "after the errors")
