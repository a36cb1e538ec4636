"""chain / fast-chain: the batches of tests/test_chain_forms_gpu.py -- calls on either side of every limit a kernel form of
genarchbench_amd/csrc/chain.hip / chain_tab.hip sets for the calls it takes.

A case is (calls, want): `calls` as tools.gabgen.chain_from_calls takes them; want[mode][c] is what the TABLE form does with call c
when every call is sent there (3 folds it, 4 does not take it: the conditions of ctab_prep), for mode 0 chain and 1 fast-chain."""
import numpy as np

TOP = (1 << 24) - (1 << 15)      # scores a key holds: 24 bits above the 7-bit code, a block's growth to spare


def pack_y(q, span, seg=0):
    """minimap2's y word: seg_id << 48 | q_span << 32 | query position (32 bits, whatever its sign)"""
    q = np.asarray(q, np.int64) & 0xffffffff
    n = len(q)
    return (np.broadcast_to(np.asarray(seg, np.uint64), n) << np.uint64(48)) | (np.broadcast_to(np.asarray(span, np.uint64), n) << np.uint64(32)) | q.astype(np.uint64)


def diagonal(rng, n=2000, step=20, noise=25, q0=1000):
    """a noisy diagonal: x ascending, ~`step` apart (with max_dist 5000 a window holds ~5000 / step predecessors), q = x + q0 +- noise,
    spans 1 .. 60 -- many pairs pass the filters of a header with bw >= 2 * noise -> (x, q, span), int64"""
    x = np.sort(rng.integers(0, step * n, n))
    return x, x + q0 + rng.integers(-noise, noise + 1, n), rng.integers(1, 61, n)


def call(x, q, span, avg_qspan=15.0, max_dist_x=5000, max_dist_y=5000, bw=500, n_segs=1, seg=0, x_off=0):
    return (avg_qspan, max_dist_x, max_dist_y, bw, n_segs, np.asarray(x, np.int64).astype(np.uint64) + np.uint64(x_off), pack_y(q, span, seg))


def limit_cases():
    """name -> (calls, {0: forms, 1: forms}, chains): one small call per side of each limit, and a plain call beside them that
    every form takes.  chains[c]: the call's header and data let pairs through (its oracle result holds many parents); calls it is
    False for have parent -1 everywhere, and that is what the kernels have to give."""
    rng = np.random.default_rng(61)
    D = lambda **kw: diagonal(rng, **kw)
    plain = lambda: call(*D())
    cases = {}
    # q_span: 0 makes the table form ineligible (its byte 0 means "filtered"), 255 is the largest value the field holds
    x, q, s = D()
    x2, q2, s2 = D(); s2 = np.where(rng.random(len(s2)) < 0.1, 0, s2)
    x3, q3, s3 = D(); s3 = np.where(rng.random(len(s3)) < 0.1, 255, s3)
    cases["q_span_0_and_255"] = ([call(x, q, 0 * s), call(x2, q2, s2), call(x3, q3, s3), plain()], {0: [4, 4, 4, 3], 1: [4, 4, 4, 3]}, [False, True, True, True])
    # avg_qspan: 0 <= avg_qspan <= 4096 (bw = 1 keeps the gap costs, ~41 per unit of |dr - dq|, inside a byte: q = x + 0 or 1)
    a = []
    for v in (4096.0, 4097.0):
        x = D()[0]
        a.append(call(x, x + 1000 + rng.integers(0, 2, len(x)), rng.integers(1, 61, len(x)), avg_qspan=v, bw=1))
    cases["avg_qspan_4096"] = (a + [plain()], {0: [3, 4, 3], 1: [3, 4, 3]}, [True, True, True])
    # max_dist_x: 0 <= max_dist_x < 2^30
    cases["max_dist_x_2p30"] = ([call(*D(), max_dist_x=(1 << 30) - 1), call(*D(), max_dist_x=1 << 30), plain()], {0: [3, 4, 3], 1: [3, 4, 3]}, [True, True, True])
    cases["max_dist_x_neg_and_0"] = ([call(*D(), max_dist_x=-1), call(*D(), max_dist_x=0), plain()], {0: [4, 3, 3], 1: [4, 3, 3]}, [False, False, True])
    cases["max_dist_y_0_and_neg"] = ([call(*D(), max_dist_y=0), call(*D(), max_dist_y=-5), plain()], {0: [3, 3, 3], 1: [3, 3, 3]}, [False, False, True])
    # min(max_dist_x, max_dist_y) <= 2^20: the fast-chain limit of both key forms (dq - dr cannot wrap below it); chain has none
    M = 1 << 20
    cases["min_max_dist_2p20"] = ([call(*D(), max_dist_x=M, max_dist_y=M), call(*D(), max_dist_x=2 * M, max_dist_y=M + 1), call(*D(), max_dist_x=M + 1, max_dist_y=2 * M), plain()],
                                  {0: [3, 3, 3, 3], 1: [3, 4, 4, 3]}, [True, True, True, True])
    cases["bw_neg1"] = ([call(*D(), bw=-1), plain()], {0: [4, 3], 1: [4, 3]}, [False, True])
    # chain's "plain" fact: max(x) - min(x) + min(max_dist_x, max_dist_y) < 2^31 - 1 -- two clusters, the limit crossed by exactly one
    a = []
    for span in ((1 << 31) - 2 - 5000, (1 << 31) - 1 - 5000):
        x, q, s = D()
        far = x >= x[len(x) // 2]
        x = np.where(far, x - x.max() + span, x - x.min())          # min 0, max `span`; q keeps following the clusters' own diagonal
        a.append(call(x, q, s))
    cases["x_span_2p31"] = (a + [plain()], {0: [3, 4, 3], 1: [3, 3, 3]}, [True, True, True])
    # x within max_dist_x of 2^64: max(x) <= 2^64 - 1 - max_dist_x, beyond it the reference's x[st] + max_dist_x wraps
    a = []
    for room in (5000, 0):
        x, q, s = D()
        a.append(call(x - x.min(), q, s, x_off=(1 << 64) - 1 - room - int(x.max() - x.min())))
    cases["x_top_of_64_bits"] = (a + [plain()], {0: [3, 4, 3], 1: [3, 3, 3]}, [True, True, True])
    # q crosses 2^31 in mid-call: the reference holds it as int32_t
    x, q, s = D(q0=(1 << 31) - 20000)
    assert (q < 1 << 31).sum() > 500 and (q >= 1 << 31).sum() > 500
    cases["q_across_2p31"] = ([call(x, q, s), plain()], {0: [3, 3], 1: [3, 3]}, [True, True])
    # segments: MSEG comes from the header, "plain" from the data
    x, q, s = D()
    cases["n_segs_header_against_data"] = ([call(*D(), n_segs=2), call(x, q, s, n_segs=1, seg=rng.integers(0, 2, len(x))), plain()],
                                           {0: [3, 4, 3], 1: [3, 3, 3]}, [True, True, True])
    return cases


SWEEP_SPANS = tuple(range(166, 186)) + (250, 255)


def byte_limit_sweep():
    """ctab_geo keeps oc - gc + bias in a byte: the call's largest q_span + its largest gap cost + 1 <= 255.  bw = 500, avg_qspan = 15
    (largest gap cost about 80): calls whose largest q_span sweeps the range around 255 - bias, after one with spans 15 -> calls"""
    rng = np.random.default_rng(62)
    calls = []
    for v in (15,) + SWEEP_SPANS:
        x, q, s = diagonal(rng, n=1500)
        s = np.where(rng.random(len(s)) < 0.02, v, np.minimum(s, v))
        assert s.max() == v
        calls.append(call(x, q, s))
    return calls


def collinear(n, span, x0=1000):
    """x = q = x0 + i * span, spans `span`: with bw = 0 and max_dist 5000 every anchor chains to i - 1 and the last score is n * span"""
    x = x0 + span * np.arange(n, dtype=np.int64)
    return call(x, x, np.full(n, span), bw=0)


def backbone(n, span):
    """even anchors: the collinear backbone, 2 * span apart (each adds `span`: scores to n / 2 * span); odd anchors: half-way between
    two of them, 1 .. 3 beside the diagonal (filtered against the backbone by bw = 0, collinear with every third of their own kind)
    with spans 1 .. 4 -- windows twice as deep, ties between equal small chains, filtered pairs, all beside high scores"""
    i = np.arange(n, dtype=np.int64)
    x = 1000 + span * i
    odd = (i & 1) == 1
    q = np.where(odd, x + 1 + (i // 2) % 3, x)
    return call(x, q, np.where(odd, 1 + (i // 2) % 4, span), bw=0)


def top_score_cases():
    """scores at the top of the 24 bits of the key forms -> (calls, table forms for both modes, last scores of the collinear calls)"""
    calls = [collinear(65900, 254), collinear(65930, 254), collinear(65000, 255), collinear(65001, 255), backbone(65900, 254)]
    assert 65900 * 254 < TOP <= 65930 * 254 and 65000 * 255 < TOP
    return calls, [3, 4, 4, 4, None], [65900 * 254, 65930 * 254, 65000 * 255, 65001 * 255]


EDGE_LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4095, 4096, 4097)


def block_edge_calls(step=3):
    """single calls at the edges of the 64-anchor blocks and of the table form's 16-row groups, anchors ~`step` apart: windows of
    ~5000 / step predecessors reach back across many blocks"""
    rng = np.random.default_rng(63)
    return [call(*diagonal(rng, n=n, step=step)) for n in EDGE_LENGTHS]
