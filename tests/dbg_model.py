"""The rules of gab_dbg_build (include/gab.h, dbg section) in plain Python: Platypus' local assembly graph as the reference builds it
(dbg/src/debruijn.cpp: loadReferenceIntoGraph :1291-1317, loadBAMDataIntoGraph :1399-1414, loadReadIntoGraph :1351-1396,
DeBruijnGraph_AddEdge :917-949, NodeDict_FindOrInsert :759-843), and the region planner (the batch loop of main, :1576-1592, with
setWindowPointers / bisectReadsLeft, dbg/src/common.cpp:161-227).  Everything is an integer; tests/golden/make_dbg_golden.py holds
this file to the compiled reference node for node."""
import numpy as np

LETTERS = b"=ACMGRSVTWYHKDBN"          # what getRead makes of a BAM record (common.cpp:14-17); N is the only letter a read's filter knows
REF, READ = 1, 2
QC_FAIL = 512
MAX_K = 16
NODE = np.dtype([("src_read", "<i4"), ("src_off", "<i4"), ("colours", "<i4"), ("position", "<i4"), ("weight", "<i8"), ("n_edges", "<i4"),
                 ("edge_to", "<i4", 4), ("pad", "<i4"), ("edge_weight", "<i8", 4)])
assert NODE.itemsize == 80
REGION_SIZE = 1500


class Graph:
    def __init__(self):
        self.index = {}         # k bytes -> node number
        self.nodes = []         # [src_read, src_off, colours, position, weight, [[to, weight] ...]] in order of first occurrence
        self.dropped = 0        # edge occurrences that met four other successors

    def node(self, key, src, off, colour, position, weight):
        i = self.index.get(key)
        if i is None:
            self.index[key] = i = len(self.nodes)
            self.nodes.append([src, off, colour, position, weight, []])
        else:
            n = self.nodes[i]
            n[2] |= colour
            n[4] += weight
        return i

    def add_edge(self, ks, ke, src, off, colour, pos_s, pos_e, w):
        s = self.node(ks, src, off, colour, pos_s, w)
        e = self.node(ke, src, off + 1, colour, pos_e, w)         # (a second find even when ke == ks: a homopolymer counts twice)
        edges = self.nodes[s][5]
        for slot in edges:
            if slot[0] == e:
                slot[1] += w
                return
        if len(edges) < 4:
            edges.append([e, w])
        else:
            self.dropped += 1


def occurrences(length, k):
    """edge occurrences a sequence of `length` letters offers: i in 0 .. length - k - 2"""
    return max(0, length - k - 1)


def build_region(ref, ref_start, reads, k=15, min_qual=20, first_read=0, stats=None):
    """ref: bytes; reads: [(seq bytes, qual bytes or uint8 array, flag)], numbered from first_read on -> the records of the region"""
    g = Graph()
    offered = passed = 0
    for i in range(occurrences(len(ref), k)):
        g.add_edge(ref[i:i + k], ref[i + 1:i + 1 + k], -1, i, REF, ref_start + i, ref_start + i + 1, 1)
    offered += occurrences(len(ref), k); passed += occurrences(len(ref), k)
    for r, (seq, qual, flag) in enumerate(reads):
        if flag & QC_FAIL:
            continue
        qual = bytes(qual) if isinstance(qual, (bytes, bytearray)) else np.asarray(qual, np.uint8).tobytes()
        assert len(qual) == len(seq)
        for i in range(occurrences(len(seq), k)):
            offered += 1
            q = min(qual[i:i + k + 1])
            if q >= min_qual and b"N" not in seq[i:i + k + 1]:
                passed += 1
                g.add_edge(seq[i:i + k], seq[i + 1:i + 1 + k], first_read + r, i, READ, -1, -1, q)
    out = np.zeros(len(g.nodes), NODE)
    out["edge_to"] = -1
    for i, (src, off, colour, position, weight, edges) in enumerate(g.nodes):
        rec = out[i]
        rec["src_read"], rec["src_off"], rec["colours"], rec["position"], rec["weight"], rec["n_edges"] = src, off, colour, position, weight, len(edges)
        for j, (to, w) in enumerate(edges):
            rec["edge_to"][j] = to
            rec["edge_weight"][j] = w
    if stats is not None:
        stats["occurrences"] = stats.get("occurrences", 0) + offered
        stats["passed"] = stats.get("passed", 0) + passed
        stats["nodes"] = stats.get("nodes", 0) + len(g.nodes)
        stats["edges"] = stats.get("edges", 0) + int(out["n_edges"].sum())
        stats["dropped"] = stats.get("dropped", 0) + g.dropped
    return out


def build(regions, reads, k=15, min_qual=20, stats=None):
    """regions: [(ref bytes, ref_start, read_begin, read_end)]; reads: [(seq, qual, flag)] -> (node_off, records)"""
    recs = [build_region(ref, start, reads[b:e], k, min_qual, b, stats) for ref, start, b, e in regions]
    if stats is not None:
        stats["regions"] = len(regions)
    off = np.zeros(len(regions) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return off, (np.concatenate(recs) if recs else np.zeros(0, NODE))


def room(regions, reads, k=15):
    """the nodes a region can have at most, from lengths alone: a sequence with e > 0 occurrences has at most e + 1 k-mers"""
    def one(n):
        e = occurrences(n, k)
        return e + 1 if e else 0
    return np.array([one(len(ref)) + sum(one(len(reads[j][0])) for j in range(b, e) if not reads[j][2] & QC_FAIL) for ref, _, b, e in regions], np.int64)


def format_region(ref, ref_start, reads, records):
    """the line the reference prints with verbose > 0 (debruijn.cpp:1458-1465): "%d %d " of refStart twice, then "%s" of every node's
    sequence pointer -- the rest of the reference or of the read from the node's first occurrence on"""
    parts = [b"%d %d " % (ref_start, ref_start)]
    for rec in records:
        src = ref if rec["src_read"] < 0 else reads[int(rec["src_read"])][0]
        parts.append(src[int(rec["src_off"]):])
    return b"".join(parts) + b"\n"


# ---- the planner ------------------------------------------------------------------------------------------------------------------
def bisect_left(pos, x):
    lo, hi = 0, len(pos)
    while lo < hi:
        mid = (lo + hi) // 2
        if pos[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def window(pos, end, longest, start, stop):
    """setWindowPointers (common.cpp:161-194): the reads [first, last) of the window [start, stop)"""
    if len(pos) == 0:
        return 0, 0
    first = bisect_left(pos, max(1, start - longest))
    last = bisect_left(pos, stop)
    while first < len(pos) and end[first] <= start:
        first += 1
    assert first <= last, "the reference exits here: pos[] is not sorted, or a read ends before it starts"
    return first, min(last, len(pos))


def plan_regions(beg, end, pos, read_end, contig_len, size=REGION_SIZE):
    """the batch loop of main (debruijn.cpp:1576-1592): per region (start, ref_start, ref_len, read_begin, read_end).  The reference
    span is what faidx_fetch_seq returns for [ref_start, ref_end - 1]: cut at the contig's end"""
    longest = max([int(e) - int(p) for p, e in zip(pos, read_end)] + [0])
    shift = max(100, min(1000, size // 2))
    out = []
    for k in range(beg, end, shift):
        a_end = min(k + size, end)
        ref_start = max(0, k - size)
        ref_end = a_end + size
        first, last = window(pos, read_end, longest, k, a_end)
        out.append((k, ref_start, max(0, min(ref_end, contig_len) - ref_start), first, last))
    return np.array(out, np.int64).reshape(-1, 5)
