"""Host-side mirror of the adaptive banded event alignment, align() (abea/src/align.c:169-548), over the C ABI
(include/gab.h: gab_abea_align, gab_abea_align_device): the loop of align_db over its reads (abea/src/f5c.c:1367-1394) as one call;
and of the two steps before it, event detection and the scaling estimate (gab_abea_events, gab_abea_scalings: event_single,
f5c.c:1241-1264), so that raw samples go in and aligned pairs come out (EventAligner.signal_to_pairs); and of the block after it,
postalign, recalibrate_model and the read checks (gab_abea_calibrate: f5c.c:1438-1501), so that calibrated reads with their
base-to-event map come out (EventAligner.signal_to_calibrated); and of the step after that, realign_read (gab_abea_realign:
f5c.c:1508-1515), which turns a calibrated read, its reference substring and its CIGAR into the event alignment records of
eventalign (EventAligner.realign, eventalign_rows); and of the other branch of the same step, calculate_methylation_for_read
(gab_abea_meth: f5c.c:1397-1411), which scores every CpG group of a calibrated read, plain and methylated, against a CpG model
(EventAligner.set_cpg_model, call_methylation, methylation_rows)."""
import ctypes as C

import numpy as np

from ._lib import check, lib

K = 6             # GAB_ABEA_K
BANDWIDTH = 100   # GAB_ABEA_BANDWIDTH
NKMER = 4096      # GAB_ABEA_NKMER
LOW_EMISSION, NOT_SPANNED, GAP, NO_END = 1, 2, 4, 8      # gab_abea_read.flags
ERANGE = -34      # GAB_ERANGE

PAIR = np.dtype([("ref_pos", np.int32), ("read_pos", np.int32)])
READ = np.dtype([("n_pairs", np.int32), ("path_len", np.int32), ("end_event", np.int32), ("max_gap", np.int32), ("flags", np.uint32),
                 ("pad", np.int32), ("avg_log_emission", np.float64), ("fills", np.int64)])      # gab_abea_read, 40 bytes
FAILED_CALIBRATION, FAILED_ALIGNMENT, FAILED_QUALITY_CHK = 1, 2, 4      # gab_abea_calib.read_stat_flag
RANGE = np.dtype([("start", np.int32), ("stop", np.int32)])      # gab_abea_range: stop inclusive, -1 / -1 = no event
CALIB = np.dtype([("n_alignment", np.int32), ("n_m_state", np.int32), ("read_stat_flag", np.uint32), ("recalibrated", np.int32),
                  ("scale", np.float32), ("shift", np.float32), ("var", np.float32), ("log_var", np.float32),
                  ("events_per_base", np.float64)])                  # gab_abea_calib, 40 bytes
REALIGN_SKIPPED, REALIGN_NO_PAIRS, REALIGN_NO_EVENT, REALIGN_STRAND = 1, 2, 4, 8      # gab_abea_realign_read.flags
EALN = np.dtype([("ref_position", np.int32), ("event_idx", np.int32), ("hmm_state", np.uint8), ("pad", np.uint8, 3)])      # gab_abea_ealn, 12 bytes
REALIGN = np.dtype([("n_entries", np.int32), ("hmm_segments", np.int32), ("max_rows", np.int32), ("flags", np.uint32), ("cells", np.int64)])      # gab_abea_realign_read
CIGAR_OPS = "MIDNSHP=X"
NKMER_CPG = 15625     # GAB_ABEA_METH_NKMER: k-mers over A C G M T
LOGSUM_TBL = 16000    # GAB_ABEA_METH_LOGSUM
METH_SKIPPED, METH_NO_EVENT, METH_STRAND, METH_TRANSITIONS = 1, 2, 4, 8      # gab_abea_meth_read.flags
SITE = np.dtype([("start_position", np.int32), ("end_position", np.int32), ("n_cpg", np.int32), ("first_cpg", np.int32), ("event_start", np.int32),
                 ("event_stop", np.int32), ("ll_unmethylated", np.float32), ("ll_methylated", np.float32)])      # gab_abea_site, 32 bytes
METH = np.dtype([("n_sites", np.int32), ("groups", np.int32), ("skipped_start", np.int32), ("skipped_span", np.int32), ("skipped_unbounded", np.int32),
                 ("skipped_short", np.int32), ("flags", np.uint32), ("pad", np.int32), ("cells", np.int64)])      # gab_abea_meth_read, 40 bytes
assert SITE.itemsize == 32 and METH.itemsize == 40
assert PAIR.itemsize == 8 and READ.itemsize == 40 and RANGE.itemsize == 8 and CALIB.itemsize == 40 and EALN.itemsize == 12 and REALIGN.itemsize == 24


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_reads(reads):
    """list of (bases bytes, event means, scale, shift) -> the packed arrays of align(): seq, seq_off, seq_len, events, event_off,
    n_events, scale, shift, pair_off (n_events + n_kmers pairs of room per read, back to back)"""
    seq_len = np.array([len(r[0]) for r in reads], np.int32)
    n_events = np.array([len(r[1]) for r in reads], np.int32)
    seq_off = np.zeros(len(reads), np.int64); event_off = np.zeros(len(reads), np.int64); pair_off = np.zeros(len(reads), np.int64)
    if len(reads) > 1:
        seq_off[1:] = np.cumsum(seq_len[:-1], dtype=np.int64)
        event_off[1:] = np.cumsum(n_events[:-1], dtype=np.int64)
        pair_off[1:] = np.cumsum((n_events.astype(np.int64) + seq_len - K + 1)[:-1])
    seq = np.frombuffer(b"".join(bytes(r[0]) for r in reads), np.uint8).copy() if reads else np.zeros(0, np.uint8)
    events = np.concatenate([np.asarray(r[1], np.float32) for r in reads]) if reads else np.zeros(0, np.float32)
    scale = np.array([r[2] for r in reads], np.float32); shift = np.array([r[3] for r in reads], np.float32)
    return seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pair_off


def events_shape():
    """(chunk, warm-up) in samples of the speculative peak detector: GAB_ABEA_EVENTS_CHUNK, GAB_ABEA_EVENTS_WARMUP"""
    chunk = C.c_int32(0); warmup = C.c_int32(0)
    check(lib().gab_abea_events_shape(C.byref(chunk), C.byref(warmup)))
    return chunk.value, warmup.value


def pack_signals(signals):
    """list of (raw samples, range, digitisation, offset) -> raw, raw_off, n_samples, range, digitisation, offset"""
    n_samples = np.array([np.size(s[0]) for s in signals], np.int32)
    raw_off = np.zeros(len(signals), np.int64)
    if len(signals) > 1:
        raw_off[1:] = np.cumsum(n_samples[:-1], dtype=np.int64)
    raw = np.concatenate([np.asarray(s[0], np.float32).reshape(-1) for s in signals]) if signals else np.zeros(0, np.float32)
    par = [np.array([s[t] for s in signals], np.float32) for t in (1, 2, 3)]
    return raw, raw_off, n_samples, par[0], par[1], par[2]


def pair_room(seq_len, n_events):
    """pairs of room a read needs at its pair_off: n_events + n_kmers"""
    return np.asarray(n_events, np.int64) + np.asarray(seq_len, np.int64) - K + 1


def realign_shape():
    """rows of a wavefront's backpointer trace: GAB_ABEA_REALIGN_ROWS as the library was built"""
    rows = C.c_int32(0)
    check(lib().gab_abea_realign_shape(C.byref(rows)))
    return rows.value


def realign_room(n_events, cigar, cigar_off, n_cigar):
    """entries of room a read needs at its out_off: n_events * (1 + its number of N operations)"""
    cigar = np.asarray(cigar, np.uint32)
    skips = np.array([int(((cigar[o:o + k] & 15) == 3).sum()) for o, k in zip(cigar_off, n_cigar)], np.int64)
    return np.asarray(n_events, np.int64) * (1 + skips)


def meth_shape():
    """(k-mer blocks a lane of the methylation scoring kernel owns in a wide group, k-mers up to which a group runs with one block a
    lane): GAB_ABEA_METH_BLOCKS_PER_LANE, GAB_ABEA_METH_ONE_BLOCK_KMERS as the library was built"""
    v = C.c_int32(0); w = C.c_int32(0)
    check(lib().gab_abea_meth_shape(C.byref(v), C.byref(w)))
    return v.value, w.value


def meth_logsum():
    """the 16000 floats of the logsum table as the library builds them (no GPU needed)"""
    t = np.zeros(LOGSUM_TBL, np.float32)
    check(lib().gab_abea_meth_logsum(_p(t)))
    return t


def meth_room(ref, ref_off, ref_len):
    """site records of room a read needs at its out_off: the CpG groups of its prepared reference (gab_abea_meth_groups, no GPU needed)"""
    ref = np.ascontiguousarray(ref, np.uint8); ref_off = np.ascontiguousarray(ref_off, np.int64); ref_len = np.ascontiguousarray(ref_len, np.int32)
    groups = np.zeros(ref_len.size, np.int32)
    check(lib().gab_abea_meth_groups(_p(ref), _p(ref_off), _p(ref_len), C.c_int64(ref_len.size), _p(groups)))
    return groups.astype(np.int64)


_FIRST_BASE = bytes.maketrans(b"ACGTMRWSYKVHDBN", b"ACGTAAACCGAAACA")
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def eventalign_rows(ref, ref_pos, is_rev, entries):
    """one read's reference bases (as given to realign), position, strand and EALN entries -> per entry (position, reference_kmer,
    event_index, model_kmer, hmm_state), the columns of events.tsv that the suite's check reads.  reference_kmer is the six
    upper-cased, disambiguated reference bases at the position; model_kmer is NNNNNN for a 'B', otherwise that k-mer, reverse-
    complemented for a reverse read (eventalign.c:1474, 1486-1503)."""
    seq = bytes(ref).upper().translate(_FIRST_BASE)
    rows = []
    for e in entries:
        at = int(e["ref_position"]) - int(ref_pos)
        kmer = seq[at:at + K]
        state = chr(int(e["hmm_state"]))
        model = b"N" * K if state == "B" else kmer.translate(_COMPLEMENT)[::-1] if is_rev else kmer
        rows.append((int(e["ref_position"]), kmer.decode(), int(e["event_idx"]), model.decode(), state))
    return rows


def pack_aligned_reads(reads):
    """list of (reference bases, ref_pos, is_rev, cigar as uint32 in BAM encoding, seq_len, event means, map as (n_kmers, 2) or RANGE,
    calibration record) -> the packed arrays that realign() and call_methylation() take, in their order"""
    def offsets(lens):
        o = np.zeros(len(lens), np.int64)
        if len(lens) > 1:
            o[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        return o
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt)
    ref_len = np.array([len(r[0]) for r in reads], np.int32); n_cigar = np.array([len(r[3]) for r in reads], np.int32)
    seq_len = np.array([r[4] for r in reads], np.int32); n_events = np.array([len(r[5]) for r in reads], np.int32)
    maps = [np.ascontiguousarray(r[6] if np.asarray(r[6]).dtype == RANGE else np.asarray(r[6], np.int32)).view(np.int32).reshape(-1, 2) for r in reads]
    calib = np.zeros(len(reads), CALIB)
    for i, r in enumerate(reads):
        for f in CALIB.names:
            calib[i][f] = r[7][f] if not isinstance(r[7], np.void) or f in r[7].dtype.names else 0
    return (cat([np.frombuffer(bytes(r[0]), np.uint8) for r in reads], np.uint8), offsets(ref_len), ref_len, np.array([r[1] for r in reads], np.int32),
            np.array([r[2] for r in reads], np.uint8), cat([r[3] for r in reads], np.uint32), offsets(n_cigar), n_cigar, seq_len,
            cat([r[5] for r in reads], np.float32), offsets(n_events), n_events, cat(maps, np.int32).view(RANGE),
            offsets(np.array([len(m) for m in maps], np.int64)), calib)


def methylation_rows(contig, qname, ref, ref_pos, sites):
    """one read's reference bases (as given to call_methylation), position and SITE records -> the text lines of call-methylation in
    output version 1 (f5c.c:1746-1753): contig, start, end, read name, %.2lf of ll_methylated - ll_unmethylated, of ll_methylated and
    of ll_unmethylated as doubles, strands scored (1), CpGs in the group, and the prepared reference from five bases before the first
    CpG to six behind the start of the last (meth.c:639-643)"""
    seq = bytes(ref).upper().translate(_FIRST_BASE)
    rows = []
    for s in sites:
        m, u = float(s["ll_methylated"]), float(s["ll_unmethylated"])
        a = int(s["first_cpg"]); b = a + int(s["end_position"]) - int(s["start_position"])
        rows.append("%s\t%d\t%d\t%s\t%.2f\t%.2f\t%.2f\t%d\t%d\t%s" % (contig, s["start_position"], s["end_position"], qname, m - u, m, u, 1, s["n_cpg"],
                                                                         seq[a - K + 1:b + K].decode()))
    return rows


class EventAligner:
    """one pore model (4096 k-mer entries: level_mean, level_stdv, optionally level_log_stdv) on one GPU"""

    def __init__(self, level_mean, level_stdv, level_log_stdv=None, device=0):
        self._h = C.c_void_p()
        mean = np.ascontiguousarray(level_mean, np.float32); stdv = np.ascontiguousarray(level_stdv, np.float32)
        if mean.size != NKMER or stdv.size != NKMER or (level_log_stdv is not None and np.size(level_log_stdv) != NKMER):
            raise ValueError(f"the pore model has {NKMER} entries")
        lstd = None if level_log_stdv is None else np.ascontiguousarray(level_log_stdv, np.float32)
        check(lib().gab_abea_create(C.c_int(device), _p(mean), _p(stdv), _p(lstd) if lstd is not None else None, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().gab_abea_destroy(self._h)
            self._h = None

    __del__ = close

    def reserve(self, max_reads, max_bases, max_events):
        check(lib().gab_abea_reserve(self._h, C.c_int64(max_reads), C.c_int64(max_bases), C.c_int64(max_events)))

    def align(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pair_off=None):
        """numpy arrays (pack_reads gives them) -> (pairs, pair_off, records): pairs a PAIR array in which read i's path is
        pairs[pair_off[i] : pair_off[i] + records[i]["path_len"]], records a READ array"""
        seq = np.ascontiguousarray(seq, np.uint8); events = np.ascontiguousarray(events, np.float32)
        seq_off = np.ascontiguousarray(seq_off, np.int64); event_off = np.ascontiguousarray(event_off, np.int64)
        seq_len = np.ascontiguousarray(seq_len, np.int32); n_events = np.ascontiguousarray(n_events, np.int32)
        scale = np.ascontiguousarray(scale, np.float32); shift = np.ascontiguousarray(shift, np.float32)
        n = seq_len.size
        room = pair_room(seq_len, n_events)
        if pair_off is None:
            pair_off = np.zeros(n, np.int64)
            if n > 1:
                pair_off[1:] = np.cumsum(room[:-1])
        pair_off = np.ascontiguousarray(pair_off, np.int64)
        total = int((pair_off + np.maximum(room, 0)).max()) if n else 0
        pairs = np.full(max(total, 0), -1, np.int32).repeat(2).view(PAIR)
        res = np.zeros(n, READ)
        check(lib().gab_abea_align(self._h, _p(seq), _p(seq_off), _p(seq_len), _p(events), _p(event_off), _p(n_events), _p(scale), _p(shift),
                                   C.c_int64(n), _p(pairs), _p(pair_off), _p(res)))
        return pairs, pair_off, res

    def align_reads(self, reads):
        """list of (bases, event means, scale, shift) -> (pairs, pair_off, records)"""
        return self.align(*pack_reads(reads))

    def align_device(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, res, stream=0):
        """torch tensors on the handle's GPU: uint8, int64, int32, float32, int64, int32, float32, float32; pairs an int32 tensor of
        shape (room, 2) and res a uint8 tensor of 40 bytes per read, both filled in place (complete when the call returns)"""
        n = seq_len.numel()
        if pairs.numel() % 2 or res.numel() * res.element_size() < n * READ.itemsize:
            raise ValueError("pairs holds (ref_pos, read_pos) int32 pairs, res 40 bytes per read")
        check(lib().gab_abea_align_device(
            self._h, C.c_void_p(seq.data_ptr()), C.c_int64(seq.numel()), C.c_void_p(seq_off.data_ptr()), C.c_void_p(seq_len.data_ptr()),
            C.c_void_p(events.data_ptr()), C.c_int64(events.numel()), C.c_void_p(event_off.data_ptr()), C.c_void_p(n_events.data_ptr()),
            C.c_void_p(scale.data_ptr()), C.c_void_p(shift.data_ptr()), C.c_int64(n), C.c_void_p(pairs.data_ptr()), C.c_int64(pairs.numel() // 2),
            C.c_void_p(pair_off.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(stream)))

    # ---- event detection and the scaling estimate (gab_abea_events, gab_abea_scalings) ----------------------------------------
    def events(self, raw, raw_off, n_samples, rng, digitisation, offset, event_cap=None, slabs=None):
        """packed numpy arrays (pack_signals gives them) -> (rc, n_events, event_off, total, mean, stdv, start, length); rc is 0, or
        ERANGE when the events do not fit event_cap (default: one per sample, always enough) -- the counts are valid then and the
        slabs untouched.  slabs: four arrays (mean, stdv, start, length) to write into instead of new ones."""
        raw = np.ascontiguousarray(raw, np.float32); raw_off = np.ascontiguousarray(raw_off, np.int64)
        n_samples = np.ascontiguousarray(n_samples, np.int32)
        rng = np.ascontiguousarray(rng, np.float32); digitisation = np.ascontiguousarray(digitisation, np.float32)
        offset = np.ascontiguousarray(offset, np.float32)
        n = n_samples.size
        if event_cap is None:
            event_cap = int(np.maximum(n_samples, 0).sum())
        if slabs is None:
            slabs = (np.zeros(event_cap, np.float32), np.zeros(event_cap, np.float32), np.zeros(event_cap, np.int32), np.zeros(event_cap, np.float32))
        mean, stdv, start, length = slabs
        if not (mean.dtype == stdv.dtype == length.dtype == np.float32 and start.dtype == np.int32) or min(a.size for a in slabs) < event_cap:
            raise ValueError("slabs: float32, float32, int32, float32 arrays of event_cap entries at least")
        n_events = np.zeros(n, np.int32); event_off = np.zeros(n, np.int64); total = C.c_int64(0)
        rc = lib().gab_abea_events(self._h, _p(raw), _p(raw_off), _p(n_samples), _p(rng), _p(digitisation), _p(offset), C.c_int64(n),
                                   _p(n_events), _p(event_off), _p(mean), _p(stdv), _p(start), _p(length), C.c_int64(event_cap), C.byref(total))
        if rc not in (0, ERANGE):
            check(rc)
        return rc, n_events, event_off, total.value, mean, stdv, start, length

    def detect_events(self, signals):
        """list of (raw samples, range, digitisation, offset) -> per read a dict of its event table: mean, stdv, start, length"""
        rc, n_events, event_off, _, mean, stdv, start, length = self.events(*pack_signals(signals))
        check(rc)
        return [dict(mean=mean[o:o + k], stdv=stdv[o:o + k], start=start[o:o + k], length=length[o:o + k]) for o, k in zip(event_off, n_events)]

    def detect_events_device(self, raw, raw_off, n_samples, rng, digitisation, offset, n_events, event_off, mean, stdv, start, length, total, stream=0,
                             event_cap=None):
        """torch tensors on the handle's GPU: float32, int64, int32, float32 x 3 in; int32 n_events, int64 event_off, the four slabs
        (float32, float32, int32, float32; their room, or event_cap if that is less) and a one-element int64 `total` out.
        -> 0 or ERANGE"""
        cap = min(mean.numel(), stdv.numel(), start.numel(), length.numel())
        cap = cap if event_cap is None else min(cap, int(event_cap))
        rc = lib().gab_abea_events_device(
            self._h, C.c_void_p(raw.data_ptr()), C.c_int64(raw.numel()), C.c_void_p(raw_off.data_ptr()), C.c_void_p(n_samples.data_ptr()),
            C.c_void_p(rng.data_ptr()), C.c_void_p(digitisation.data_ptr()), C.c_void_p(offset.data_ptr()), C.c_int64(n_samples.numel()),
            C.c_void_p(n_events.data_ptr()), C.c_void_p(event_off.data_ptr()), C.c_void_p(mean.data_ptr()), C.c_void_p(stdv.data_ptr()),
            C.c_void_p(start.data_ptr()), C.c_void_p(length.data_ptr()), C.c_int64(cap), C.c_void_p(total.data_ptr()), C.c_void_p(stream))
        if rc not in (0, ERANGE):
            check(rc)
        return rc

    def scalings(self, seq, seq_off, seq_len, events, event_off, n_events):
        """packed numpy arrays -> (scale, shift), float32 per read"""
        seq = np.ascontiguousarray(seq, np.uint8); events = np.ascontiguousarray(events, np.float32)
        seq_off = np.ascontiguousarray(seq_off, np.int64); event_off = np.ascontiguousarray(event_off, np.int64)
        seq_len = np.ascontiguousarray(seq_len, np.int32); n_events = np.ascontiguousarray(n_events, np.int32)
        n = seq_len.size
        scale = np.zeros(n, np.float32); shift = np.zeros(n, np.float32)
        check(lib().gab_abea_scalings(self._h, _p(seq), _p(seq_off), _p(seq_len), _p(events), _p(event_off), _p(n_events), C.c_int64(n), _p(scale), _p(shift)))
        return scale, shift

    def scalings_last_stats(self):
        """the last scalings call: reads, and those whose event sum / k-mer level sum / sum of squared levels was added in order"""
        v = [C.c_int64(-1) for _ in range(4)]
        check(lib().gab_abea_scalings_last_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("reads", "event_sums_in_order", "kmer_sums_in_order", "kmer_sq_sums_in_order"), (x.value for x in v)))

    def estimate_scalings(self, reads):
        """list of (bases, event means) -> (scale, shift) by the method of moments against the handle's pore model"""
        packed = pack_reads([(r[0], r[1], 0.0, 0.0) for r in reads])
        return self.scalings(*packed[:6])

    def estimate_scalings_device(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, stream=0):
        """torch tensors on the handle's GPU: uint8, int64, int32, float32, int64, int32 in; float32 scale and shift out"""
        check(lib().gab_abea_scalings_device(
            self._h, C.c_void_p(seq.data_ptr()), C.c_int64(seq.numel()), C.c_void_p(seq_off.data_ptr()), C.c_void_p(seq_len.data_ptr()),
            C.c_void_p(events.data_ptr()), C.c_int64(events.numel()), C.c_void_p(event_off.data_ptr()), C.c_void_p(n_events.data_ptr()),
            C.c_int64(seq_len.numel()), C.c_void_p(scale.data_ptr()), C.c_void_p(shift.data_ptr()), C.c_void_p(stream)))

    def signal_to_pairs(self, signals, seqs):
        """signals: list of (raw samples, range, digitisation, offset); seqs: the reads' bases.  Events, then scalings, then the
        alignment, on device buffers: only n_events comes to the host in between (the room of the pairs depends on it).
        -> (pairs, pair_off, records, n_events, scale, shift) as numpy arrays"""
        import torch
        packed = pack_signals(signals)
        n = len(signals)
        dev = [torch.from_numpy(a).cuda() for a in packed]
        cap = max(int(packed[2].sum()), 1)
        n_events = torch.zeros(n, dtype=torch.int32, device="cuda"); event_off = torch.zeros(n, dtype=torch.int64, device="cuda")
        mean = torch.empty(cap, dtype=torch.float32, device="cuda"); stdv = torch.empty_like(mean); length = torch.empty_like(mean)
        start = torch.empty(cap, dtype=torch.int32, device="cuda"); total = torch.zeros(1, dtype=torch.int64, device="cuda")
        check(self.detect_events_device(*dev, n_events, event_off, mean, stdv, start, length, total))
        ne = n_events.cpu().numpy()
        seq_len = np.array([len(s) for s in seqs], np.int32)
        seq_off = np.zeros(n, np.int64); pair_off = np.zeros(n, np.int64)
        room = pair_room(seq_len, ne)
        if n > 1:
            seq_off[1:] = np.cumsum(seq_len[:-1], dtype=np.int64); pair_off[1:] = np.cumsum(room[:-1])
        seq = np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8).copy()
        d_seq, d_so, d_sl, d_po = (torch.from_numpy(a).cuda() for a in (seq, seq_off, seq_len, pair_off))
        scale = torch.zeros(n, dtype=torch.float32, device="cuda"); shift = torch.zeros_like(scale)
        self.estimate_scalings_device(d_seq, d_so, d_sl, mean, event_off, n_events, scale, shift)
        pairs = torch.full((max(int(room.sum()), 1), 2), -1, dtype=torch.int32, device="cuda")
        res = torch.zeros(n * READ.itemsize, dtype=torch.uint8, device="cuda")
        self.align_device(d_seq, d_so, d_sl, mean, event_off, n_events, scale, shift, pairs, d_po, res)
        return (pairs.cpu().numpy().reshape(-1).view(PAIR), pair_off, res.cpu().numpy().view(READ), ne, scale.cpu().numpy(), shift.cpu().numpy())

    # ---- base-to-event map, recalibration and read checks (gab_abea_calibrate) ---------------------------------------------------
    def calibrate(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, n_pairs, map_off=None, out=None):
        """the packed arrays of align(), its pairs (a PAIR array or an int32 array of shape (n, 2)), pair_off and the n_pairs of its
        records -> (map, map_off, records): map a RANGE array in which read i's seq_len[i] - 5 entries start at map_off[i] (back to
        back unless map_off is given), records a CALIB array.  out: (map, records) to write into instead of new arrays."""
        seq = np.ascontiguousarray(seq, np.uint8); events = np.ascontiguousarray(events, np.float32)
        seq_off = np.ascontiguousarray(seq_off, np.int64); event_off = np.ascontiguousarray(event_off, np.int64)
        seq_len = np.ascontiguousarray(seq_len, np.int32); n_events = np.ascontiguousarray(n_events, np.int32)
        scale = np.ascontiguousarray(scale, np.float32); shift = np.ascontiguousarray(shift, np.float32)
        pairs = np.asarray(pairs)
        pairs = np.ascontiguousarray(pairs if pairs.dtype == PAIR else pairs.astype(np.int32))
        pair_off = np.ascontiguousarray(pair_off, np.int64); n_pairs = np.ascontiguousarray(n_pairs, np.int32)
        n = seq_len.size
        n_kmers = np.maximum(seq_len.astype(np.int64) - K + 1, 0)
        if map_off is None:
            map_off = np.zeros(n, np.int64)
            if n > 1:
                map_off[1:] = np.cumsum(n_kmers[:-1])
        map_off = np.ascontiguousarray(map_off, np.int64)
        if out is None:
            total = int((map_off + n_kmers).max()) if n else 0
            out = (np.full(total, -1, np.int32).repeat(2).view(RANGE), np.zeros(n, CALIB))
        rmap, res = out
        if rmap.dtype != RANGE or res.dtype != CALIB or res.size < n or (n and rmap.size < int((map_off + n_kmers).max())):
            raise ValueError("out: a RANGE array with room for every read's map and a CALIB array of one record per read")
        check(lib().gab_abea_calibrate(self._h, _p(seq), _p(seq_off), _p(seq_len), _p(events), _p(event_off), _p(n_events), _p(scale), _p(shift),
                                       _p(pairs), _p(pair_off), _p(n_pairs), C.c_int64(n), _p(rmap), _p(map_off), _p(res)))
        return rmap, map_off, res

    def calibrate_reads(self, reads, paths):
        """reads: list of (bases, event means, scale, shift); paths: per read the pairs of its alignment, (n, 2) of (ref_pos,
        read_pos), empty for a read that align() failed -> (map, map_off, records)"""
        n_pairs = np.array([len(p) for p in paths], np.int32)
        pair_off = np.zeros(len(paths), np.int64)
        if len(paths) > 1:
            pair_off[1:] = np.cumsum(n_pairs[:-1], dtype=np.int64)
        flat = np.concatenate([np.asarray(p, np.int32).reshape(-1, 2) for p in paths]) if paths else np.zeros((0, 2), np.int32)
        return self.calibrate(*pack_reads(reads)[:8], flat, pair_off, n_pairs)

    def calibrate_device(self, seq, seq_off, seq_len, events, event_off, n_events, scale, shift, pairs, pair_off, n_pairs, rmap, map_off, res, stream=0):
        """torch tensors on the handle's GPU: the inputs and the pairs of align_device, int32 n_pairs; rmap an int32 tensor of shape
        (entries, 2) and res a uint8 tensor of 40 bytes per read, both filled in place (complete when the call returns)"""
        n = seq_len.numel()
        if pairs.numel() % 2 or rmap.numel() % 2 or res.numel() * res.element_size() < n * CALIB.itemsize:
            raise ValueError("pairs and rmap hold int32 pairs, res 40 bytes per read")
        check(lib().gab_abea_calibrate_device(
            self._h, C.c_void_p(seq.data_ptr()), C.c_int64(seq.numel()), C.c_void_p(seq_off.data_ptr()), C.c_void_p(seq_len.data_ptr()),
            C.c_void_p(events.data_ptr()), C.c_int64(events.numel()), C.c_void_p(event_off.data_ptr()), C.c_void_p(n_events.data_ptr()),
            C.c_void_p(scale.data_ptr()), C.c_void_p(shift.data_ptr()), C.c_void_p(pairs.data_ptr()), C.c_int64(pairs.numel() // 2),
            C.c_void_p(pair_off.data_ptr()), C.c_void_p(n_pairs.data_ptr()), C.c_int64(n), C.c_void_p(rmap.data_ptr()), C.c_int64(rmap.numel() // 2),
            C.c_void_p(map_off.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(stream)))

    def calibrate_last_stats(self):
        """the last calibrate call: reads, reads recalibrated, 'M' entries of all reads, device time of its check, map and fit
        kernels and of the whole call (ms)"""
        v = [C.c_int64(-1) for _ in range(3)]; kms = C.c_float(-1); tms = C.c_float(-1)
        check(lib().gab_abea_calibrate_last_stats(self._h, *[C.byref(x) for x in v], C.byref(kms), C.byref(tms)))
        return {"reads": v[0].value, "recalibrated": v[1].value, "m_states": v[2].value, "kernel_ms": kms.value, "total_ms": tms.value}

    def signal_to_calibrated(self, signals, seqs):
        """signal_to_pairs' three steps and then the calibration, everything resident: raw samples go in, calibrated reads with
        their base-to-event map come out.  Only n_events comes to the host in between.
        -> (map, map_off, calibration records, pairs, pair_off, alignment records, n_events) as numpy arrays"""
        import torch
        packed = pack_signals(signals)
        n = len(signals)
        dev = [torch.from_numpy(a).cuda() for a in packed]
        cap = max(int(packed[2].sum()), 1)
        n_events = torch.zeros(n, dtype=torch.int32, device="cuda"); event_off = torch.zeros(n, dtype=torch.int64, device="cuda")
        mean = torch.empty(cap, dtype=torch.float32, device="cuda"); stdv = torch.empty_like(mean); length = torch.empty_like(mean)
        start = torch.empty(cap, dtype=torch.int32, device="cuda"); total = torch.zeros(1, dtype=torch.int64, device="cuda")
        check(self.detect_events_device(*dev, n_events, event_off, mean, stdv, start, length, total))
        ne = n_events.cpu().numpy()
        seq_len = np.array([len(s) for s in seqs], np.int32)
        seq_off = np.zeros(n, np.int64); pair_off = np.zeros(n, np.int64); map_off = np.zeros(n, np.int64)
        room = pair_room(seq_len, ne)
        n_kmers = seq_len.astype(np.int64) - K + 1
        if n > 1:
            seq_off[1:] = np.cumsum(seq_len[:-1], dtype=np.int64); pair_off[1:] = np.cumsum(room[:-1]); map_off[1:] = np.cumsum(n_kmers[:-1])
        seq = np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8).copy()
        d_seq, d_so, d_sl, d_po, d_mo = (torch.from_numpy(a).cuda() for a in (seq, seq_off, seq_len, pair_off, map_off))
        scale = torch.zeros(n, dtype=torch.float32, device="cuda"); shift = torch.zeros_like(scale)
        self.estimate_scalings_device(d_seq, d_so, d_sl, mean, event_off, n_events, scale, shift)
        pairs = torch.full((max(int(room.sum()), 1), 2), -1, dtype=torch.int32, device="cuda")
        res = torch.zeros(n * READ.itemsize, dtype=torch.uint8, device="cuda")
        self.align_device(d_seq, d_so, d_sl, mean, event_off, n_events, scale, shift, pairs, d_po, res)
        n_pairs = res.view(torch.int32).view(n, READ.itemsize // 4)[:, 0].contiguous()      # gab_abea_read.n_pairs
        rmap = torch.full((max(int(n_kmers.sum()), 1), 2), -1, dtype=torch.int32, device="cuda")
        cal = torch.zeros(n * CALIB.itemsize, dtype=torch.uint8, device="cuda")
        self.calibrate_device(d_seq, d_so, d_sl, mean, event_off, n_events, scale, shift, pairs, d_po, n_pairs, rmap, d_mo, cal)
        return (rmap.cpu().numpy().reshape(-1).view(RANGE), map_off, cal.cpu().numpy().view(CALIB),
                pairs.cpu().numpy().reshape(-1).view(PAIR), pair_off, res.cpu().numpy().view(READ), ne)

    # ---- realign_read: the event alignment records (gab_abea_realign) ---------------------------------------------------------------
    def realign(self, ref, ref_off, ref_len, ref_pos, is_rev, cigar, cigar_off, n_cigar, seq_len, events, event_off, n_events, rmap, map_off, calib,
                region=(-1, -1), out_off=None, out=None):
        """packed numpy arrays: the reference bases of every read (uint8), where they start and how many, the position of the first,
        the strand, the CIGARs in BAM encoding (uint32) with offsets and counts, and seq_len, the events, the map (RANGE) and the
        calibration records (CALIB) as calibrate() returned them -> (entries, out_off, records): entries an EALN array in which read
        i's are entries[out_off[i] : out_off[i] + records[i]["n_entries"]], records a REALIGN array.  out: (entries, records) to
        write into instead of new arrays."""
        ref = np.ascontiguousarray(ref, np.uint8); cigar = np.ascontiguousarray(cigar, np.uint32); events = np.ascontiguousarray(events, np.float32)
        ref_off = np.ascontiguousarray(ref_off, np.int64); cigar_off = np.ascontiguousarray(cigar_off, np.int64)
        event_off = np.ascontiguousarray(event_off, np.int64); map_off = np.ascontiguousarray(map_off, np.int64)
        ref_len = np.ascontiguousarray(ref_len, np.int32); ref_pos = np.ascontiguousarray(ref_pos, np.int32); n_cigar = np.ascontiguousarray(n_cigar, np.int32)
        seq_len = np.ascontiguousarray(seq_len, np.int32); n_events = np.ascontiguousarray(n_events, np.int32)
        is_rev = np.ascontiguousarray(is_rev, np.uint8)
        rmap = np.ascontiguousarray(rmap); calib = np.ascontiguousarray(calib)
        if rmap.dtype != RANGE or calib.dtype != CALIB:
            raise ValueError("rmap is a RANGE array, calib a CALIB array")
        n = seq_len.size
        room = realign_room(np.maximum(n_events, 0), cigar, cigar_off, n_cigar) if n else np.zeros(0, np.int64)
        if out_off is None:
            out_off = np.zeros(n, np.int64)
            if n > 1:
                out_off[1:] = np.cumsum(room[:-1])
        out_off = np.ascontiguousarray(out_off, np.int64)
        if out is None:
            out = (np.zeros(int((out_off + room).max()) if n else 0, EALN), np.zeros(n, REALIGN))
        entries, res = out
        if entries.dtype != EALN or res.dtype != REALIGN or res.size < n:
            raise ValueError("out: an EALN array and a REALIGN array of one record per read")
        check(lib().gab_abea_realign(self._h, _p(ref), _p(ref_off), _p(ref_len), _p(ref_pos), _p(is_rev), _p(cigar), _p(cigar_off), _p(n_cigar), _p(seq_len),
                                     _p(events), _p(event_off), _p(n_events), _p(rmap), _p(map_off), _p(calib), C.c_int32(region[0]), C.c_int32(region[1]),
                                     C.c_int64(n), _p(entries), _p(out_off), _p(res)))
        return entries, out_off, res

    def realign_reads(self, reads, region=(-1, -1)):
        """list of (reference bases, ref_pos, is_rev, cigar as uint32 in BAM encoding, seq_len, event means, map as (n_kmers, 2) or
        RANGE, calibration record) -> (entries, out_off, records)"""
        return self.realign(*pack_aligned_reads(reads), region)

    def realign_device(self, ref, ref_off, ref_len, ref_pos, is_rev, cigar, cigar_off, n_cigar, seq_len, events, event_off, n_events, rmap, map_off, calib,
                       out, out_off, res, region=(-1, -1), stream=0):
        """torch tensors on the handle's GPU: uint8, int64, int32, int32, uint8 | int32 (the uint32 CIGAR words), int64, int32 | int32 |
        float32, int64, int32 | rmap an int32 tensor of shape (entries, 2) and calib a uint8 tensor of 40 bytes per read, both as
        calibrate_device filled them | out a uint8 tensor of 12 bytes per entry, int64 out_off and res a uint8 tensor of 24 bytes per
        read, filled in place (complete when the call returns)"""
        n = seq_len.numel()
        if rmap.numel() % 2 or calib.numel() * calib.element_size() < n * CALIB.itemsize or res.numel() * res.element_size() < n * REALIGN.itemsize:
            raise ValueError("rmap holds int32 pairs, calib 40 bytes and res 24 bytes per read")
        check(lib().gab_abea_realign_device(
            self._h, C.c_void_p(ref.data_ptr()), C.c_int64(ref.numel()), C.c_void_p(ref_off.data_ptr()), C.c_void_p(ref_len.data_ptr()), C.c_void_p(ref_pos.data_ptr()),
            C.c_void_p(is_rev.data_ptr()), C.c_void_p(cigar.data_ptr()), C.c_int64(cigar.numel()), C.c_void_p(cigar_off.data_ptr()), C.c_void_p(n_cigar.data_ptr()),
            C.c_void_p(seq_len.data_ptr()), C.c_void_p(events.data_ptr()), C.c_int64(events.numel()), C.c_void_p(event_off.data_ptr()), C.c_void_p(n_events.data_ptr()),
            C.c_void_p(rmap.data_ptr()), C.c_int64(rmap.numel() // 2), C.c_void_p(map_off.data_ptr()), C.c_void_p(calib.data_ptr()),
            C.c_int32(region[0]), C.c_int32(region[1]), C.c_int64(n), C.c_void_p(out.data_ptr()), C.c_int64(out.numel() * out.element_size() // EALN.itemsize),
            C.c_void_p(out_off.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(stream)))

    def realign_last_stats(self):
        """the last realign call: reads, calls of profile_hmm_align, their rows and cells, reads finished by the second launch, device
        time of the kernels and of the whole call, and the time by stage (ms)"""
        v = [C.c_int64(-1) for _ in range(5)]; kms = C.c_float(-1); tms = C.c_float(-1); st = [C.c_float(-1) for _ in range(3)]
        check(lib().gab_abea_realign_last_stats(self._h, *[C.byref(x) for x in v], C.byref(kms), C.byref(tms)))
        check(lib().gab_abea_realign_stage_ms(self._h, *[C.byref(x) for x in st]))
        names = ("reads", "hmm_segments", "rows", "cells", "reads_requeued")
        return {**{k: x.value for k, x in zip(names, v)}, "kernel_ms": kms.value, "total_ms": tms.value,
                "prep_ms": st[0].value, "viterbi_ms": st[1].value, "requeue_ms": st[2].value}

    # ---- call-methylation: the two log-likelihoods of every CpG group (gab_abea_meth) ----------------------------------------------
    def set_cpg_model(self, level_mean, level_stdv, level_log_stdv):
        """the CpG model: 15625 entries each, k-mers over A C G M T ranked base 5"""
        a = [np.ascontiguousarray(x, np.float32) for x in (level_mean, level_stdv, level_log_stdv)]
        if any(x.size != NKMER_CPG for x in a):
            raise ValueError(f"the CpG model has {NKMER_CPG} entries")
        check(lib().gab_abea_set_cpg_model(self._h, _p(a[0]), _p(a[1]), _p(a[2])))

    def call_methylation(self, ref, ref_off, ref_len, ref_pos, is_rev, cigar, cigar_off, n_cigar, seq_len, events, event_off, n_events, rmap, map_off, calib,
                         out_off=None, out=None):
        """the packed numpy arrays of realign() -> (sites, out_off, records): sites a SITE array in which read i's are
        sites[out_off[i] : out_off[i] + records[i]["n_sites"]] in ascending start_position, records a METH array.  out: (sites,
        records) to write into instead of new arrays."""
        ref = np.ascontiguousarray(ref, np.uint8); cigar = np.ascontiguousarray(cigar, np.uint32); events = np.ascontiguousarray(events, np.float32)
        ref_off = np.ascontiguousarray(ref_off, np.int64); cigar_off = np.ascontiguousarray(cigar_off, np.int64)
        event_off = np.ascontiguousarray(event_off, np.int64); map_off = np.ascontiguousarray(map_off, np.int64)
        ref_len = np.ascontiguousarray(ref_len, np.int32); ref_pos = np.ascontiguousarray(ref_pos, np.int32); n_cigar = np.ascontiguousarray(n_cigar, np.int32)
        seq_len = np.ascontiguousarray(seq_len, np.int32); n_events = np.ascontiguousarray(n_events, np.int32)
        is_rev = np.ascontiguousarray(is_rev, np.uint8)
        rmap = np.ascontiguousarray(rmap); calib = np.ascontiguousarray(calib)
        if rmap.dtype != RANGE or calib.dtype != CALIB:
            raise ValueError("rmap is a RANGE array, calib a CALIB array")
        n = seq_len.size
        if out_off is None:
            room = meth_room(ref, ref_off, ref_len)
            out_off = np.zeros(n, np.int64)
            if n > 1:
                out_off[1:] = np.cumsum(room[:-1])
            total = int(room.sum())
        else:
            total = None
        out_off = np.ascontiguousarray(out_off, np.int64)
        if out is None:
            if total is None:
                total = int((out_off + meth_room(ref, ref_off, ref_len)).max()) if n else 0
            out = (np.zeros(total, SITE), np.zeros(n, METH))
        sites, res = out
        if sites.dtype != SITE or res.dtype != METH or res.size < n:
            raise ValueError("out: a SITE array and a METH array of one record per read")
        check(lib().gab_abea_meth(self._h, _p(ref), _p(ref_off), _p(ref_len), _p(ref_pos), _p(is_rev), _p(cigar), _p(cigar_off), _p(n_cigar), _p(seq_len),
                                  _p(events), _p(event_off), _p(n_events), _p(rmap), _p(map_off), _p(calib), C.c_int64(n), _p(sites), _p(out_off), _p(res)))
        return sites, out_off, res

    def call_methylation_reads(self, reads):
        """list of (reference bases, ref_pos, is_rev, cigar as uint32 in BAM encoding, seq_len, event means, map as (n_kmers, 2) or
        RANGE, calibration record) -> (sites, out_off, records)"""
        return self.call_methylation(*pack_aligned_reads(reads))

    def call_methylation_device(self, ref, ref_off, ref_len, ref_pos, is_rev, cigar, cigar_off, n_cigar, seq_len, events, event_off, n_events, rmap, map_off,
                                calib, out, out_off, res, stream=0):
        """torch tensors on the handle's GPU as realign_device takes them | out a uint8 tensor of 32 bytes per site record, int64
        out_off and res a uint8 tensor of 40 bytes per read, filled in place (complete when the call returns)"""
        n = seq_len.numel()
        if rmap.numel() % 2 or calib.numel() * calib.element_size() < n * CALIB.itemsize or res.numel() * res.element_size() < n * METH.itemsize:
            raise ValueError("rmap holds int32 pairs, calib 40 bytes and res 40 bytes per read")
        check(lib().gab_abea_meth_device(
            self._h, C.c_void_p(ref.data_ptr()), C.c_int64(ref.numel()), C.c_void_p(ref_off.data_ptr()), C.c_void_p(ref_len.data_ptr()), C.c_void_p(ref_pos.data_ptr()),
            C.c_void_p(is_rev.data_ptr()), C.c_void_p(cigar.data_ptr()), C.c_int64(cigar.numel()), C.c_void_p(cigar_off.data_ptr()), C.c_void_p(n_cigar.data_ptr()),
            C.c_void_p(seq_len.data_ptr()), C.c_void_p(events.data_ptr()), C.c_int64(events.numel()), C.c_void_p(event_off.data_ptr()), C.c_void_p(n_events.data_ptr()),
            C.c_void_p(rmap.data_ptr()), C.c_int64(rmap.numel() // 2), C.c_void_p(map_off.data_ptr()), C.c_void_p(calib.data_ptr()),
            C.c_int64(n), C.c_void_p(out.data_ptr()), C.c_int64(out.numel() * out.element_size() // SITE.itemsize),
            C.c_void_p(out_off.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(stream)))

    def meth_last_stats(self):
        """the last call_methylation call: reads, CpG groups, sites scored, their rows and cells, device time of the kernels and of the
        whole call, and the time by stage (ms)"""
        v = [C.c_int64(-1) for _ in range(5)]; kms = C.c_float(-1); tms = C.c_float(-1); st = [C.c_float(-1) for _ in range(2)]
        check(lib().gab_abea_meth_last_stats(self._h, *[C.byref(x) for x in v], C.byref(kms), C.byref(tms)))
        check(lib().gab_abea_meth_stage_ms(self._h, *[C.byref(x) for x in st]))
        names = ("reads", "groups", "sites", "rows", "cells")
        return {**{k: x.value for k, x in zip(names, v)}, "kernel_ms": kms.value, "total_ms": tms.value, "prep_ms": st[0].value, "score_ms": st[1].value}

    def events_last_stats(self):
        """the last detect_events call: samples, events, reads whose sums were added in order, chunks, chunks run again, kernel and
        whole-call device time, and the kernel time by stage (ms)"""
        v = [C.c_int64(-1) for _ in range(5)]; kms = C.c_float(-1); tms = C.c_float(-1); st = [C.c_float(-1) for _ in range(3)]
        check(lib().gab_abea_events_last_stats(self._h, *[C.byref(x) for x in v], C.byref(kms), C.byref(tms)))
        check(lib().gab_abea_events_stage_ms(self._h, *[C.byref(x) for x in st]))
        names = ("samples", "events", "reads_serial_sums", "chunks", "chunks_redone")
        return {**{k: x.value for k, x in zip(names, v)}, "kernel_ms": kms.value, "total_ms": tms.value,
                "sums_ms": st[0].value, "detect_ms": st[1].value, "fill_ms": st[2].value}

    def last_stats(self):
        """cells filled, bands swept, launches, and the device time of the DP kernels and of all kernels (ms) of the last call"""
        cells = C.c_int64(-1); bands = C.c_int64(-1); launches = C.c_int64(-1); kms = C.c_float(-1); tms = C.c_float(-1)
        check(lib().gab_abea_last_stats(self._h, C.byref(cells), C.byref(bands), C.byref(launches), C.byref(kms), C.byref(tms)))
        return {"cells": cells.value, "bands": bands.value, "launches": launches.value, "kernel_ms": kms.value, "total_ms": tms.value}
