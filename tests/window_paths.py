"""Which kernel and which counting route takes each pass of 64 records of a window batch (kernels/bam_window.hip), restated
from the kernel's stated conditions; dense inputs that reach the fast kernel; and the cases test_window_paths_host.py holds
to their routes and test_window_paths_gpu.py runs against the oracle.

k_window_add takes a pass only if it is one target, one window (or exactly one window seam), one read length <= 256 and no
piece straddles the readable end; inside it a pass is counted record by record (`one`), in two rounds (`seam`) or as one
aligned span (`span`).  k_window_rest takes everything else (`rest`); a pass without a counted record is `empty`."""
import functools
from collections import namedtuple

import numpy as np

from highperformancengs_amd.bamio import BamSoA

WAVE = 64                 # records per pass
SPAN_RECORDS = 1024       # records a wave keeps its state across (kWinSpan)
MAX_LQ = 256              # longest read of a fast pass
FAST_REACH = 0x3fffffff   # bytes a fast pass's descriptor covers at most (kFastReach)
SPAN_BYTES = 8192         # eight steps of 64 x 16 bytes
POISON = 0x24             # a C and a G: what lies around the sequences and must never be counted
TAIL = 64                 # bytes of POISON behind seq_off[n]
FAST = ("one", "seam", "span")

# route: rest | one | seam | span | empty.  For the fast routes: lq, nvalid (records of the pass), steps (of the record-wise
# pieces), head (bytes in front of the pass's first sequence in its 16-byte piece), span_steps (span only), first (seam only:
# counted records of the first window).  nok: counted records of the pass, on every route.
Pass = namedtuple("Pass", "route lq nvalid steps head span_steps first nok")


def steps_of(lq):
    """steps of the record-wise pieces: P = pieces per record, floor(64 / P) records per step"""
    P = ((lq + 1) // 2 + 15) // 16
    rps = WAVE // P
    return (WAVE + rps - 1) // rps


def n_windows(refs, W):
    return [ln // W + 1 for _, ln in refs]


def route(soa, W, lim, base_align=0):
    """One Pass per 64 records of the batch.  lim: first byte offset of seq4 that may not be read (seq_off[n] + 16 for
    hpn_window_add, seq_off[n] for hpn_window_add_dev, None = unbounded for the raw route); base_align: address of seq4 mod 16
    (hpn_window_add keeps the host offsets' alignment pattern: 0)."""
    n, nt, nwin = len(soa.tid), len(soa.refs), n_windows(soa.refs, W)
    tid, pos, lqs = soa.tid.astype(np.int64), soa.pos.astype(np.int64), soa.l_qseq.astype(np.int64)
    so, skip = soa.seq_off.astype(np.int64), (soa.flag & 4) != 0
    out = []
    for r0 in range(0, n, WAVE):
        r1 = min(n, r0 + WAVE)
        nvalid = r1 - r0
        t, p, l, s = tid[r0:r1], pos[r0:r1], lqs[r0:r1], so[r0:r1]
        ok = (t >= 0) & ~skip[r0:r1]
        nok = int(ok.sum())

        def entry(kind, lq=0, head=0, span_steps=0, first=0):
            out.append(Pass(kind, lq, nvalid, steps_of(lq) if lq else 0, head, span_steps, first, nok))
        if nok == 0:
            entry("empty")
            continue
        t0, lq = int(t[ok][0]), int(l[0])
        if not (t0 < nt and 1 <= lq <= MAX_LQ and (t[ok] == t0).all() and (l == lq).all() and (p[ok] >= 0).all()):
            entry("rest")
            continue
        w = p[ok] // W
        w0 = int(w[0])
        if (w == w0).all() and (w0 & 0xffff) < nwin[t0]:
            kind = "one"
        elif not (w == w0).all() and ((w == w0) | (w == w0 + 1)).all() and (w0 & 0xffff) < nwin[t0] and ((w0 + 1) & 0xffff) < nwin[t0]:
            kind = "seam"
        else:
            entry("rest")
            continue
        s0 = int(s[0])
        room = FAST_REACH if lim is None else max(int(lim) - s0, 0)
        reach = min(room, FAST_REACH)
        rel = s - s0
        nb = (lq + 1) // 2
        if ((rel < 0) | (rel + 16 * ((nb + 15) // 16) > reach)).any():       # a piece straddles the readable end
            entry("rest")
            continue
        head = (base_align + s0) & 15
        if kind == "one" and lq % 2 == 0 and lq >= 32 and nok == nvalid and (rel == np.arange(nvalid) * (lq // 2)).all():
            total = head + nvalid * (lq // 2)
            if total <= SPAN_BYTES and total - head + 16 <= reach:
                entry("span", lq, head, (total + 1023) >> 10)
                continue
        entry(kind, lq, head, 0, int((w == w0).sum()) if kind == "seam" else 0)
    return out


def tally(passes):
    out = {}
    for p in passes:
        out[p.route] = out.get(p.route, 0) + 1
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------

def dense(groups, W, lead=0, gap=0, seed=1, refs=None):
    """One window per group.  groups: (n, l_qseq[, window[, tid]]) -- n records of one length whose positions climb inside the
    window (default: the group's number; target 0).  Sequences back to back from seq_off[0] = lead, or `gap` bytes apart;
    seq4 takes all 256 byte values at random (padding nibbles hold C/G codes too); the lead, the gaps and TAIL bytes behind
    seq_off[n] hold POISON.  Flags are zero.  One CIGAR operation (l_qseq M) per record."""
    rng = np.random.default_rng(seed)
    tid, pos, lq = [], [], []
    for g, grp in enumerate(groups):
        n, l = grp[0], grp[1]
        w = grp[2] if len(grp) > 2 else g
        t = grp[3] if len(grp) > 3 else 0
        tid.append(np.full(n, t, np.int32))
        pos.append((w * W + (np.arange(n, dtype=np.int64) * W) // max(n, 1)).astype(np.int32))
        lq.append(np.full(n, l, np.int32))
    tid, pos, lq = np.concatenate(tid), np.concatenate(pos), np.concatenate(lq)
    n = len(tid)
    if refs is None:
        refs = [("chrD", int(pos.max()) + W)]
    nb = (lq.astype(np.int64) + 1) // 2
    seq_off = np.zeros(n + 1, np.int64)
    seq_off[0] = lead
    np.cumsum(nb + gap, out=seq_off[1:])
    seq_off[1:] += lead
    seq_off[n] -= gap
    total = int(seq_off[n]) + TAIL
    inside = np.zeros(total + 1, np.int64)
    np.add.at(inside, seq_off[:-1], 1)
    np.add.at(inside, seq_off[:-1] + nb, -1)
    inside = np.cumsum(inside)[:total] > 0
    seq4 = np.where(inside, rng.integers(0, 256, total, dtype=np.uint8), np.uint8(POISON)).astype(np.uint8)
    return BamSoA(refs=list(refs), tid=tid, pos=pos, flag=np.zeros(n, np.uint32), l_qseq=lq,
                  cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=(lq.astype(np.uint32) << 4), seq_off=seq_off.astype(np.uint64),
                  seq4=seq4)


def cut(soa, a, b):
    """records [a, b) as a batch of their own over the same seq4 (seq_off[b] ends it)"""
    return BamSoA(refs=soa.refs, tid=soa.tid[a:b], pos=soa.pos[a:b], flag=soa.flag[a:b], l_qseq=soa.l_qseq[a:b],
                  cigar_off=(soa.cigar_off[a:b + 1] - soa.cigar_off[a]), cigar=soa.cigar[int(soa.cigar_off[a]):int(soa.cigar_off[b])],
                  seq_off=soa.seq_off[a:b + 1], seq4=soa.seq4)


def lim_of(soa, entry):
    """what route() takes as lim for a batch handed to `entry`: host (hpn_window_add), dev (hpn_window_add_dev) or raw"""
    end = int(soa.seq_off[len(soa.tid)])
    return {"host": end + 16, "dev": end, "raw": None}[entry]


def routes(soa, W, entry, base_align=0, cuts=None):
    """route() of every call a batch is handed over in (cuts: the record numbers a new call starts at)"""
    edges = [0] + list(cuts or []) + [len(soa.tid)]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        part = cut(soa, a, b)
        out += route(part, W, lim_of(part, entry), base_align)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------
# A case: soa, W, and how it is handed over.  cuts: record numbers at which a new hpn_window_add call starts; prefixes: record
# counts n -- the case is run once for each batch soa[:n] (a ragged last pass); base_aligns: byte offsets of the seq4 tensor of
# the _dev entry; domain: the oracle and the kernels refuse it (HPN_E_DOMAIN).
Case = namedtuple("Case", "soa W cuts prefixes base_aligns domain")

EVERY_LENGTH = [("every_length", 192, 0), ("every_length_lead5", 192, 5), ("every_length_lead11", 192, 11), ("every_length_200", 200, 0),
                ("every_length_ragged", 0, 0)]            # (193 .. 205 records per length: a head of every value)
TAIL_LENGTHS = [1, 2, 31, 32, 33, 36, 75, 150, 151, 250, 255, 256]
TAIL_BASES = [WAVE, SPAN_RECORDS]                         # the last pass behind one whole pass, and behind a whole span
SPAN_LENGTHS = [32, 34, 36, 62, 64, 100, 150, 176, 208, 250, 254, 256]   # (176 and 208: the only ones with 6 and 7 span steps)
SPAN_NVALID = [64, 63, 17, 1]
SEAM_LENGTHS = [36, 150, 151]
SKIP_LENGTHS = [36, 150, 151]
CALL_CUTS = [1, 63, 65, 1000, 1025]
RAW_TAIL_LENGTHS = [1, 36, 150, 151, 256]
# (a raw batch is a BAM file packed in two block layouts: eight tails per length, not 128)
RAW_TAIL_PREFIXES = [WAVE + k for k in (1, 2, 17, 32, 63, 64)] + [SPAN_RECORDS + 1, SPAN_RECORDS + 63]
RAW_SEED = 7
W_DENSE = 1000


def _case(soa, W, cuts=None, prefixes=None, base_aligns=(0,), domain=False):
    return Case(soa, W, cuts, prefixes, tuple(base_aligns), domain)


@functools.lru_cache(maxsize=None)
def every_length(per, lead):
    return dense([(per or 193 + lq * 7 % 13, lq) for lq in range(1, MAX_LQ + 1)], W_DENSE, lead=lead, seed=100 + per + lead)


@functools.lru_cache(maxsize=None)
def every_tail(lq):
    """1,088 records of one length in one window: the batches are its prefixes of 64 + k and 1024 + k records, k = 1..64"""
    return dense([(SPAN_RECORDS + WAVE, lq, 0)], 1 << 20, seed=200 + lq)


def tail_prefixes():
    return [b + k for b in TAIL_BASES for k in range(1, WAVE + 1)]


@functools.lru_cache(maxsize=None)
def span_align(lq, lead):
    """128 records of one even length in one window, `lead` bytes in front: prefixes of 64 + nvalid records"""
    return dense([(2 * WAVE, lq, 0)], 1 << 20, lead=lead, seed=300 + 16 * lq + lead)


SKIP_SCENES = ["plain", "lane 0 flag 4", "lane 0 tid -1", "lane 63 flag 4", "all but lane 17", "every record", "plain after empty",
               "lane 30 of a span-eligible pass", "skipped record of another length", "lane 0 skipped, of another length",
               "skipped record in front of lane 0", "plain last"]


@functools.lru_cache(maxsize=None)
def skipped(lq):
    """One pass (and one window) per scene of SKIP_SCENES, in that order."""
    soa = dense([(WAVE, lq) for _ in SKIP_SCENES], W_DENSE, seed=400 + lq)
    at = {s: WAVE * i for i, s in enumerate(SKIP_SCENES)}
    soa.flag[at["lane 0 flag 4"]] = 4
    soa.tid[at["lane 0 tid -1"]] = -1
    soa.flag[at["lane 63 flag 4"] + 63] = 4 | 1024
    r = at["all but lane 17"]
    soa.flag[r:r + WAVE] = 4
    soa.flag[r + 17] = 16
    r = at["every record"]
    soa.flag[r:r + WAVE:2] = 4
    soa.tid[r + 1:r + WAVE:2] = -1
    soa.flag[at["lane 30 of a span-eligible pass"] + 30] = 4
    r = at["skipped record of another length"] + 41
    soa.flag[r], soa.l_qseq[r] = 4, lq + 2
    r = at["lane 0 skipped, of another length"]
    soa.tid[r], soa.l_qseq[r] = -1, lq + 1
    r = at["skipped record in front of lane 0"]
    soa.flag[r + 9], soa.seq_off[r + 9] = 4, soa.seq_off[r] - 1
    return soa


def skipped_routes(lq, entry):
    """the route each scene must take (the last pass of a batch cannot be a span under the _dev entry's exact end, and goes to
    k_window_rest there unless its last piece is whole)"""
    fast = "span" if lq % 2 == 0 and lq >= 32 else "one"
    want = [fast, "one", "one", "one", "one", "empty", fast, "one", "rest", "rest", "rest", fast]
    if entry == "dev":
        want[-1] = "one" if ((lq + 1) // 2) % 16 == 0 else "rest"
    return want


@functools.lru_cache(maxsize=None)
def seams(lq):
    """63 passes; in pass k - 1 the window boundary falls behind record k.  Every pass has its own two windows."""
    groups = []
    for k in range(1, WAVE):
        groups += [(k, lq, 2 * k - 2), (WAVE - k, lq, 2 * k - 1)]
    return dense(groups, W_DENSE, seed=500 + lq)


@functools.lru_cache(maxsize=None)
def two_seams():
    """two boundaries under one pass, between two passes of one window"""
    return dense([(WAVE, 150, 0), (20, 150, 1), (20, 150, 2), (24, 150, 3), (WAVE, 150, 4)], W_DENSE, seed=510)


@functools.lru_cache(maxsize=None)
def width_one():
    """W = 1: 64 records per position, then a seam between two positions, at three lengths"""
    groups, w = [], 0
    for lq in SEAM_LENGTHS:
        groups += [(WAVE, lq, w), (WAVE, lq, w + 1), (32, lq, w + 2), (32, lq, w + 3), (WAVE, lq, w + 4)]
        w += 5
    return dense(groups, 1, seed=520)


@functools.lru_cache(maxsize=None)
def cached_window():
    """one wave's passes: windows 5, 5, 3, 5, then the same positions on target 0 and on target 1, and back"""
    refs = [("chrD", 10 * W_DENSE), ("chrE", 10 * W_DENSE)]
    groups = [(WAVE, 150, 5), (WAVE, 150, 5), (WAVE, 150, 3), (WAVE, 150, 5), (WAVE, 150, 7, 0), (WAVE, 150, 7, 1), (WAVE, 150, 7, 0),
              (WAVE, 36, 5, 1), (WAVE, 36, 5, 0), (WAVE, 151, 5, 0), (WAVE, 151, 5, 1)]
    soa = dense(groups, W_DENSE, seed=530, refs=refs)
    for g, grp in enumerate(groups):                         # each pass sorted inside: the same offsets in every pass
        soa.pos[WAVE * g:WAVE * (g + 1)] = grp[2] * W_DENSE + np.arange(WAVE) * 15
    return soa


@functools.lru_cache(maxsize=None)
def short_wrap():
    """more than 65,536 windows at W = 16: window 65,541 is slot 5, and a seam from 65,535 to 65,536 is slots 65,535 and 0"""
    refs = [("long", 16 * 70_000)]
    groups = [(WAVE, 150, 5), (WAVE, 150, 65_541), (WAVE, 36, 0), (30, 36, 65_535), (34, 36, 65_536), (WAVE, 151, 65_541),
              (30, 151, 65_535), (34, 151, 65_536), (WAVE, 150, 0)]
    return dense(groups, 16, seed=540, refs=refs)


@functools.lru_cache(maxsize=None)
def seam_out_of_target():
    """ten windows; a seam from the last one to an eleventh"""
    return dense([(WAVE, 150, 8), (30, 150, 9), (34, 150, 10)], W_DENSE, seed=550, refs=[("c", 10 * W_DENSE - 1)])


@functools.lru_cache(maxsize=None)
def tid_out_of_range():
    soa = dense([(WAVE, 150, 1), (WAVE, 150, 2), (WAVE, 150, 3)], W_DENSE, seed=560)
    soa.tid[WAVE:2 * WAVE] = 1
    return soa


@functools.lru_cache(maxsize=None)
def negative_pos():
    """pos -1 at W > 1: window 0 by the reference's int division"""
    soa = dense([(WAVE, 150, 0), (WAVE, 36, 0), (WAVE, 151, 1)], W_DENSE, seed=570)
    soa.pos[3], soa.pos[WAVE], soa.pos[WAVE + 63] = -1, -1, -1
    return soa


@functools.lru_cache(maxsize=None)
def one_window_many_waves():
    return dense([(70_000, 150, 0)], 100_000, seed=580)


@functools.lru_cache(maxsize=None)
def gaps(gap, lead):
    return dense([(3 * WAVE, lq) for lq in (1, 2, 31, 32, 36, 75, 150, 151, 250, 256)], W_DENSE, lead=lead, gap=gap, seed=590 + gap)


def raw_every_length(half):
    """every_length's records of lengths 1..128 (half 0) or 129..256 (half 1), as a batch of their own for the raw route"""
    soa = every_length(192, 0)
    a, b = (0, 128 * 192) if half == 0 else (128 * 192, 256 * 192)
    return cut(soa, a, b)


def raw_view(soa, seed, layout):
    """soa as the raw route sees it when test_bam_raw_layouts_gpu._raw_check hands it over in `layout`: seq_off = where each
    sequence lies in the inflated stream on the device (which starts with the block the first record starts in)"""
    import bam_layouts as BL
    n = len(soa.tid)
    names = BL.cycling_names(n)
    data, bounds = BL.encode_stream(soa, names, BL.pick_aux(seed, n), qual_seed=seed)
    at = bounds[:-1] + 36 + np.diff(names[1]) + 1 + 4 * np.diff(soa.cigar_off.astype(np.int64))
    nb = (soa.l_qseq.astype(np.int64) + 1) // 2
    stream = np.frombuffer(data, np.uint8)
    assert np.array_equal(BL._gather(stream, at, nb), BL._gather(soa.seq4, soa.seq_off[:-1].astype(np.int64), nb))
    hl = int(bounds[0])
    origin = hl if layout == "samtools" else hl // int(layout[len("htsjdk"):]) * int(layout[len("htsjdk"):])
    return BamSoA(refs=soa.refs, tid=soa.tid, pos=soa.pos, flag=soa.flag, l_qseq=soa.l_qseq, cigar_off=soa.cigar_off, cigar=soa.cigar,
                  seq_off=np.concatenate([at - origin, [int(bounds[-1]) - origin]]).astype(np.uint64), seq4=stream[origin:])


def cases():
    """name -> Case, in the order of the issue's sections"""
    c = {}
    for name, per, lead in EVERY_LENGTH:                                         # a
        c[name] = _case(every_length(per, lead), W_DENSE)
    for lq in TAIL_LENGTHS:                                                      # b
        c["every_tail_%d" % lq] = _case(every_tail(lq), 1 << 20, prefixes=tail_prefixes())
    for lq in SPAN_LENGTHS:                                                      # c
        for lead in range(16):
            c["span_%d_lead%d" % (lq, lead)] = _case(span_align(lq, lead), 1 << 20, prefixes=[WAVE + k for k in SPAN_NVALID],
                                                    base_aligns=range(16) if lead in (0, 9) else (0, (7 * lead + 1) & 15))
    for gap, lead in ((1, 0), (7, 3), (16, 0), (33, 13)):                        # d
        c["gap%d_lead%d" % (gap, lead)] = _case(gaps(gap, lead), W_DENSE, base_aligns=(0, 5))
    for lq in SKIP_LENGTHS:                                                      # e
        c["skipped_%d" % lq] = _case(skipped(lq), W_DENSE)
    for lq in SEAM_LENGTHS:                                                      # f
        c["seams_%d" % lq] = _case(seams(lq), W_DENSE)
    c["two_seams"] = _case(two_seams(), W_DENSE)
    c["width_one"] = _case(width_one(), 1)
    c["cached_window"] = _case(cached_window(), W_DENSE)
    c["short_wrap"] = _case(short_wrap(), 16)
    c["seam_out_of_target"] = _case(seam_out_of_target(), W_DENSE, domain=True)
    c["tid_out_of_range"] = _case(tid_out_of_range(), W_DENSE, domain=True)
    c["negative_pos"] = _case(negative_pos(), W_DENSE)
    c["one_window_many_waves"] = _case(one_window_many_waves(), 100_000)         # g
    c["several_calls"] = _case(every_length(192, 0), W_DENSE, cuts=CALL_CUTS)    # h
    return c


def raw_cases():
    """name -> Case: what goes through the raw route (i), each batch as a BAM file"""
    c = {"raw_every_length_%d" % h: _case(raw_every_length(h), W_DENSE) for h in (0, 1)}
    for lq in RAW_TAIL_LENGTHS:
        c["raw_tails_%d" % lq] = _case(every_tail(lq), 1 << 20, prefixes=RAW_TAIL_PREFIXES)
    for lq in SEAM_LENGTHS:
        c["raw_seams_%d" % lq] = _case(seams(lq), W_DENSE)
    return c


def batches(case):
    """(label, soa of the batch, cuts) for every batch a case is run on"""
    if case.prefixes:
        return [("n=%d" % n, cut(case.soa, 0, n), None) for n in case.prefixes]
    return [("", case.soa, case.cuts)]
