"""k_bedgraph_text (kernels/bam_depth.hip) picks, per wave of 128 lines, one of four ways to write "%s\\t%d\\t%d\\t%d\\n".  This
module holds what the tests of those ways share: a builder of records whose coverage is a GIVEN list of runs (soa_for_runs), a
plain-Python restatement of the kernel's selection rules (predict), the designed run lists (inputs) and the comparison that
names the path of the first wrong line (check_text).

Nothing here looks at what the device computes: the expected text is formatted from the designed runs."""
import ctypes as C
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

from highperformancengs_amd import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "highperformancengs_amd", "csrc", "kernels", "bam_depth.hip")
COMMON = os.path.join(ROOT, "highperformancengs_amd", "csrc", "kernels", "common.hpp")

# Written as literals in the kernel's conditions (k_bedgraph_text): the one-layout path takes names that fit two registers, the
# word and the one-layout path depths of at most four digits (one ascii4 group).
UNIFORM_MAX_NAME = 8
DEPTH_LIMIT = 10000
POS_LIMIT = 1 << 28          # breakpoints are keys of 28 bits (hpn_bam.hip: kPosLimit); the largest end a run can have is one less


# ---- the geometry, from the source ---------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Geometry:
    wave: int            # lanes of a wavefront
    threads: int         # kFmtThreads
    per: int             # kFmtPer: lines per lane
    subs: int            # HPN_BG_SUBS: pieces a workgroup takes in a row
    lds: int             # HPN_BG_LDS: bytes of text a piece may stage
    max_name: int        # kFmtMaxName
    word_cases: frozenset   # (name length, digits of start and end) put_pair_words is compiled for

    @property
    def wave_lines(self):
        return self.wave * self.per

    @property
    def waves(self):
        return self.threads // self.wave

    @property
    def sub(self):       # kFmtSub: lines of a piece
        return self.threads * self.per

    @property
    def tile(self):      # kFmtTile: lines of a workgroup
        return self.sub * self.subs

    @property
    def wave_lds(self):  # kFmtWaveLds: every wave's own part of the staging buffer
        return (self.lds // self.waves) & ~15


@functools.lru_cache(None)
def geometry():
    src = open(SRC).read()
    assert re.search(r"kFmtSub = kFmtThreads \* kFmtPer;", src)
    assert re.search(r"kFmtSubs = HPN_BG_SUBS, kFmtTile = kFmtSub \* kFmtSubs;", src)
    assert re.search(r"kFmtLds = HPN_BG_LDS;", src)
    assert re.search(r"kFmtWaveLds = \(kFmtLds / \(kFmtThreads / kWave\)\) & ~15;", src)
    assert re.search(r"name_len <= kFmtMaxName && wave_bytes \+ 4u <= \(uint32_t\)kFmtWaveLds", src)

    def num(pattern, text=src):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    cases = frozenset((int(a), int(b)) for a, b in re.findall(r"HPN_BG_CASE\((\d+), (\d+)\)", src))
    return Geometry(wave=num(r"constexpr int kWave = (\d+);", open(COMMON).read()), threads=num(r"kFmtThreads = (\d+)"),
                    per=num(r"kFmtPer = (\d+)"), subs=num(r"#define HPN_BG_SUBS (\d+)"), lds=num(r"#define HPN_BG_LDS (\d+)"),
                    max_name=num(r"kFmtMaxName = (\d+);"), word_cases=cases)


# ---- records whose coverage is a given list of runs -----------------------------------------------------------------------------

def as_runs(runs):
    a = np.asarray(runs, np.int64).reshape(-1, 3)
    if len(a):
        assert (a[:, 0] >= 0).all() and (a[:, 1] > a[:, 0]).all() and (a[:, 2] > 0).all(), "a run is (start, end > start, depth > 0)"
        assert a[:, 1].max() < POS_LIMIT
        assert (a[1:, 0] >= a[:-1, 1]).all(), "runs are disjoint and ascending"
        touch = a[1:, 0] == a[:-1, 1]
        assert (a[1:, 2][touch] != a[:-1, 2][touch]).all(), "runs that touch differ in depth (else they are one run)"
    return a.astype(np.int32)


def records_for_runs(runs):
    """(pos, length) of plain nM records, sorted by pos, that cover exactly `runs`: layers over every stretch of touching runs -- a
    record opens where the depth rises and the one opened last closes where it falls, so a stretch costs the sum of its rises."""
    pos, ln, cnt = [], [], []
    stack = []                                    # [start, how many records opened there are still open]

    def close(k, at):
        while k:
            top = stack[-1]
            t = min(k, top[1])
            pos.append(top[0]), ln.append(at - top[0]), cnt.append(t)
            top[1] -= t
            k -= t
            if top[1] == 0:
                stack.pop()
    prev_end, prev_d = None, 0
    for s, e, d in as_runs(runs).tolist():
        if prev_end is not None and s != prev_end:
            close(prev_d, prev_end)
            prev_d = 0
        if d > prev_d:
            stack.append([s, d - prev_d])
        else:
            close(prev_d - d, s)
        prev_end, prev_d = e, d
    if prev_end is not None:
        close(prev_d, prev_end)
    assert not stack
    cnt = np.array(cnt, np.int64)
    pos, ln = np.repeat(np.array(pos, np.int64), cnt), np.repeat(np.array(ln, np.int64), cnt)
    order = np.argsort(pos, kind="stable")
    return pos[order].astype(np.int32), ln[order].astype(np.int64)


def soa_for_runs(runs, refs):
    """A bamio.BamSoA of plain nM records on target 0 of `refs` whose coverage is exactly the disjoint, ascending (start, end,
    depth) `runs`."""
    pos, ln = records_for_runs(runs)
    n = len(pos)
    cigar = (ln.astype(np.uint32) << 4) if n else np.zeros(1, np.uint32)        # op 0: M
    return bamio.BamSoA(refs=list(refs), tid=np.zeros(n, np.int32), pos=pos, flag=np.zeros(n, np.uint32), l_qseq=np.zeros(n, np.int32),
                        cigar_off=np.arange(n + 1, dtype=np.uint32), cigar=np.ascontiguousarray(cigar, np.uint32),
                        seq_off=np.zeros(n + 1, np.uint64), seq4=np.zeros(1, np.uint8))


# ---- the kernel's selection rules, restated --------------------------------------------------------------------------------------

_P10 = np.array([10 ** k for k in range(1, 10)], np.int64)


def digits(v):
    return 1 + np.searchsorted(_P10, np.asarray(v, np.int64), side="right")


@dataclass
class Wave:
    index: int
    first: int                  # index of its first run
    lines: int                  # 1 .. wave_lines
    path: str                   # "words" | "staged" | "direct"
    halves: tuple               # per half-wave (even lines, odd lines): "words" | "uniform" | "bytes" | "direct" | "none"
    layout: tuple               # words: (name length, digits); else None
    reuse: bool                 # the start digits of the odd lines were taken from the even lines' end
    gap_lanes: int              # lanes whose two runs do not touch
    bytes: int
    aligns: tuple = ()          # (set of `at & 3` of the even lines, of the odd lines)
    depth_digits: frozenset = frozenset()
    half_digits: tuple = ()     # per half-wave: the set of (n1, n2, n3) of its lines
    dec: tuple = ()             # per half-wave that put_line writes: per field (start, end, depth) "dec4" | "dec10" | "mixed"

    @property
    def residue(self):
        return self.bytes % 16

    @property
    def full(self):
        return self.lines == geometry().wave_lines

    @property
    def label(self):
        if self.path == "words":
            return "words(%d, %d)%s" % (self.layout + (" reuse" if self.reuse else "",))
        if self.path == "direct":
            return "direct"
        return "staged: even lines %s, odd lines %s%s" % (self.halves + (" (reuse)" if self.reuse else "",))


def predict(name_len, runs):
    """What k_bedgraph_text does with every wave of `runs` under a name of `name_len` characters: a list of Wave."""
    g = geometry()
    assert g.per == 2, "a lane's two lines: even and odd"
    a = np.asarray(runs, np.int64).reshape(-1, 3)
    assert (a >= 0).all(), "no run the scan emits is negative"
    out = []
    for w0 in range(0, len(a), g.wave_lines):
        r = a[w0:w0 + g.wave_lines]
        n = len(r)
        n1, n2, n3 = digits(r[:, 0]), digits(r[:, 1]), digits(r[:, 2])
        size = name_len + 4 + n1 + n2 + n3
        at = np.concatenate([[0], np.cumsum(size)[:-1]])
        total = int(size.sum())
        full = n == g.wave_lines
        ev, od = slice(0, n, 2), slice(1, n, 2)
        pairs = n // 2                                           # lanes that hold two lines
        gap_lanes = int((r[1:2 * pairs:2, 0] != r[0:2 * pairs:2, 1]).sum())
        adjacent = full and gap_lanes == 0                       # (the ballot counts a missing line as a gap: its values are zero)
        small = bool((r[:, 2] < DEPTH_LIMIT).all())
        staged = name_len <= g.max_name and total + 4 <= g.wave_lds
        layout, reuse, dec = None, False, []
        if not staged:
            path, halves = "direct", ["direct" if n > k else "none" for k in range(2)]
        elif (full and small and (name_len, int(n1[0])) in g.word_cases and (n1 == n1[0]).all() and (n2 == n1[0]).all()):
            path, halves, layout, reuse = "words", ["words", "words"], (name_len, int(n1[0])), adjacent
        else:
            path, halves = "staged", []
            for k, sl in enumerate((ev, od)):
                m = len(r[sl])
                if m == 0:
                    halves.append("none")
                elif (name_len <= UNIFORM_MAX_NAME and m == g.wave and (r[sl, 2] < DEPTH_LIMIT).all() and
                      (n1[sl] == n1[sl][0]).all() and (n2[sl] == n2[sl][0]).all() and (n3[sl] == n3[sl][0]).all()):
                    halves.append("uniform")
                else:
                    halves.append("bytes")
            reuse = halves == ["uniform", "uniform"] and adjacent
        for k, sl in enumerate((ev, od)):                         # put_dec's ballot, per field, over the lanes that hold the line
            if halves[k] in ("bytes", "direct"):
                big = r[sl] >= DEPTH_LIMIT
                dec.append(tuple("dec4" if not c.any() else "dec10" if c.all() else "mixed" for c in big.T))
            else:
                dec.append(None)
        out.append(Wave(index=w0 // g.wave_lines, first=w0, lines=n, path=path, halves=tuple(halves), layout=layout, reuse=reuse,
                        gap_lanes=gap_lanes, bytes=total, aligns=(frozenset((at[ev] & 3).tolist()), frozenset((at[od] & 3).tolist())),
                        depth_digits=frozenset(n3.tolist()),
                        half_digits=tuple(frozenset(zip(n1[sl].tolist(), n2[sl].tolist(), n3[sl].tolist())) for sl in (ev, od)),
                        dec=tuple(dec)))
    return out


# ---- the expected text and the comparison ------------------------------------------------------------------------------------------

def fmt_text(name, runs):
    nm = name.encode()
    return b"".join(b"%s\t%d\t%d\t%d\n" % (nm, s, e, d) for s, e, d in np.asarray(runs).tolist())


def oracle_text(name, runs):
    """The reference's fprintf over the same runs (orc_fmt_bedgraph)."""
    import orc
    L = orc.lib()
    f = orc._CFile()
    arr = np.ascontiguousarray(runs, np.int32).reshape(-1, 3)
    L.orc_fmt_bedgraph(f.fp, name.encode(), C.cast(arr.ctypes.data, C.POINTER(orc.Run)), len(arr))
    return f.read()


def check_text(got, name, runs, want=None):
    """`got` must be the text of the DESIGNED runs; the first wrong line is reported with its wave and that wave's predicted path."""
    want = fmt_text(name, runs) if want is None else want
    if got == want:
        return
    n = min(len(got), len(want))
    diff = np.nonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))[0]
    at = int(diff[0]) if len(diff) else n
    line = want.count(b"\n", 0, at)
    waves = predict(len(name), runs)
    g = geometry()
    where = waves[line // g.wave_lines].label if line // g.wave_lines < len(waves) else "behind the last wave"
    beg = want.rfind(b"\n", 0, at) + 1
    end = want.find(b"\n", at)
    raise AssertionError("name of %d characters: %d bytes for %d; first wrong byte %d in line %d (line %d of wave %d, lane %d): path %s\n"
                         "  want %r\n  got  %r" % (len(name), len(got), len(want), at, line, line % g.wave_lines, line // g.wave_lines,
                                                   line % g.wave_lines // g.per, where, want[beg:end + 1 if end >= 0 else len(want)],
                                                   got[beg:beg + (end + 1 - beg if end >= 0 else 80) + 8]))


# ---- the designed inputs ---------------------------------------------------------------------------------------------------------

@dataclass
class Input:
    runs: np.ndarray
    names: list
    tlen: int

    @property
    def refs(self):
        return [("t", self.tlen)]


def lay(start, depths, lens=1, gaps=None):
    """Runs from `start` on: run i has depth depths[i] and length lens (one number, or one per run); gaps[i] positions without
    coverage lie in front of run i.  -> (runs, the position behind the last run)."""
    n = len(depths)
    lens = np.broadcast_to(np.asarray(lens, np.int64), (n,))
    gap = np.zeros(n, np.int64)
    for i, v in (gaps or {}).items():
        gap[i] = v
    s = start + np.cumsum(gap) + np.concatenate([[0], np.cumsum(lens)[:-1]])
    runs = np.stack([s, s + lens, np.asarray(depths, np.int64)], axis=1)
    return runs, int(runs[-1, 1])


def hill(n=None):
    """Depths of one wave: up through one, two, three and four digits and down again, in stretches of uneven length, no two
    neighbours alike: ~1,100 records whatever n; both sides of 9 | 10, 99 | 100 and 999 | 1000."""
    n = geometry().wave_lines if n is None else n
    edges = [0, 13, 30, 45, 64, 79, 98, 111, 128]
    bases = [8, 98, 998, 1000, 1002, 100, 10, 1]
    i = np.arange(n)
    seg = np.searchsorted(np.array(edges[1:]) * n // 128, i, side="right").clip(0, 7)
    return np.array(bases)[seg] + (i & 1)


def flat(base, n=None):
    """Depths base, base + 1, base, ...: one digit count in both half-waves."""
    n = geometry().wave_lines if n is None else n
    return base + (np.arange(n) & 1)


def _words():
    """Every compiled layout of the word path twice (all lanes adjacent / one lane with a gap), the refusals by one line that
    straddles a power of ten, by one depth of 10000 (and its twin with 9999), and the largest end of the domain."""
    g = geometry()
    L = g.wave_lines
    parts = []
    for nd in range(5, 10):
        at = 2 * 10 ** (nd - 1)
        # gaps BETWEEN lanes only (in front of even lines): every lane's two runs touch, the reuse is taken
        r, at = lay(at, hill(), lens=1 + (np.arange(L) % 3 == 0), gaps={10: 3, 64: 1, 126: 7})
        parts.append(r)
        r, at = lay(at + 5, hill(), gaps={2 * 37 + 1: 2})        # exactly one lane whose runs do not touch
        parts.append(r)
        if nd == 7:                                              # one depth of 10000 in a wave that qualifies; its twin with 9999
            for big in (10000, 9999):
                d = hill()
                d[51] = big
                r, at = lay(at + 5, d)
                parts.append(r)
        if nd < 9:                                               # one line from 10^nd - 1 to beyond: the last line of a wave, or the first
            edge = 10 ** nd
            if nd % 2:
                r, _ = lay(edge - L, hill(), lens=[1] * (L - 1) + [3])
            else:
                r, _ = lay(edge - 1, hill(), lens=[3] + [1] * (L - 1))
            assert r[:, 0].min() > at and (r[:, 0] == edge - 1).sum() == 1 and r[r[:, 0] == edge - 1][0, 1] > edge
            parts.append(r)
    d = hill()                                                   # the last wave ends at the largest end there is
    r, _ = lay(POS_LIMIT - 1 - L - 4, d, lens=[1] * (L - 1) + [5])
    assert r[-1, 1] == POS_LIMIT - 1
    parts.append(r)
    return Input(np.concatenate(parts), ["chr", "chr1", "chr10", "chr1_a"], POS_LIMIT - 1)


def _words_tail(extra):
    """Two whole waves of the word path and a last wave of `extra` lines."""
    L = geometry().wave_lines
    d = np.concatenate([hill(), hill(), hill()[:extra]])
    r, _ = lay(30_000, d, gaps={200: 4})
    return Input(r, ["chr1", "chr10"], 100_000)


def _uniform():
    """Half-waves of one layout: start and end of 3 .. 9 digits, depths of 1 .. 4 digits, with every lane's runs touching and with one
    lane's apart; then waves of which only the even or only the odd lines have one layout."""
    parts = []
    for nd in range(3, 10):
        at = 10 ** (nd - 1) + (0 if nd == 3 else 11)
        for n3, base in enumerate((4, 40, 400, 4000), 1):
            gaps = {2 * 20 + 1: 1} if n3 % 2 == 0 else {2 * 9: 2}       # (a gap between lanes leaves the reuse alone)
            r, at = lay(at + 1, flat(base), gaps=gaps)
            parts.append(r)
        if nd == 4:
            for odd_one_out in (77, 78):                         # one line of another depth digit count: its half-wave goes byte by byte
                d = flat(40)
                d[odd_one_out] = 100
                r, at = lay(at + 1, d)
                parts.append(r)
    return Input(np.concatenate(parts), ["c", "chr", "chr1", "chr10", "chr1_a", "chr1_abc", "chr1_abcd"], POS_LIMIT - 1)


def _bytes():
    """Lines of mixed digit counts: position 0, starts and ends on both sides of 10000 within one half-wave, depths on both sides of
    10000 and of five and six digits."""
    L = geometry().wave_lines
    r0, _ = lay(0, flat(1))
    d = flat(3)
    d[60:66] = [9999, 10000, 99999, 100000, 99998, 10001]
    r1, _ = lay(10_000 - L // 2, d)
    r2, _ = lay(123_456_700, flat(7, 40), gaps={11: 3})
    return Input(np.concatenate([r0, r1, r2]), ["chr1_abc", "chr1_abcd", "n" * 20, "x" * 44, "y" * 45, "z" * 64, "w" * 65, "HLA-" + "q" * 196],
                 200_000_000)


def lds_edge_name_len():
    """The name length at which a wave of 128 lines with positions of three digits reaches kFmtWaveLds - 4 bytes through the depths'
    digits (one or two) alone."""
    g = geometry()
    for nl in range(UNIFORM_MAX_NAME + 1, g.max_name + 1):
        lo, hi = g.wave_lines * (nl + 4 + 3 + 3 + 1), g.wave_lines * (nl + 4 + 3 + 3 + 2)
        if lo <= g.wave_lds - 5 and g.wave_lds - 3 <= hi:
            return nl
    raise AssertionError("no name length puts a wave of three-digit positions on the staging threshold")


def _lds_edge():
    """Three waves of kFmtWaveLds - 5, - 4 and - 3 bytes under one name length (the staging test is `bytes + 4 <= kFmtWaveLds`), and a
    short last wave that a name of kFmtMaxName characters still stages."""
    g = geometry()
    L, nl = g.wave_lines, lds_edge_name_len()
    parts, at = [], 100
    for target in (g.wave_lds - 5, g.wave_lds - 4, g.wave_lds - 3):
        ones = L * (nl + 4 + 3 + 3 + 2) - target                 # lines whose depth has one digit instead of two
        d = flat(10)
        d[1:2 * ones:2] = 9
        r, at = lay(at + 1, d)
        parts.append(r)
    r, at = lay(at + 1, flat(10, 40))
    parts.append(r)
    assert at < 1000
    return Input(np.concatenate(parts), ["e" * nl, "f" * g.max_name, "g" * (g.max_name + 1)], 1000)


def _tail16():
    """Sixteen waves whose byte counts differ by one: every length of the copy-out's byte-wise tail."""
    parts, at = [], 1000
    for w in range(16):
        d = flat(10)
        d[1:2 * w:2] = 9
        r, at = lay(at + 1, d, lens=2)
        parts.append(r)
    assert at < 10_000
    return Input(np.concatenate(parts), ["c", "chr1", "chr10", "s" * 20], 10_000)


def _count(n):
    d = 5 + (np.arange(n) & 1)
    if n == 0:
        return Input(np.zeros((0, 3), np.int64), ["chr1", "c", "v" * 50], 100_000)
    r, at = lay(20_000, d, gaps={i: 1 for i in range(7, n, 7)})
    assert at < 100_000
    return Input(r, ["chr1", "c", "v" * 50], 100_000)


def run_counts():
    g = geometry()
    return [0, 1, 2, g.wave_lines - 1, g.wave_lines, g.wave_lines + 1, g.sub - 1, g.sub, g.sub + 1, g.tile - 1, g.tile, g.tile + 1,
            2 * g.tile + 77]


# (the keys are fixed here so that tests can be parametrised by them without building anything)
KEYS = ["words", "words_tail127", "words_tail1", "uniform", "bytes", "lds_edge", "tail16"] + ["count%02d" % i for i in range(13)]


@functools.lru_cache(None)
def inputs():
    g = geometry()
    d = {"words": _words(), "words_tail127": _words_tail(g.wave_lines - 1), "words_tail1": _words_tail(1), "uniform": _uniform(),
         "bytes": _bytes(), "lds_edge": _lds_edge(), "tail16": _tail16()}
    counts = run_counts()
    assert len(counts) == 13
    for i, n in enumerate(counts):
        d["count%02d" % i] = _count(n)
    assert list(d) == KEYS
    for v in d.values():
        v.runs = as_runs(v.runs)
        v.runs.setflags(write=False)
    return d
