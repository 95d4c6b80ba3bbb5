"""Host: the inputs of test_bedgraph_paths_gpu.py are what they are meant to be.  The predictor (bedgraph_paths.predict, the
kernel's selection rules restated) must find every class of CLASSES in at least one wave of some input under some name, and the
oracle's dense model must give back the designed runs for the records soa_for_runs makes.  These are conditions on the inputs:
nothing here runs on the device."""
import numpy as np
import pytest

import bedgraph_paths as BP
import orc

G = BP.geometry()
WORD_CASES = [(nm, nd) for nm in (4, 5) for nd in (5, 6, 7, 8, 9)]
# A full half-wave of one layout is 64 runs with 63 others between them: 127 disjoint runs whose starts and ends all have the
# same digit count n (only ONE run of an ascending list can begin below a power of ten and end at or above it, so start and end
# cannot differ in all 64).  [10^(n-1), 10^n) must hold 127 runs: n >= 3.
UNIFORM_DIGITS = [n for n in range(1, 10) if 9 * 10 ** (n - 1) >= 2 * G.wave - 1]
UNIFORM_NAMES = [1, 3, 4, 5, 6, 8]
PUT_LINE_NAMES = [8, 9, 44, 45, 64, 65, 200]


def class_list():
    c = []
    for nm, nd in WORD_CASES:
        for what in ("depth digits 1-4 in one wave", "all four alignments of even and of odd lines", "reuse taken", "one lane with a gap"):
            c.append("words(%d, %d): %s" % (nm, nd, what))
    for nm in (4, 5):
        c.append("name %d: refused by one depth of 10000" % nm)
        c.append("name %d: the twin with 9999 stays on the word path" % nm)
        for k in (5, 6, 7, 8):
            c.append("name %d: refused by one line from 10^%d - 1 to beyond" % (nm, k))
        c.append("name %d: last wave of %d lines" % (nm, G.wave_lines - 1))
        c.append("name %d: last wave of 1 line" % nm)
    for nl in (3, 6):
        c.append("name %d: a wave the word path would take under 4 characters" % nl)
    for nd in UNIFORM_DIGITS:
        for n3 in (1, 2, 3, 4):
            c.append("uniform: start and end of %d digits, depth of %d" % (nd, n3))
    for nl in UNIFORM_NAMES:
        c.append("uniform: name %d, reuse taken" % nl)
        c.append("uniform: name %d, reuse refused by one lane" % nl)
    c += ["uniform even lines, bytes odd lines", "bytes even lines, uniform odd lines"]
    c += ["bytes: positions below and from 10000 on in one half-wave", "bytes: depths below and from 10000 on in one half-wave",
          "bytes: every value of a field below 10000", "bytes: every value of a field from 10000 on",
          "bytes: depth of 5 digits", "bytes: depth of 6 digits", "bytes: position 0"]
    for nl in PUT_LINE_NAMES:
        c.append("put_line: name %d" % nl)
    c.append("largest end of the domain (best effort: any path)")
    c += ["staging: kFmtWaveLds - 5 bytes, staged", "staging: kFmtWaveLds - 4 bytes, staged", "staging: kFmtWaveLds - 3 bytes, direct",
          "staging: name of kFmtMaxName characters, staged", "staging: name of kFmtMaxName + 1 characters, direct though it would fit"]
    for r in range(16):
        c.append("copy-out: staged wave of 16 k + %d bytes" % r)
    for n in BP.run_counts():
        c.append("run count %d" % n)
    return c


CLASSES = class_list()


def qualifies(runs):
    """Start and end of every line have one digit count the word path is compiled for."""
    n1, n2 = BP.digits(runs[:, 0]), BP.digits(runs[:, 1])
    return bool((n1 == n1[0]).all() and (n2 == n1[0]).all() and 5 <= n1[0] <= 9)


def classify(key, name_len, runs, waves, hit):
    L = G.wave_lines
    edge_nl = BP.lds_edge_name_len()
    as4 = BP.predict(4, runs) if name_len in (3, 6) else None
    if len(runs) in BP.run_counts():
        hit("run count %d" % len(runs), None)
    for w in waves:
        r = runs[w.first:w.first + w.lines].astype(np.int64)
        where = w
        staged = w.path in ("words", "staged")
        if staged:
            hit("copy-out: staged wave of 16 k + %d bytes" % w.residue, where)
        if w.path == "words":
            pre = "words(%d, %d): " % w.layout
            if w.depth_digits >= {1, 2, 3, 4}:
                hit(pre + "depth digits 1-4 in one wave", where)
            if w.aligns[0] == {0, 1, 2, 3} and w.aligns[1] == {0, 1, 2, 3}:
                hit(pre + "all four alignments of even and of odd lines", where)
            if w.reuse:
                hit(pre + "reuse taken", where)
            if w.gap_lanes == 1:
                hit(pre + "one lane with a gap", where)
            if r[:, 2].max() == 9999:
                hit("name %d: the twin with 9999 stays on the word path" % name_len, where)
        elif name_len in (4, 5) and staged:
            big = r[:, 2] >= BP.DEPTH_LIMIT
            if w.full and qualifies(r) and big.sum() == 1 and r[big][0, 2] == 10000:
                hit("name %d: refused by one depth of 10000" % name_len, where)
            for k in (5, 6, 7, 8):
                odd = (r[:, 0] == 10 ** k - 1) & (r[:, 1] >= 10 ** k)
                if w.full and not big.any() and odd.sum() == 1 and qualifies(r[~odd]):
                    hit("name %d: refused by one line from 10^%d - 1 to beyond" % (name_len, k), where)
            if w is waves[-1] and w.index > 0 and waves[w.index - 1].path == "words" and qualifies(r) and not big.any():
                if w.lines == L - 1:
                    hit("name %d: last wave of %d lines" % (name_len, L - 1), where)
                if w.lines == 1:
                    hit("name %d: last wave of 1 line" % name_len, where)
        if as4 is not None and as4[w.index].path == "words" and w.path != "words":
            hit("name %d: a wave the word path would take under 4 characters" % name_len, where)
        if w.path == "staged":
            for k in range(2):
                if w.halves[k] == "uniform":
                    (n1, n2, n3), = w.half_digits[k]
                    if n1 == n2:
                        hit("uniform: start and end of %d digits, depth of %d" % (n1, n3), where)
            if w.halves == ("uniform", "uniform") and name_len in UNIFORM_NAMES:
                if w.reuse:
                    hit("uniform: name %d, reuse taken" % name_len, where)
                elif w.gap_lanes == 1:
                    hit("uniform: name %d, reuse refused by one lane" % name_len, where)
            if w.halves == ("uniform", "bytes"):
                hit("uniform even lines, bytes odd lines", where)
            if w.halves == ("bytes", "uniform"):
                hit("bytes even lines, uniform odd lines", where)
        for k in range(2):
            if w.halves[k] not in ("bytes", "direct"):
                continue
            rk = r[k::2]
            if len(rk) == G.wave and w.halves[k] == "bytes":          # a whole half-wave, staged: put_dec's ballot over 64 lanes
                if "mixed" in w.dec[k][:2]:
                    hit("bytes: positions below and from 10000 on in one half-wave", where)
                if w.dec[k][2] == "mixed":
                    hit("bytes: depths below and from 10000 on in one half-wave", where)
                if "dec4" in w.dec[k]:
                    hit("bytes: every value of a field below 10000", where)
                if "dec10" in w.dec[k]:
                    hit("bytes: every value of a field from 10000 on", where)
            if w.halves[k] == "bytes":
                for nd in (5, 6):
                    if (BP.digits(rk[:, 2]) == nd).any():
                        hit("bytes: depth of %d digits" % nd, where)
                if (rk[:, 0] == 0).any():
                    hit("bytes: position 0", where)
            if name_len in PUT_LINE_NAMES and len(rk) == G.wave:
                hit("put_line: name %d" % name_len, where)
        if (r[:, 1] == BP.POS_LIMIT - 1).any():
            hit("largest end of the domain (best effort: any path)", where)
        if name_len == edge_nl and w.full:
            for back, path in ((5, "staged"), (4, "staged"), (3, "direct")):
                if w.bytes == G.wave_lds - back and w.path == path:
                    hit("staging: kFmtWaveLds - %d bytes, %s" % (back, path), where)
        if name_len == G.max_name and w.path == "staged":
            hit("staging: name of kFmtMaxName characters, staged", where)
        if name_len == G.max_name + 1 and w.path == "direct" and w.bytes + 4 <= G.wave_lds:
            hit("staging: name of kFmtMaxName + 1 characters, direct though it would fit", where)


@pytest.fixture(scope="module")
def table():
    t = {c: [] for c in CLASSES}
    for key, inp in BP.inputs().items():
        for name in inp.names:
            waves = BP.predict(len(name), inp.runs)

            def hit(cls, w):
                assert cls in t, cls
                t[cls].append((key, len(name), None if w is None else w.index, None if w is None else w.label))
            classify(key, len(name), inp.runs, waves, hit)
    return t


def test_geometry_is_read_from_the_source():
    assert G.wave_lines == 128 and G.waves == 4, "the predictor speaks of even and odd lines of a wave of 128"
    assert sorted(G.word_cases) == WORD_CASES
    assert G.tile == G.sub * G.subs and G.wave_lds % 16 == 0 and G.wave_lds * G.waves <= G.lds
    assert UNIFORM_DIGITS == [3, 4, 5, 6, 7, 8, 9]


def test_class_list_is_the_fixed_one():
    assert len(CLASSES) == len(set(CLASSES)) == 40 + 2 * 8 + 2 + 28 + 12 + 2 + 7 + 7 + 1 + 5 + 16 + 13


@pytest.mark.parametrize("cls", CLASSES)
def test_every_class_is_met(table, cls):
    assert table[cls], "no wave of any input is of this class"


def test_coverage_table(table):
    """The table itself (pytest -s shows it): class, number of waves, the first one."""
    for c in CLASSES:
        hits = table[c]
        first = hits[0] if hits else ("-", 0, None, None)
        print("%-78s %5d  %s name %d wave %s: %s" % ((c, len(hits)) + first))
    assert all(table[c] for c in CLASSES)


def test_the_predictor_on_hand_made_waves():
    """The rules on waves small enough to check by eye."""
    L = G.wave_lines
    runs, _ = BP.lay(20_000, BP.flat(5))
    (w,) = BP.predict(4, runs)
    assert (w.path, w.layout, w.reuse, w.bytes) == ("words", (4, 5), True, L * (4 + 4 + 5 + 5 + 1)) and w.label == "words(4, 5) reuse"
    (w,) = BP.predict(3, runs)
    assert (w.path, w.halves, w.reuse) == ("staged", ("uniform", "uniform"), True)
    (w,) = BP.predict(9, runs)
    assert (w.path, w.halves, w.dec) == ("staged", ("bytes", "bytes"), (("dec10", "dec10", "dec4"),) * 2)
    (w,) = BP.predict(G.max_name + 1, runs)
    assert w.path == "direct"
    (w,) = BP.predict(4, runs[:L - 1])
    assert (w.path, w.halves) == ("staged", ("uniform", "bytes"))
    gap, _ = BP.lay(20_000, BP.flat(5), gaps={3: 1})
    (w,) = BP.predict(4, gap)
    assert (w.path, w.reuse, w.gap_lanes) == ("words", False, 1)
    gap, _ = BP.lay(20_000, BP.flat(5), gaps={4: 1})
    (w,) = BP.predict(4, gap)
    assert (w.path, w.reuse, w.gap_lanes) == ("words", True, 0)      # between lanes: every lane's two runs still touch
    deep = runs.copy()
    deep[7, 2] = 10000
    (w,) = BP.predict(4, deep)
    assert (w.path, w.halves) == ("staged", ("uniform", "bytes")) and w.dec[1] == ("dec10", "dec10", "mixed")
    assert [x.lines for x in BP.predict(4, np.concatenate([runs, BP.lay(30_000, BP.flat(5))[0][:5]]))] == [L, 5]
    assert BP.predict(4, np.zeros((0, 3), np.int64)) == []


def test_records_for_runs_layers():
    pos, ln = BP.records_for_runs([(5, 7, 2), (7, 9, 3), (9, 10, 1), (12, 13, 1)])
    assert sorted(zip(pos.tolist(), ln.tolist())) == [(5, 4), (5, 5), (7, 2), (12, 1)]
    for bad in ([(5, 7, 2), (7, 9, 2)], [(5, 7, 2), (6, 9, 1)], [(5, 5, 1)], [(5, 6, 0)]):
        with pytest.raises(AssertionError):
            BP.as_runs(bad)


@pytest.mark.parametrize("key", BP.KEYS)
def test_oracle_gives_back_the_designed_runs(key):
    inp = BP.inputs()[key]
    soa = BP.soa_for_runs(inp.runs, inp.refs)
    assert len(soa.tid) < 1_000_000
    rc, runs, _ = orc.depth_target(soa, 0, 1 << 20, 0x704)
    assert rc == 0 and np.array_equal(runs, inp.runs)
    assert BP.oracle_text("chr1", inp.runs) == BP.fmt_text("chr1", inp.runs)


def test_check_text_names_the_path():
    inp = BP.inputs()["words_tail1"]
    good = BP.fmt_text("chr10", inp.runs)
    BP.check_text(good, "chr10", inp.runs)
    at = good.index(b"\n", len(good) // 2) - 1
    with pytest.raises(AssertionError, match=r"wave 1, lane \d+\): path words\(5, 5\)"):
        BP.check_text(good[:at] + b"x" + good[at + 1:], "chr10", inp.runs)
    with pytest.raises(AssertionError, match="wave 2.*path staged: even lines bytes, odd lines none"):
        BP.check_text(good[:-3], "chr10", inp.runs)
