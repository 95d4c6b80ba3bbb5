"""CPU only: the plain reference of the K2 tests (trim_ref.py) against the C oracle on every input test_trim_paths_gpu.py uses, and
the inputs (trim_inputs.py) against what they claim to hit.  The second half is a condition on the inputs: a wave of k_trim_copy
is records 64 w .. 64 w + 63 of the batch as passed, and it takes the fast path when lane 0 keeps 16..1024 bytes and all 64 lanes
keep the same count (trim_ref.uniform_waves computes exactly that).  If a builder drifts, these fail -- the GPU file does not
silently stop covering a path.
"""
import numpy as np
import pytest

import orc
import trim_inputs as ti
import trim_ref

GRID_SLICE = 50_000


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} differ, first at {int(bad[0])}: ref {got[bad[0]]}, oracle {want[bad[0]]}")


def _some(a):
    return a if len(a) else np.zeros(1, a.dtype)          # (the oracle's bindings want a non-empty array)


def _orc_points(seq, qual, off, beg, end):
    n = len(off) - 1
    cap = max(len(seq), 1)
    oseq, oqual, ooff = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64)
    rc = orc.lib().orc_trim_points_soa(_some(seq), _some(qual), off, n, _some(beg), _some(end), oseq, oqual, ooff)
    assert rc == 0
    tot = int(ooff[-1])
    return oseq[:tot], oqual[:tot], ooff


def _orc_qtrim(qual, off, T):
    n = len(off) - 1
    beg, end = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    orc.lib().orc_qtrim_points(_some(qual), off, n, T, beg, end)
    return beg[:n], end[:n]


def _fixed_vs_oracle(b, S, E, what):
    """trim_ref.cut against orc_trim_soa and, with the cycles as every record's points, against orc_trim_points_soa."""
    n = len(b.off) - 1
    got = trim_ref.cut(b.seq, b.qual, b.off, S, E)
    rc, wseq, wqual, woff = orc.trim_soa(b.seq, b.qual, b.off, S, E)
    assert rc == 0
    for g, w, name in zip(got, (wseq, wqual, woff), ("out_seq", "out_qual", "out_off")):
        _same(g, w, f"{what} {name} vs orc_trim_soa")
    want = _orc_points(b.seq, b.qual, b.off, np.full(n, S, np.uint32), np.full(n, E, np.uint32))
    for g, w, name in zip(got, want, ("out_seq", "out_qual", "out_off")):
        _same(g, w, f"{what} {name} vs orc_trim_points_soa")
    return got


def _head(b, m):
    """The first m records of a batch (the arrays stay whole)."""
    return ti.Batch(b.seq, b.qual, b.off[:m + 1], b.hits, None if b.beg is None else b.beg[:m], None if b.end is None else b.end[:m])


# ---- 1. the reference equals the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in ti.fixed_cases() if not k.startswith("A2 ")])
def test_cut_equals_oracle(name):
    build, S, E = ti.fixed_cases()[name]
    _fixed_vs_oracle(build(), S, E, name)


def test_cut_equals_oracle_a2():
    b = ti.case_a2()
    for k in ti.A2_KEPT:
        for S in ti.A2_S:
            oseq, oqual, ooff = _fixed_vs_oracle(b, S, S + k, f"A2 kept={k} S={S}")
            assert ooff.tolist() == [k * i for i in range(ti.A2_N + 1)]


@pytest.mark.parametrize("n", ti.D_SEAMS)
def test_cut_equals_oracle_seams(n):
    b = ti.case_d_seam(n)
    w = ti.Batch(b.seq, b.qual, b.off[ti.D_LEAD:], b.hits)
    got = _fixed_vs_oracle(w, *ti.D_SEAM_CUT, f"D n={n} window")
    alone = _fixed_vs_oracle(ti.own(b, ti.D_LEAD), *ti.D_SEAM_CUT, f"D n={n} own")
    for g, a in zip(got, alone):
        _same(g, a, f"D n={n} window vs own")
    assert len(w.off) == n + 1 and int(w.off[0]) > 0 and int(ti.own(b, ti.D_LEAD).off[0]) == 0
    assert n < 4096 or (trim_ref.kept_counts(w.off, *ti.D_SEAM_CUT) == 0).sum() > n // 4       # many empty records


def test_cut_and_points_equal_oracle_grid_slice():
    g = ti.case_d_grid()
    assert len(g.off) - 1 == ti.GRID_CUS * 8 * 256 + 4096 + 77 == g.hits["n"]
    b = _head(g, GRID_SLICE)
    _fixed_vs_oracle(b, *ti.D_GRID_CUT, "D grid")
    got = trim_ref.qtrim_points(b.qual, b.off, ti.D_GRID_T)
    for x, w, name in zip(got, _orc_qtrim(b.qual, b.off, ti.D_GRID_T), ("beg", "end")):
        _same(x, w, f"D grid qtrim {name}")
    # the whole batch goes through the reference's loop-free form: held against the loop on the slice, the oracle on all of it
    for x, w, name in zip(trim_ref.qtrim_points_flat(b.qual, b.off, ti.D_GRID_T), got, ("beg", "end")):
        _same(x, w, f"D grid qtrim_points_flat vs qtrim_points {name}")
    for x, w, name in zip(trim_ref.qtrim_points_flat(g.qual, g.off, ti.D_GRID_T), _orc_qtrim(g.qual, g.off, ti.D_GRID_T), ("beg", "end")):
        _same(x, w, f"D grid qtrim_points_flat {name}")
    ln = np.diff(b.off.astype(np.int64))
    assert ((got[1] == 0) & (ln > 0)).any() and (got[0] > 0).any() and (got[1] < ln).any()    # no hit, a late first, an early last


@pytest.mark.parametrize("name", list(ti.points_cases()))
def test_cut_points_equals_oracle(name):
    b = ti.points_cases()[name]()
    got = trim_ref.cut_points(b.seq, b.qual, b.off, b.beg, b.end)
    for g, w, what in zip(got, _orc_points(b.seq, b.qual, b.off, b.beg, b.end), ("out_seq", "out_qual", "out_off")):
        _same(g, w, f"{name} {what}")


def _qtrim_vs_oracle(b, T, what):
    beg, end = trim_ref.qtrim_points(b.qual, b.off, T)
    wb, we = _orc_qtrim(b.qual, b.off, T)
    _same(beg, wb, f"{what} T={T} beg")
    _same(end, we, f"{what} T={T} end")
    got = trim_ref.cut_points(b.seq, b.qual, b.off, beg, end)
    for g, w, name in zip(got, _orc_points(b.seq, b.qual, b.off, wb, we), ("out_seq", "out_qual", "out_off")):
        _same(g, w, f"{what} T={T} cut {name}")
    for x, w, name in zip(trim_ref.qtrim_points_flat(b.qual, b.off, T), (beg, end), ("beg", "end")):
        _same(x, w, f"{what} T={T} qtrim_points_flat {name}")
    return beg, end


@pytest.mark.parametrize("T", ti.F_T)
def test_qtrim_points_equals_oracle_directed(T):
    b = ti.case_f_directed(T)
    beg, end = _qtrim_vs_oracle(b, T, "F directed")
    # the builder's own statement of where the hits are
    for i, (ln, ps) in enumerate(b.hits["rows"]):
        want = (0, ln) if ps is None else (min(ps), max(ps) + 1) if ps else (0, 0)
        assert (int(beg[i]), int(end[i])) == want, (i, ln, ps)


@pytest.mark.parametrize("T", ti.F_RANDOM_T)
def test_qtrim_points_equals_oracle_random(T):
    b = ti.case_f_random()
    beg, end = _qtrim_vs_oracle(b, T, "F random")
    ln = np.diff(b.off.astype(np.int64))
    if T == 0:
        assert not beg.any() and np.array_equal(end, ln)
    if T > 255:
        assert not beg.any() and not end.any()


@pytest.mark.parametrize("T", [53, 256])
def test_qtrim_points_equals_oracle_dev_inputs(T):
    _qtrim_vs_oracle(ti.case_dev("e_mixed_0_300"), T, "E mixed")


# ---- 2. the builders hit what they claim --------------------------------------------------------------------------------------
def test_case_a_has_a_uniform_wave_at_every_fast_path_count():
    b = ti.case_a()
    assert sorted(b.hits["group_lengths"]) == sorted(ti.A_LENGTHS) and len(b.off) - 1 == 64 * len(ti.A_LENGTHS)
    every = set(range(trim_ref.FAST_MIN, trim_ref.FAST_MAX + 1))
    for S, E in ti.A_CUTS:
        assert set(trim_ref.uniform_waves(b.off, S, E)) == every, (S, E)
        # and on both sides of it: waves of one count below 16 and above 1024, which must take the mixed path
        flat = trim_ref.wave_counts(b.off, S, E)
        one = flat[(flat == flat[:, :1]).all(axis=1), 0]
        assert {0, 1, 15, 1025, 1037 - S, 1279 - S, 4100 - S} <= set(one.tolist())
    # S = 3: within the uniform waves, sources and destinations differ mod 16 (a piece is never aligned on both sides)
    o = b.off.astype(np.int64)
    dst = np.concatenate([[0], np.cumsum(trim_ref.kept_counts(b.off, 3, ti.E_ALL))])[:-1]
    assert ((o[:-1] + 3 - dst) % 16 != 0).mean() > 0.9


def test_case_a2_has_two_uniform_waves_and_a_tail():
    b = ti.case_a2()
    for k in ti.A2_KEPT:
        for S in ti.A2_S:
            want = [k, k] if trim_ref.FAST_MIN <= k <= trim_ref.FAST_MAX else []
            assert trim_ref.uniform_waves(b.off, S, S + k) == want, (k, S)
            w = trim_ref.wave_counts(b.off, S, S + k)
            assert w.shape == (3, 64) and w[2].tolist() == [k] + [0] * 63


def test_case_b_has_no_uniform_wave():
    for p in ti.B_PREFIX:
        b = ti.case_a(p)
        assert len(b.off) - 1 == p + 64 * len(ti.A_LENGTHS)
        assert trim_ref.uniform_waves(b.off, 0, ti.E_ALL, lo=16, hi=1 << 40) == [], p
        # every length of case A is still there, 64 times
        ln, cnt = np.unique(np.diff(b.off.astype(np.int64))[p:], return_counts=True)
        assert ln.tolist() == sorted(ti.A_LENGTHS) and (cnt == 64).all()
    b = ti.case_b_groups()
    assert trim_ref.uniform_waves(b.off, 0, ti.E_ALL, lo=16, hi=1 << 40) == []
    ln, cnt = np.unique(np.diff(b.off.astype(np.int64))[ti.B_GROUPS_LEAD:], return_counts=True)
    assert ln.tolist() == sorted(ti.B_GROUP_LENGTHS) and (cnt == 128).all()
    # a record of every length in every quarter of a wave (the 16 lanes of quarter g serve records 4 it + g)
    lens = np.diff(b.off.astype(np.int64))
    for L in ti.B_GROUP_LENGTHS:
        assert {int(i) % 4 for i in np.flatnonzero(lens == L)} == {0, 1, 2, 3}


def test_case_c_has_a_uniform_wave_at_every_listed_count():
    b = ti.case_c()
    assert sorted(b.hits["group_counts"]) == list(ti.C_COUNTS) and len(ti.C_COUNTS) == 128
    assert {16 * P for P in range(1, 65)} | {16 * (P - 1) + 1 for P in range(1, 65)} == set(ti.C_COUNTS)
    listed = {c for c in ti.C_COUNTS if trim_ref.FAST_MIN <= c <= trim_ref.FAST_MAX}       # all of them but c = 1
    assert listed == set(ti.C_COUNTS) - {1}
    got = trim_ref.uniform_waves(b.off, b.beg, b.end)
    assert set(got) == listed and len(got) == len(listed)
    ln = np.diff(b.off.astype(np.int64))
    assert ln.max() <= ti.C_MAX_LEN and (b.end.astype(np.int64) <= ln).all() and (b.end > b.beg).all()
    # irregular: within the uniform waves the sources and the read lengths take many values mod 16
    src = b.off[:-1].astype(np.int64) + b.beg
    assert len(set((src % 16).tolist())) == 16 and len(set(ln.tolist())) > 500


def test_case_c_edges_lists_every_edge():
    b = ti.case_c_edges()
    ln = np.diff(b.off.astype(np.int64))
    beg, end = b.beg.astype(np.int64), b.end.astype(np.int64)
    for cond in (beg > ln, end > ln, end < beg, beg == end, (beg == ti.FFFF) & (end == ti.FFFF), (beg == 0) & (end == ti.FFFF)):
        assert cond.any() and (cond & (ln == 0)).any() and (cond & (ln > 16)).any()
    assert trim_ref.uniform_waves(b.off, b.beg, b.end) == []


def test_dev_cases_take_the_paths_they_name():
    for name, want in (("a_150_s5_e140", [135] * 3), ("b_kept16", [16] * 3), ("c_kept1024", [1024] * 3), ("d_kept1025", []),
                       ("e_mixed_0_300", [])):
        b = ti.case_dev(name)
        lo, hi, S, E = ti.DEV_FIXED[name]
        assert len(b.off) - 1 == ti.DEV_N == 193
        assert trim_ref.uniform_waves(b.off, S, E) == want, name
    assert (trim_ref.kept_counts(ti.case_dev("d_kept1025").off, 3, 1028) == 1025).all()
    ln = np.diff(ti.case_dev("e_mixed_0_300").off.astype(np.int64))
    assert ln.min() == 0 and ln.max() > 256


def test_grid_batch_is_larger_than_one_sweep():
    g = ti.case_d_grid()
    assert g.hits["n"] > g.hits["sweep"] + 4096 and trim_ref.uniform_waves(g.off[:GRID_SLICE + 1], *ti.D_GRID_CUT) == []
