"""Deterministic inputs of test_trim_paths_gpu.py (kernels/fastq_trim.hip), shared with test_trim_ref_host.py, which checks on the
CPU that the plain reference agrees with the C oracle on every one of them and that each builder hits the path it is meant to.

Sequence and quality bytes are drawn independently over 0..255 (k_trim_copy never interprets them): a swap of the two arrays, a
shifted piece or a piece of the neighbouring record shows up as wrong bytes.  A builder returns a Batch: the arrays, the points
where the case has its own, and `hits`, a small description of what it is meant to hit.  Builders are cached and their arrays
read-only: the tests share them.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

Batch = namedtuple("Batch", "seq qual off hits beg end", defaults=(None, None))

E_ALL = 2**31 - 1                                            # "to the end of every read" as a fixed cycle

# A: one read length per aligned group of 64 records
A_LENGTHS = tuple(range(0, 1041)) + (1279, 1280, 1281, 2053, 4100)
A_CUTS = ((0, E_ALL), (3, E_ALL))
A2_N, A2_LEN = 129, 1100                                     # two uniform waves and a one-record tail wave
A2_KEPT = (15, 16, 17, 31, 32, 33, 47, 48, 49, 1007, 1008, 1009, 1023, 1024, 1025)
A2_S = (0, 1, 15, 16, 17)
# B: the same lengths with no uniform wave
B_PREFIX = (1, 17, 63)
B_GROUP_LENGTHS = (15, 16, 17, 255, 256, 257, 271, 272, 273, 511, 512, 513, 1024, 1025)
B_GROUPS_LEAD = 20                                           # records of 5 bytes in front: no group of 65 then holds a whole wave
# C: one kept count per aligned group under per-record points
C_COUNTS = tuple(sorted({16 * P for P in range(1, 65)} | {16 * (P - 1) + 1 for P in range(1, 65)}))
C_MAX_LEN = 1200
# D: scan tiles of 4096 records, and the grid of the copy (n_cu * 8 workgroups of 256 records)
D_SEAMS = (0, 1, 4095, 4096, 4097, 8191, 8192, 8193, 12288)
D_SEAM_CUT, D_LEAD = (1, 3), 5
D_GRID_CUT, D_GRID_T, GRID_CUS = (2, 30), 70, 256            # (an MI355X has 256 CUs; the GPU test asks the device)
# E: the device entry points
DEV_N = 64 * 3 + 1
DEV_FIXED = {"a_150_s5_e140": (150, 150, 5, 140), "b_kept16": (150, 150, 5, 21), "c_kept1024": (1100, 1100, 3, 1027),
             "d_kept1025": (1100, 1100, 3, 1028), "e_mixed_0_300": (0, 300, 2, 250)}      # name -> (len lo, len hi, S, E)
# F: k_qtrim_points, directed
F_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 1000)
F_T = (1, 53, 128, 255)
F_RANDOM_T = (0, 200, 256, 0xFFFFFFFF)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def _offsets(lens, lead=0):
    return (lead + np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))])).astype(np.uint64)


def _batch(rng, lens, hits, beg=None, end=None, lead=0):
    """Records of the given lengths behind `lead` bytes that belong to no record."""
    off = _offsets(lens, lead)
    tot = int(off[-1])
    seq, qual = rng.integers(0, 256, tot, dtype=np.uint8), rng.integers(0, 256, tot, dtype=np.uint8)
    return Batch(*_ro(seq, qual, off), hits, *_ro(beg, end))


# ---- A ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case_a(prefix=0):
    """Aligned group g of 64 records has one read length; the groups in a fixed shuffled order.  With `prefix` records of 5
    bytes in front (case B) every wave straddles two groups of different lengths."""
    rng = np.random.default_rng(20240 + prefix)
    groups = np.random.default_rng(7).permutation(np.array(A_LENGTHS))
    lens = np.concatenate([np.full(prefix, 5), np.repeat(groups, 64)])
    return _batch(rng, lens, {"group_lengths": groups.tolist(), "prefix": prefix})


@lru_cache(maxsize=None)
def case_a2():
    """129 reads of 1100 bytes: waves 0 and 1 are uniform at every cut, wave 2 holds one record."""
    return _batch(np.random.default_rng(20241), np.full(A2_N, A2_LEN), {"n": A2_N, "len": A2_LEN})


# ---- B ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case_b_groups():
    """Groups of 65 and then of 63 equal-length records: every quarter of a wave and every 16-lane position meets every length,
    and no wave holds 64 equal records (a group of 63 cannot; a group of 65 starts at record 20 + 65 j, which is 0 or 63 mod 64
    only from j = 43 on)."""
    lens = np.concatenate([np.full(B_GROUPS_LEAD, 5)] + [np.full(65, L) for L in B_GROUP_LENGTHS] + [np.full(63, L) for L in B_GROUP_LENGTHS])
    return _batch(np.random.default_rng(20242), lens, {"lengths": list(B_GROUP_LENGTHS)})


# ---- C ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case_c():
    """Reads of random length; aligned group g keeps one count c from its own random begin: equal counts, irregular sources and
    destinations."""
    rng = np.random.default_rng(20243)
    counts = rng.permutation(np.array(C_COUNTS))
    c = np.repeat(counts, 64)
    lens = rng.integers(c, C_MAX_LEN + 1)
    beg = rng.integers(0, lens - c + 1)
    return _batch(rng, lens, {"group_counts": counts.tolist()}, beg.astype(np.uint32), (beg + c).astype(np.uint32))


C_EDGE_LENGTHS = (0, 1, 15, 16, 17, 40, 0, 100, 300)
FFFF = 0xFFFFFFFF


def _edge_points(ln):
    """(what, beg, end) for a read of `ln` bytes."""
    return (("beg > len", ln + 1, ln + 5), ("end > len", min(2, ln), ln + 7), ("end < beg", 5, 2), ("beg == end", 3, 3),
            ("beg = end = 0xffffffff", FFFF, FFFF), ("beg = 0, end = 0xffffffff", 0, FFFF), ("end < beg, both past the end", FFFF, ln + 1))


@lru_cache(maxsize=None)
def case_c_edges():
    """Every point edge at every length, zero-length reads among them."""
    rows = [(ln,) + p for ln in C_EDGE_LENGTHS for p in _edge_points(ln)]
    lens = [r[0] for r in rows]
    beg, end = np.array([r[2] for r in rows], np.uint32), np.array([r[3] for r in rows], np.uint32)
    return _batch(np.random.default_rng(20244), lens, {"edges": [r[1] for r in rows]}, beg, end)


# ---- D ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case_d_seam(n):
    """n + 5 records of 0..3 bytes behind 11 unused bytes: the tests cut the window off[5:] of it, and the same n records again
    as a batch of their own with off[0] = 0 (`own`)."""
    b = _batch(np.random.default_rng(20250 + n), np.random.default_rng(n).integers(0, 4, n + D_LEAD), {"n": n}, lead=11)
    return b


def own(b, skip):
    """Records skip.. of a batch as a batch of their own: off[0] = 0, arrays that hold nothing else."""
    o = b.off[skip:]
    lo, hi = int(o[0]), int(o[-1])
    return Batch(*_ro(b.seq[lo:hi].copy(), b.qual[lo:hi].copy(), o - o[0]), b.hits)


@lru_cache(maxsize=None)
def case_d_grid(n_cu=GRID_CUS):
    """One grid sweep of k_trim_copy and of k_qtrim_points (n_cu * 8 workgroups of 256 records), a scan tile and 77 records more:
    mixed lengths 0..40."""
    n = n_cu * 8 * 256 + 4096 + 77
    rng = np.random.default_rng(20260)
    return _batch(rng, rng.integers(0, 41, n), {"n": n, "sweep": n_cu * 8 * 256})


# ---- E ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case_dev(name):
    lo, hi, S, E = DEV_FIXED[name]
    rng = np.random.default_rng(20270 + sorted(DEV_FIXED).index(name))
    return _batch(rng, rng.integers(lo, hi + 1, DEV_N), {"S": S, "E": E, "kept": E - S if lo == hi else None})


# ---- F ----------------------------------------------------------------------------------------------------------------------
def _f_positions(ln):
    return sorted({p for p in (0, 1, 62, 63, 64, 65, 127, 128, ln - 2, ln - 1) if 0 <= p < ln})


@lru_cache(maxsize=None)
def case_f_directed(T):
    """Per length: no hit, all hits, one hit at each position of _f_positions, and every pair of them.  A hit byte is T exactly,
    every other quality byte T - 1."""
    rows = []                                                # (len, hit positions or None = all)
    for ln in F_LENGTHS:
        ps = _f_positions(ln)
        rows += [(ln, ()), (ln, None)] + [(ln, (p,)) for p in ps] + [(ln, (p, q)) for i, p in enumerate(ps) for q in ps[i + 1:]]
    b = _batch(np.random.default_rng(20280 + T), [r[0] for r in rows], None)
    qual = np.full(len(b.qual), T - 1, np.uint8)
    o = b.off.astype(np.int64)
    for i, (ln, ps) in enumerate(rows):
        if ps is None:
            qual[o[i]:o[i + 1]] = T
        else:
            qual[o[i] + np.array(ps, np.int64)] = T
    return Batch(b.seq, *_ro(qual), b.off, {"rows": rows, "T": T})


@lru_cache(maxsize=None)
def case_f_random():
    rng = np.random.default_rng(20290)
    return _batch(rng, rng.integers(0, 400, 3000), {})


# ---- the registries both test files walk --------------------------------------------------------------------------------------
def fixed_cases():
    """name -> (builder, S, E) of every fixed-cycle run of the GPU file (case D's seams and grid apart)."""
    cases = {f"A S={S}": (case_a, S, E) for S, E in A_CUTS}
    cases.update({f"A2 kept={k} S={S}": (case_a2, S, S + k) for k in A2_KEPT for S in A2_S})
    cases.update({f"B prefix={p}": ((lambda p=p: case_a(p)), 0, E_ALL) for p in B_PREFIX})
    cases["B groups"] = (case_b_groups, 0, E_ALL)
    cases.update({f"E {name}": ((lambda name=name: case_dev(name)), v[2], v[3]) for name, v in DEV_FIXED.items()})
    return cases


def points_cases():
    return {"C": case_c, "C edges": case_c_edges}
