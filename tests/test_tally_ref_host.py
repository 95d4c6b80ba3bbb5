"""The numpy references of tally_ref.py against the C oracle, on random ragged batches with qualities over 0..127 and bases
over all 256 byte values: two independent statements of the same matrices.  No GPU involved."""
import numpy as np
import pytest

import orc
from tally_ref import LEN_BINS, NUC_CODES, QUAL_ROWS, counts_for, nuc_ref, qual_ref


def _batch(seed, n, lo, hi, lead=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n)
    off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    tot = int(off[-1]) + 5                       # bytes in front of and behind the batch: a reference must not count them
    return rng.integers(0, 128, tot, dtype=np.uint8), rng.integers(0, 256, tot, dtype=np.uint8), off


@pytest.mark.parametrize("n,lo,hi,lead", [(4000, 1, 300, 0), (700, 0, 511, 0), (300, 1, 300, 13), (1, 1, 1, 0), (5, 0, 0, 3)])
def test_qual_ref_is_count_soa(n, lo, hi, lead):
    qual, base, off = _batch(n + lo, n, lo, hi, lead)
    rc, want = orc.count_soa(qual, off)
    assert rc == 0
    got = qual_ref(qual, off)
    assert got.shape == (QUAL_ROWS, LEN_BINS) and got.dtype == np.uint64
    assert np.array_equal(got, want.quality)
    assert int(got.sum()) == int(off[-1] - off[0])


@pytest.mark.parametrize("n,lead", [(4000, 0), (300, 13), (1, 0)])
def test_refs_are_rqc_soa(n, lead):
    qual, base, off = _batch(n, n, 1, orc.RQC_MAXLEN, lead)
    rc, want = orc.rqc_soa(base, qual, off)
    assert rc == 0
    got = nuc_ref(base, off)
    assert got.shape == (NUC_CODES, LEN_BINS) and got.dtype == np.uint64
    assert np.array_equal(got[:, :orc.RQC_MAXLEN], want["nucleotide"].T) and not got[:, orc.RQC_MAXLEN:].any()
    gq = qual_ref(qual, off)
    assert np.array_equal(gq[:, :orc.RQC_MAXLEN], want["quality"].T) and not gq[:, orc.RQC_MAXLEN:].any()


def test_every_base_value_has_the_reference_code():
    base = np.arange(256, dtype=np.uint8)
    got = nuc_ref(base, np.arange(257, dtype=np.uint64))       # 256 reads of one base
    codes = {c: 0 for c in range(256)}
    codes.update({ord(ch): v for chs, v in (("tTuU", 0), ("cC", 1), ("aA", 2), ("gG", 3), (".N", 4)) for ch in chs})
    for v in range(NUC_CODES):
        assert got[v, 0] == sum(1 for c in codes.values() if c == v)
    assert got[:, 1:].sum() == 0
    rc, want = orc.rqc_soa(base, np.zeros(256, np.uint8), np.arange(257, dtype=np.uint64))
    assert rc == 0 and np.array_equal(got[:, 0], want["nucleotide"][0])


def test_counts_for():
    assert counts_for(16) == [1, 511, 512, 513, 4096, 4097, 8703, 4609]          # ngr 2, rpr 512
    assert counts_for(150) == [1, 52, 53, 54, 424, 425, 900, 4150]               # ngr 19, rpr 53
    assert counts_for(256) == [1, 31, 32, 33, 256, 257, 543, 4129]               # ngr 32, rpr 32
    for L in range(16, 257):
        c = counts_for(L)
        assert min(c) == 1 and all(1 <= x < 3 * 4096 for x in c)
