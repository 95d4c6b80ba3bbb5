"""References for the K1 / K1L tally tests: numpy restatements of the two per-cycle matrices and the read counts of the
length sweep.  tests/test_tally_ref_host.py holds them against the C oracle, so a GPU test may use either."""
import numpy as np

import orc

LEN_BINS, QUAL_ROWS, NUC_CODES = 512, 128, 5

# The build's defaults in kernels/fastq_tally.hip: a 1024-thread workgroup, HPN_SPAN1 items per set, HPN_SETS sets in the ring.
HIST_THREADS, SPAN1, SETS, HIST_RECS = 1024, 8, 2, 4096

NUC_LUT = np.zeros(256, np.int64)     # Rgzfastq_uniq.c:97-108: T/U 0, C 1, A 2, G 3, N and '.' 4, every other byte 0
for _ch, _v in ((b"tTuU", 0), (b"cC", 1), (b"aA", 2), (b"gG", 3), (b".N", 4)):
    for _c in _ch:
        NUC_LUT[_c] = _v


def _per_cycle(code, off, rows):
    """out[code of byte, cycle of byte] over the bytes [off[0], off[n]); code is indexed like the array off points into."""
    o = off.astype(np.int64)
    lens = np.diff(o)
    pos = np.arange(int(o[-1] - o[0]), dtype=np.int64) - np.repeat(o[:-1] - o[0], lens)
    return np.bincount(code[int(o[0]):int(o[-1])] * LEN_BINS + pos, minlength=rows * LEN_BINS).astype(np.uint64).reshape(rows, LEN_BINS)


def nuc_ref(base, off):
    """Nucleotide[5][512] per Rgzfastq_uniq.c:50-57,97-108."""
    return _per_cycle(NUC_LUT[base], off, NUC_CODES)


def qual_ref(qual, off):
    """Quality[128][512] per fastq_count.c:29-35 (AssignQuality); quality bytes 0..127."""
    return _per_cycle(qual.astype(np.int64), off, QUAL_ROWS)


def counts_for(L):
    """Read counts that take stream_uniform through its shapes at read length L.  A workgroup takes rpr = 1024 // ngr reads per
    round, a set is SPAN1 rounds and the ring holds SETS sets: 1, 2 and SETS + 1 sets, whole and ragged last rounds, a wave with a
    lane that holds a single item of a set (8 = SPAN1, 17 = SETS * SPAN1 + 1); the last count adds an interior chunk, whose
    partial item is loaded whole and reaches into the next read."""
    ngr = (L + 7) // 8
    rpr = HIST_THREADS // ngr
    return [1, rpr - 1, rpr, rpr + 1, SPAN1 * rpr, SPAN1 * rpr + 1, (SETS * SPAN1 + 1) * rpr - 1, HIST_RECS + rpr + 1]


class Want:
    """What every mode of the tally must give for one batch: the C oracle where it applies, numpy beyond."""

    def __init__(self, qual, base, off):
        rc, box = orc.count_soa(qual, off)
        assert rc == 0
        s = box.summary()
        self.seqlen, self.qual_hist = box.seqlen, box.quality
        self.total, self.q20, self.q30 = s.sum, s.q20, s.q30       # q20 / q30: rows >= 53 and >= 63
        lens = np.diff(off.astype(np.int64))
        if base is None:
            self.nuc_hist = None
        elif len(lens) and lens.min() >= 1 and lens.max() <= orc.RQC_MAXLEN:
            rc, r = orc.rqc_soa(base, qual, off)
            assert rc == 0
            self.nuc_hist = np.zeros((NUC_CODES, LEN_BINS), np.uint64)
            self.nuc_hist[:, :orc.RQC_MAXLEN] = r["nucleotide"].T
        else:
            self.nuc_hist = nuc_ref(base, off)
