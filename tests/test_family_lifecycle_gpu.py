"""GPU: the life cycle of the states a context owns -- the nine store families (hpn_fastq_uniq_*, _uniqq_*, _usort_*, _sort_*,
_pair_*, hpn_twobit_pack_*, hpn_mrle_*, hpn_rfastqc_*, hpn_kseq_*) and hpn_bam_split_* -- with contexts of the test's own: a
context closed behind a whole session and a second one on the same device, _begin twice, and contexts closed with sessions at
every stage (after _add, after _finish with the output unfetched, three families open at once; the split session mid-run and
finished).  The inputs are test_store_session_gpu.py's three records (ten for usort); expected bytes are the Python
restatements', never the library's.  Every step runs once."""
import pytest

import rqc_ref
import split_inputs
import split_ref
import test_split_gpu as TS
from highperformancengs_amd import _lib
from test_split_gpu import made      # noqa: F401  (the fixture)
from test_store_session_gpu import FAMILIES, THREE, Family, _grouping

pytestmark = pytest.mark.gpu

RQC_ARRAYS = (_lib.RFASTQC_GC, _lib.RFASTQC_QUALITY, _lib.RFASTQC_NUCLEOTIDE, _lib.RFASTQC_LENGTH)


class Rfastqc(Family):
    """hpn_rfastqc_*: its fourth call reads typed arrays -- the output is the list's elements in the plugin's order, as bytes."""

    def __init__(self):
        want = b"".join(a.tobytes() for a in rqc_ref.elements(rqc_ref.tally(THREE)))
        super().__init__("rfastqc", "hpn_rfastqc", _lib.RfastqcResult, _lib.SortInfo, 1, THREE, want, _grouping, True)

    def output(self, ctx):
        arrays = [ctx.rfastqc_array(_lib.RFASTQC_DUP, slice_elems=4096)] + [ctx.rfastqc_array(w, 0, slice_elems=4096) for w in RQC_ARRAYS]
        return b"".join(a.tobytes() for a in arrays)


ONE_EACH = ("uniq", "uniqq", "usort", "sort", "twobit", "pair", "mrle", "kseq")
NINE = [next(f for f in FAMILIES if f.name == n) for n in ONE_EACH] + [Rfastqc()]
by_name = dict(argvalues=NINE, ids=[f.name for f in NINE])


def new_ctx():
    import highperformancengs_amd as hp
    return hp.Context(0)


def whole_session(ctx, fam):
    fam.begin(ctx)
    fam.feed_all(ctx)
    assert fam.finish(ctx)[0] == 0
    return fam.output(ctx)


def test_the_table_has_the_nine_families():
    assert len({f.prefix for f in NINE}) == 9 and all(f.want for f in NINE)


@pytest.mark.parametrize("fam", **by_name)
def test_a_second_context_gives_the_same_bytes(fam):
    first = new_ctx()
    a = whole_session(first, fam)
    first.close()
    second = new_ctx()
    b = whole_session(second, fam)
    second.close()
    assert a == b == fam.want


@pytest.mark.parametrize("fam", **by_name)
def test_begin_twice_then_a_whole_session(fam):
    ctx = new_ctx()
    fam.begin(ctx)
    got = whole_session(ctx, fam)
    ctx.close()
    assert got == fam.want


@pytest.mark.parametrize("fam", **by_name)
def test_close_after_add(fam):
    ctx = new_ctx()
    fam.begin(ctx)
    rc, info = fam.add(ctx, 0, fam.text, True)
    assert rc == 0 and info.n_records == fam.text.count(b"\n") // 4
    ctx.close()


@pytest.mark.parametrize("fam", **by_name)
def test_close_after_finish_with_the_output_unfetched(fam):
    ctx = new_ctx()
    fam.begin(ctx)
    fam.feed_all(ctx)
    assert fam.finish(ctx)[0] == 0
    ctx.close()


@pytest.mark.parametrize("k", range(len(NINE)), ids=[f.name for f in NINE])
def test_three_families_left_open(k):
    ctx = new_ctx()
    for fam in (NINE[k], NINE[(k + 1) % 9], NINE[(k + 2) % 9]):
        fam.begin(ctx)
        assert fam.add(ctx, 0, fam.text, False)[0] == 0
    ctx.close()


# ---- hpn_bam_split_* ----------------------------------------------------------------------------------------------
SPLIT_CASE = "hdr_notext"      # the smallest of test_split_gpu.SMALL whose first batch leaves a block open on the device


class Stopped(Exception):
    pass


class StopAtSecondBatch:
    """the context as test_split_gpu.abi_split drives it, up to the second hpn_bam_split_add_raw_dev"""

    def __init__(self, ctx):
        self._ctx, self._adds = ctx, 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def split_add_raw_dev(self, d_raw, last=False):
        self._adds += 1
        if self._adds == 2:
            raise Stopped
        info = self._ctx.split_add_raw_dev(d_raw, last)
        assert info.open_bytes > 0
        return info


@pytest.mark.parametrize("level0", [False, True])
def test_split_context_closed_mid_run(made, level0):      # noqa: F811
    bam = split_ref.read(split_inputs.path_of(SPLIT_CASE, made))
    ctx = new_ctx()
    with pytest.raises(Stopped):
        TS.abi_split(StopAtSecondBatch(ctx), bam, set(TS.boundaries(bam)), level0)
    ctx.close()


@pytest.mark.parametrize("level0", [False, True])
def test_split_context_closed_after_finish(made, level0):      # noqa: F811
    bam = split_ref.read(split_inputs.path_of(SPLIT_CASE, made))
    want, wimg = TS.expected(bam)
    ctx = new_ctx()
    blocks, image, counts, bad = TS.abi_split(ctx, bam, set(TS.boundaries(bam)), level0)
    ctx.close()
    assert bad is None and blocks == want and (not level0 or image == wimg)
