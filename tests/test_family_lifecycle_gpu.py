"""GPU: the life cycle of the states a context owns -- the nine store families (hpn_fastq_uniq_*, _uniqq_*, _usort_*, _sort_*,
_pair_*, hpn_twobit_pack_*, hpn_mrle_*, hpn_rfastqc_*, hpn_kseq_*), hpn_bam_split_*, hpn_bam_sort_* and hpn_bam_rmdup_* -- with
contexts of the test's own: a context closed behind a whole session and a second one on the same device, _begin twice, and
contexts closed with sessions at every stage (after _add, after _finish with the output unfetched, three families open at once;
the split session mid-run and finished; the sort and rmdup sessions after one batch, finished, between two slices with a block
open, and behind the last slice with its stored image made).  The inputs are test_store_session_gpu.py's three records (ten for
usort) and the general cases of the BAM families; expected bytes are the Python restatements', never the library's.  Every step
runs once."""
import functools

import numpy as np
import pytest

import bamsort_inputs
import bamsort_ref
import rmdup_inputs
import rqc_ref
import split_inputs
import split_ref
import test_bamsort_gpu as TB
import test_rmdup_gpu as TR
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


# ---- hpn_bam_sort_* and hpn_bam_rmdup_*: the record store and the slices -----------------------------------------------------
PER = 7      # records a slice: a block stays open between slices


class SortSession:
    """bamsort_inputs' "strands" through hpn_bam_sort_*; want: the blocks bamsort_ref cuts of the model's order, and their stored image"""

    def __init__(self):
        self.raw = bamsort_ref.parse(bamsort_inputs.own_inputs()["strands"]).recs
        self.order = list(np.argsort(bamsort_ref.model_keys(self.raw), kind="stable"))
        self.feed, self.emit_all = TB.feed, TB.emit_all

    def begin(self, ctx):
        ctx.bam_sort_begin()

    def finish(self, ctx):
        res = ctx.bam_sort_finish()
        assert (res.n_records, res.bad_record) == (len(self.raw), -1)
        return res.n_records

    def emit(self, ctx, first, cnt, last):
        return ctx.bam_sort_emit(first, cnt, last)


class RmdupSession:
    """rmdup_inputs' "mixed" through hpn_bam_rmdup_*; want: the same of rmdup_ref's plan"""

    def __init__(self):
        self.model = TR.Model(rmdup_inputs.own_inputs()["mixed"])
        self.raw = self.model.raw
        self.order, _, _, bad = self.model.plan()
        assert bad is None
        self.feed, self.emit_all = TR.feed, TR.emit_all

    def begin(self, ctx):
        self.model.begin(ctx)

    def finish(self, ctx):
        res = ctx.bam_rmdup_finish()
        assert (res.n_records, res.bad_record, res.n_out) == (len(self.raw), -1, len(self.order))
        return res.n_out

    def emit(self, ctx, first, cnt, last):
        return ctx.bam_rmdup_emit(first, cnt, last)


@functools.lru_cache(maxsize=None)
def bam_session(name):
    s = {"sort": SortSession, "rmdup": RmdupSession}[name]()
    s.stream = b"".join(s.raw)
    s.half = sum(len(r) for r in s.raw[:len(s.raw) // 2])      # a record boundary: the stream up to it is a stream
    s.want = TB.expected_blocks(s.raw, s.order)
    s.want_image = b"".join(bamsort_ref.member(p, 0) for p, _ in s.want)
    assert len(s.order) > 2 * PER and len(s.want) >= 1
    return s


def fed_and_finished(ctx, s):
    """two batches, the cut inside a record -> the records to emit"""
    s.begin(ctx)
    info = s.feed(ctx, s.stream, {s.half + 9})
    assert info.bad_record == -1 and info.store_bytes == len(s.stream)
    return s.finish(ctx)


def whole_bam_session(ctx, s):
    return s.emit_all(ctx, fed_and_finished(ctx, s), PER, stored=True)


both = pytest.mark.parametrize("name", ["sort", "rmdup"])


@both
def test_bam_context_closed_after_one_add(name):
    s = bam_session(name)
    ctx = new_ctx()
    s.begin(ctx)
    info = s.feed(ctx, s.stream[:s.half], set())
    assert info.bad_record == -1 and info.n_records == len(s.raw) // 2 and info.store_bytes == s.half
    ctx.close()


@both
def test_bam_context_closed_after_finish_with_nothing_emitted(name):
    s = bam_session(name)
    ctx = new_ctx()
    assert fed_and_finished(ctx, s) == len(s.order)
    ctx.close()


@both
def test_bam_context_closed_between_two_slices_with_a_block_open(name):
    s = bam_session(name)
    ctx = new_ctx()
    n = fed_and_finished(ctx, s)
    info = s.emit(ctx, 0, PER, False)
    assert info.n_records == PER and info.open_bytes > 0
    assert n > PER
    ctx.close()


@both
def test_bam_context_closed_behind_the_last_slice_with_the_stored_image_made(name):
    s = bam_session(name)
    ctx = new_ctx()
    blocks, image = whole_bam_session(ctx, s)
    ctx.close()
    assert blocks == s.want and image == s.want_image


@both
def test_bam_begin_one_add_begin_again_then_a_whole_session(name):
    s = bam_session(name)
    ctx = new_ctx()
    s.begin(ctx)
    assert s.feed(ctx, s.stream[:s.half], set()).store_bytes == s.half
    again = whole_bam_session(ctx, s)
    ctx.close()
    fresh = new_ctx()
    first = whole_bam_session(fresh, s)
    fresh.close()
    assert again == first == (s.want, s.want_image)
