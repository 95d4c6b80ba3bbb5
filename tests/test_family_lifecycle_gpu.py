"""GPU: the life cycle of the states a context owns -- the nine store families (hpn_fastq_uniq_*, _uniqq_*, _usort_*, _sort_*,
_pair_*, hpn_twobit_pack_*, hpn_mrle_*, hpn_rfastqc_*, hpn_kseq_*), hpn_bam_split_* and the four record-store sessions
(hpn_bam_sort_*, _rmdup_*, _merge_*, _fixmate_*) -- with
contexts of the test's own: a context closed behind a whole session and a second one on the same device, _begin twice, and
contexts closed with sessions at every stage (after _add, after _finish with the output unfetched, three families open at once;
the split session mid-run and finished; the record-store sessions after one batch, finished, between two slices with a block
open -- fixmate's with its patch pointing back into the state that goes --, and behind the last slice with its stored image made).  The inputs are test_store_session_gpu.py's three records (ten for
usort) and the general cases of the BAM families; expected bytes are the Python restatements', never the library's.  Every step
runs once."""
import functools

import numpy as np
import pytest

import bammerge_inputs
import bammerge_ref
import bamsort_inputs
import bamsort_ref
import fixmate_inputs
import fixmate_ref
import rmdup_inputs
import rqc_ref
import split_inputs
import split_ref
import test_bammerge_gpu as TM
import test_fixmate_gpu as TF
import test_rmdup_gpu as TR
import test_split_gpu as TS
from bam_session import FAMILIES as BAM_FAMILIES, blocks_of_records, emit_all, feed
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


# ---- hpn_bam_sort_*, _rmdup_*, _merge_* and _fixmate_*: the record store and the slices ---------------------------------------
PER = 7      # records a slice: a block stays open between slices


class BamSession:
    """a family of bam_session.FAMILIES over one general input.  files: per input file its records; order: the output's, as
    session ordinals; out: the output's records as bytes, if they are not the stored ones"""
    out = None

    def begin(self, ctx):
        getattr(ctx, "bam_%s_begin" % self.family)()

    def next_file(self, ctx):
        pass

    def feed(self, ctx, upto, cuts):
        """the session's stream up to byte `upto`, file by file, in batches that end at `cuts` -> (the last info, the records of
        every file's last batch)"""
        at, info, n = 0, None, 0
        for f in self.files:
            if at >= upto:
                break
            self.next_file(ctx)
            info = feed(ctx, getattr(ctx, "bam_%s_add_raw_dev" % self.family), b"".join(f)[:upto - at], {c - at for c in cuts})
            at, n = at + sum(len(r) for r in f), n + info.n_records
        return info, n

    def finish(self, ctx):
        res = getattr(ctx, "bam_%s_finish" % self.family)()
        assert (res.n_records, res.bad_record) == (len(self.raw), -1)
        return res

    def emit(self, ctx, first, cnt, last):
        return getattr(ctx, "bam_%s_emit" % self.family)(first, cnt, last)


class SortSession(BamSession):
    """bamsort_inputs' "strands" through hpn_bam_sort_*; want: the blocks bamsort_ref cuts of the model's order, and their stored image"""
    family = "sort"

    def __init__(self):
        self.files = [bamsort_ref.parse(bamsort_inputs.own_inputs()["strands"]).recs]
        self.order = list(np.argsort(bamsort_ref.model_keys(self.files[0]), kind="stable"))


class RmdupSession(BamSession):
    """rmdup_inputs' "mixed" through hpn_bam_rmdup_*; want: the same of rmdup_ref's plan"""
    family = "rmdup"

    def __init__(self):
        self.model = TR.Model(rmdup_inputs.own_inputs()["mixed"])
        self.files = [self.model.raw]
        self.order, _, _, bad = self.model.plan()
        assert bad is None

    def begin(self, ctx):
        self.model.begin(ctx)

    def finish(self, ctx):
        res = super().finish(ctx)
        assert res.n_out == len(self.order)
        return res


class MergeSession(BamSession):
    """bammerge_inputs' "unsorted_all", three files, through hpn_bam_merge_*; want: the same of the heap's order"""
    family = "merge"

    def __init__(self):
        self.files = [bammerge_ref.parse(f).recs for f in bammerge_inputs.own_sets()["unsorted_all"]]
        assert len(self.files) == 3 and all(len(f) > 20 for f in self.files)
        self.order, self.lifted, _ = TM.restated(self.files)

    def next_file(self, ctx):
        ctx.bam_merge_next_file()

    def finish(self, ctx):
        res = super().finish(ctx)
        assert (res.n_files, res.n_lifted) == (3, self.lifted)
        return res


class FixmateSession(BamSession):
    """fixmate_inputs' "run_lengths" through hpn_bam_fixmate_* -- of the device's cases that write more than 2 * PER records and add a
    CT field the smallest in bytes, so SliceOut's `extra` and `patch` are live at every stage; want: the blocks of fixmate_ref's
    rewritten records"""
    family = "fixmate"

    def __init__(self):
        recs, self.target_len = TF.parsed(fixmate_inputs.own_inputs()["run_lengths"])
        self.files = [recs]
        written, n = fixmate_ref.machine(recs, self.target_len, False)
        self.order, self.out, self.counts = [i for i, _ in written], [r for _, r in written], n
        assert n["tags"] >= 1 and n["added"] > 0 and any(r != recs[i] for i, r in written[:PER]) and any(r != recs[i] for i, r in written[PER:])

    def begin(self, ctx):
        ctx.bam_fixmate_begin(False, self.target_len)

    def finish(self, ctx):
        res = super().finish(ctx)
        assert (res.n_out, res.n_tags, res.bytes_added) == (len(self.order), self.counts["tags"], self.counts["added"])
        return res


@functools.lru_cache(maxsize=None)
def bam_session(name):
    s = {"sort": SortSession, "rmdup": RmdupSession, "merge": MergeSession, "fixmate": FixmateSession}[name]()
    s.raw = [r for f in s.files for r in f]
    s.stream = b"".join(s.raw)
    s.half = sum(len(r) for r in s.raw[:len(s.raw) // 2])      # a record boundary: the stream up to it is a stream
    s.want = blocks_of_records(s.out if s.out is not None else [s.raw[i] for i in s.order])
    s.want_image = b"".join(bamsort_ref.member(p, 0) for p, _ in s.want)
    assert len(s.order) > 2 * PER and len(s.want) >= 1
    return s


def fed_and_finished(ctx, s):
    """two batches (of the file it lies in), the cut inside a record -> the records to emit"""
    s.begin(ctx)
    info, _ = s.feed(ctx, len(s.stream), {s.half + 9})
    assert info.bad_record == -1 and info.store_bytes == len(s.stream)
    res = s.finish(ctx)
    assert res.payload_bytes == sum(len(p) for p, _ in s.want)
    return res.n_out if hasattr(res, "n_out") else res.n_records


def whole_bam_session(ctx, s):
    return emit_all(ctx, s.family, fed_and_finished(ctx, s), PER, stored=True)


four = pytest.mark.parametrize("name", BAM_FAMILIES)


def test_the_table_has_the_four_bam_families():
    assert [bam_session(n).family for n in BAM_FAMILIES] == list(BAM_FAMILIES)


@four
def test_bam_context_closed_after_one_add(name):
    s = bam_session(name)
    ctx = new_ctx()
    s.begin(ctx)
    info, n = s.feed(ctx, s.half, set())
    assert info.bad_record == -1 and n == len(s.raw) // 2 and info.store_bytes == s.half
    ctx.close()


@four
def test_bam_context_closed_after_finish_with_nothing_emitted(name):
    s = bam_session(name)
    ctx = new_ctx()
    assert fed_and_finished(ctx, s) == len(s.order)
    ctx.close()


@four
def test_bam_context_closed_between_two_slices_with_a_block_open(name):
    s = bam_session(name)
    ctx = new_ctx()
    n = fed_and_finished(ctx, s)
    info = s.emit(ctx, 0, PER, False)
    assert info.n_records == PER and info.open_bytes > 0
    assert n > PER
    ctx.close()


@four
def test_bam_context_closed_behind_the_last_slice_with_the_stored_image_made(name):
    s = bam_session(name)
    ctx = new_ctx()
    blocks, image = whole_bam_session(ctx, s)
    ctx.close()
    assert blocks == s.want and image == s.want_image


@four
def test_bam_begin_one_add_begin_again_then_a_whole_session(name):
    s = bam_session(name)
    ctx = new_ctx()
    s.begin(ctx)
    assert s.feed(ctx, s.half, set())[0].store_bytes == s.half
    again = whole_bam_session(ctx, s)
    ctx.close()
    fresh = new_ctx()
    first = whole_bam_session(fresh, s)
    fresh.close()
    assert again == first == (s.want, s.want_image)
