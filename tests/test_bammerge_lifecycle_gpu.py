"""GPU: a context closed at every stage of an hpn_bam_merge_* session frees what the session holds (the family's state is the
context's: csrc/hpn_ctx.hpp), and a session begun over an abandoned one inherits nothing -- as tests/test_family_lifecycle_gpu.py
holds hpn_bam_sort_* and hpn_bam_rmdup_* to."""
import pytest

import bammerge_inputs
import bammerge_ref
import bamsort_ref
from bam_session import emit_all, feed
from test_bammerge_gpu import restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files():
    recs = [bammerge_ref.parse(f).recs for f in bammerge_inputs.own_sets()["unsorted_all"]]
    assert len(recs) == 3 and all(len(f) > 20 for f in recs)
    return recs


def new_ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    return hp.Context(0)


def fed(ctx, files, upto=None):
    """the files (or the first `upto`) into a fresh session, each in two batches cut inside a record"""
    ctx.bam_merge_begin()
    for f in files[:upto]:
        ctx.bam_merge_next_file()
        stream = b"".join(f)
        feed(ctx, ctx.bam_merge_add_raw_dev, stream, {len(stream) // 2 + 3})


def test_context_closed_after_one_file(files):
    c = new_ctx()
    fed(c, files, 1)
    c.close()


def test_context_closed_after_finish_with_nothing_emitted(files):
    c = new_ctx()
    fed(c, files)
    res = c.bam_merge_finish()
    assert res.n_records == sum(len(f) for f in files) and res.n_files == 3
    c.close()


def test_context_closed_between_two_slices_with_a_block_open(files):
    c = new_ctx()
    fed(c, files)
    res = c.bam_merge_finish()
    info = c.bam_merge_emit(0, 10, False)
    assert info.n_records == 10 and info.open_bytes > 0
    c.close()


def test_begin_one_file_begin_again_then_a_whole_session(files):
    want_order, lifted, want = restated(files)
    c = new_ctx()
    try:
        fed(c, files[::-1], 2)            # an abandoned session: other files, in another order
        fed(c, files)
        res = c.bam_merge_finish()
        assert (res.n_records, res.n_files, res.n_lifted, res.bad_record) == (len(want_order), 3, lifted, -1)
        assert list(c.bam_merge_order(res.n_records)) == want_order
        assert emit_all(c, "merge", res.n_records, 50)[0] == want
        image = c.bam_merge_stored()      # the last slice's blocks framed for level 0
        assert image.endswith(bamsort_ref.member(want[-1][0], 0))
    finally:
        c.close()
