"""GPU: the one life cycle of the four record-store sessions (hpn_bam_sort_*, _rmdup_*, _merge_*, _fixmate_*) and the words each
family refuses a call with -- hpn_ctx_last_error's, which HpnError carries -- as the C ABI has said them since each family arrived:
calls before _begin, calls before and behind _finish, _finish twice, a slice that is not the next one, a slice behind the one that
ended the file, _order with another count than the output's, and _emit on a session a record outside the domain has killed.  The
sessions are tests/test_family_lifecycle_gpu.py's; behind the refusals a fresh _begin on the same context runs a whole session to
the restated bytes."""
import pytest

import bammerge_inputs
import bammerge_ref
import bamsort_inputs
import bamsort_ref
import fixmate_inputs
import rmdup_inputs
import test_fixmate_gpu as TF
import test_rmdup_gpu as TR
from bam_session import FAMILIES, feed
from test_family_lifecycle_gpu import bam_session, new_ctx, whole_bam_session

pytestmark = pytest.mark.gpu

# {n}: the session's output records; {m}: n + 1, what _order is asked for
WORDS = {
    "sort": {
        "add_before_begin": "hpn_bam_sort_add_raw_dev before hpn_bam_sort_begin",
        "finish_before_begin": "hpn_bam_sort_finish before hpn_bam_sort_begin",
        "emit_before_begin": "hpn_bam_sort_emit before hpn_bam_sort_begin",
        "emit_before_finish": "hpn_bam_sort_emit before hpn_bam_sort_finish",
        "order_before_finish": "hpn_bam_sort_order before hpn_bam_sort_finish",
        "blocks_before_finish": "hpn_bam_sort_blocks before hpn_bam_sort_finish",
        "payload_before_finish": "hpn_bam_sort_payload_dev before hpn_bam_sort_finish",
        "stored_before_finish": "hpn_bam_sort_stored_dev before hpn_bam_sort_finish",
        "add_behind_finish": "hpn_bam_sort_add_raw_dev behind hpn_bam_sort_finish",
        "finish_twice": "hpn_bam_sort_finish twice",
        "emit_wrong_record": "hpn_bam_sort_emit: slice from record 1, the next one is 0 (the open block is carried from slice to slice)",
        "emit_behind_the_end": "hpn_bam_sort_emit behind the call that ended the file",
        "order_wrong_n": "hpn_bam_sort_order: {m} entries asked for, the session holds {n} records",
        "emit_killed": "hpn_bam_sort_emit: a record lies outside the domain, nothing was sorted",
    },
    "rmdup": {
        "add_before_begin": "hpn_bam_rmdup_add_raw_dev before hpn_bam_rmdup_begin",
        "finish_before_begin": "hpn_bam_rmdup_finish before hpn_bam_rmdup_begin",
        "emit_before_begin": "hpn_bam_rmdup_emit before hpn_bam_rmdup_begin",
        "emit_before_finish": "hpn_bam_rmdup_emit before hpn_bam_rmdup_finish",
        "order_before_finish": "hpn_bam_rmdup_order before hpn_bam_rmdup_finish",
        "blocks_before_finish": "hpn_bam_rmdup_blocks before hpn_bam_rmdup_finish",
        "payload_before_finish": "hpn_bam_rmdup_payload_dev before hpn_bam_rmdup_finish",
        "stored_before_finish": "hpn_bam_rmdup_stored_dev before hpn_bam_rmdup_finish",
        "add_behind_finish": "hpn_bam_rmdup_add_raw_dev behind hpn_bam_rmdup_finish",
        "finish_twice": "hpn_bam_rmdup_finish twice",
        "emit_wrong_record": "hpn_bam_rmdup_emit: slice from record 1, the next one is 0 (the open block is carried from slice to slice)",
        "emit_behind_the_end": "hpn_bam_rmdup_emit behind the call that ended the file",
        "order_wrong_n": "hpn_bam_rmdup_order: {m} entries asked for, {n} records survive",
        "emit_killed": "hpn_bam_rmdup_emit: a record lies outside the domain, nothing was decided",
    },
    "merge": {
        "add_before_begin": "hpn_bam_merge_add_raw_dev before hpn_bam_merge_begin",
        "finish_before_begin": "hpn_bam_merge_finish before hpn_bam_merge_begin",
        "emit_before_begin": "hpn_bam_merge_emit before hpn_bam_merge_begin",
        "emit_before_finish": "hpn_bam_merge_emit before hpn_bam_merge_finish",
        "order_before_finish": "hpn_bam_merge_order before hpn_bam_merge_finish",
        "blocks_before_finish": "hpn_bam_merge_blocks before hpn_bam_merge_finish",
        "payload_before_finish": "hpn_bam_merge_payload_dev before hpn_bam_merge_finish",
        "stored_before_finish": "hpn_bam_merge_stored_dev before hpn_bam_merge_finish",
        "add_behind_finish": "hpn_bam_merge_add_raw_dev behind hpn_bam_merge_finish",
        "finish_twice": "hpn_bam_merge_finish twice",
        "emit_wrong_record": "hpn_bam_merge_emit: slice from record 1, the next one is 0 (the open block is carried from slice to slice)",
        "emit_behind_the_end": "hpn_bam_merge_emit behind the call that ended the file",
        "order_wrong_n": "hpn_bam_merge_order: {m} entries asked for, the session holds {n} records",
        "emit_killed": "hpn_bam_merge_emit: a record lies outside the domain, nothing was merged",
    },
    "fixmate": {
        "add_before_begin": "hpn_bam_fixmate_add_raw_dev before hpn_bam_fixmate_begin",
        "finish_before_begin": "hpn_bam_fixmate_finish before hpn_bam_fixmate_begin",
        "emit_before_begin": "hpn_bam_fixmate_emit before hpn_bam_fixmate_begin",
        "emit_before_finish": "hpn_bam_fixmate_emit before hpn_bam_fixmate_finish",
        "order_before_finish": "hpn_bam_fixmate_order before hpn_bam_fixmate_finish",
        "blocks_before_finish": "hpn_bam_fixmate_blocks before hpn_bam_fixmate_finish",
        "payload_before_finish": "hpn_bam_fixmate_payload_dev before hpn_bam_fixmate_finish",
        "stored_before_finish": "hpn_bam_fixmate_stored_dev before hpn_bam_fixmate_finish",
        "add_behind_finish": "hpn_bam_fixmate_add_raw_dev behind hpn_bam_fixmate_finish",
        "finish_twice": "hpn_bam_fixmate_finish twice",
        "emit_wrong_record": "hpn_bam_fixmate_emit: slice from record 1, the next one is 0 (the open block is carried from slice to slice)",
        "emit_behind_the_end": "hpn_bam_fixmate_emit behind the call that ended the file",
        "order_wrong_n": "hpn_bam_fixmate_order: {m} entries asked for, the output has {n} records",
        "emit_killed": "hpn_bam_fixmate_emit: a record lies outside the domain, nothing was fixed",
    },
}


def killed(ctx, family):
    """a session of the family, begun and fed its out-of-domain input -> the info that names the record"""
    add = getattr(ctx, "bam_%s_add_raw_dev" % family)
    if family == "sort":
        ctx.bam_sort_begin()
        return feed(ctx, add, b"".join(bamsort_ref.parse(bamsort_inputs.own_inputs()["pos_out_2p30m1"]).recs), set())
    if family == "rmdup":
        model = TR.Model(rmdup_inputs.own_inputs()["pos_m1"])
        model.begin(ctx)
        return feed(ctx, add, b"".join(model.raw), set())
    if family == "fixmate":
        recs, tl = TF.parsed(fixmate_inputs.own_inputs()["op_ten"])
        ctx.bam_fixmate_begin(False, tl)
        return feed(ctx, add, b"".join(recs), set())
    ctx.bam_merge_begin()
    info = None
    for f in bammerge_inputs.own_sets()["heap_empty_2p31m2"]:
        if info is None or info.bad_record < 0:
            ctx.bam_merge_next_file()
            info = feed(ctx, add, b"".join(bammerge_ref.parse(f).recs), set())
    return info


@pytest.mark.parametrize("family", FAMILIES)
def test_every_refusal_says_what_it_always_said(family):
    import highperformancengs_amd as hp
    s, words = bam_session(family), WORDS[family]
    call = lambda what: getattr(ctx, "bam_%s_%s" % (family, what))

    def refused(key, f, *args, **fmt):
        with pytest.raises(hp.HpnError) as e:
            f(*args)
        assert str(e.value).endswith(" " + words[key].format(**fmt)), (key, str(e.value))

    ctx = new_ctx()
    try:
        refused("add_before_begin", call("add_raw_dev"), None)
        refused("finish_before_begin", call("finish"))
        refused("emit_before_begin", call("emit"), 0, 1, True)
        s.begin(ctx)
        info, _ = s.feed(ctx, len(s.stream), {s.half + 9})
        assert info.bad_record == -1
        refused("emit_before_finish", call("emit"), 0, 1, True)
        refused("order_before_finish", call("order"), 1)
        refused("blocks_before_finish", call("blocks"), 1)
        refused("payload_before_finish", call("payload"))
        refused("stored_before_finish", call("stored"))
        s.finish(ctx)
        n = len(s.order)
        refused("add_behind_finish", call("add_raw_dev"), None)
        refused("finish_twice", call("finish"))
        refused("emit_wrong_record", call("emit"), 1, 1, False)
        refused("order_wrong_n", call("order"), n + 1, n=n, m=n + 1)
        assert list(call("order")(n)) == list(s.order)
        assert s.emit(ctx, 0, n, True).n_records == n
        refused("emit_behind_the_end", call("emit"), n, 0, True)
        bad = killed(ctx, family)
        assert bad is not None and bad.bad_record >= 0
        assert call("finish")().bad_record == bad.bad_record
        refused("emit_killed", call("emit"), 0, 1, True)
        assert whole_bam_session(ctx, s) == (s.want, s.want_image)
    finally:
        ctx.close()
