"""GPU: the life cycle of the hpn_bam_view_* session and the words it refuses a call with -- hpn_ctx_last_error's, which HpnError
carries: calls before _begin, calls before and behind _finish, _finish twice, a slice that is not the next one, a BAM call on a
text session and the reverse, every call on a session a record outside the domain has killed; behind the refusals a fresh _begin
on the same context runs a whole session to the restated bytes."""
import pytest

import view_inputs
import view_ref
from bam_session import feed
from test_family_lifecycle_gpu import new_ctx

pytestmark = pytest.mark.gpu


def test_every_refusal_says_what_it_is():
    import highperformancengs_amd as hp
    from highperformancengs_amd import _lib
    inputs = view_inputs.inputs()
    p = view_ref.parse(inputs["lengths"])
    recs, names = p.recs, [nm for nm, _ in p.targets]
    want = b"".join(view_ref.format_line(r, p.targets, 0) + b"\n" for r in recs)
    ctx = new_ctx()

    def refused(words, f, *args):
        with pytest.raises(hp.HpnError) as e:
            f(*args)
        arg = "slice from record" in words or "entries asked for" in words       # (a wrong slice or count is a bad argument, as the siblings')
        assert e.value.status == (_lib.E_ARG if arg else _lib.E_STATE), str(e.value)
        assert str(e.value).endswith(" " + words), (words, str(e.value))

    def whole_text():
        ctx.bam_view_begin(ctx.VIEW_TEXT, target_names=names)
        assert feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), {len(recs[0]) + 9}).bad_record == -1
        return ctx.bam_view_finish()

    try:
        refused("hpn_bam_view_add_raw_dev before hpn_bam_view_begin", ctx.bam_view_add_raw_dev, None)
        refused("hpn_bam_view_finish before hpn_bam_view_begin", ctx.bam_view_finish)
        refused("hpn_bam_view_text_emit before hpn_bam_view_begin", ctx.bam_view_text, 0, 1)
        refused("hpn_bam_view_emit before hpn_bam_view_begin", ctx.bam_view_emit, 0, 1, True)
        ctx.bam_view_begin(ctx.VIEW_TEXT, target_names=names)
        assert feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), ()).bad_record == -1
        refused("hpn_bam_view_text_emit before hpn_bam_view_finish", ctx.bam_view_text, 0, 1)
        refused("hpn_bam_view_order before hpn_bam_view_finish", ctx.bam_view_order, 1)
        refused("hpn_bam_view_emit before hpn_bam_view_finish", ctx.bam_view_emit, 0, 1, True)
        res = ctx.bam_view_finish()
        assert res.n_out == len(recs)
        refused("hpn_bam_view_add_raw_dev behind hpn_bam_view_finish", ctx.bam_view_add_raw_dev, None)
        refused("hpn_bam_view_finish twice", ctx.bam_view_finish)
        refused("hpn_bam_view_text_emit: slice from record 1, the next one is 0", ctx.bam_view_text, 1, 1)
        # a BAM call on a text session
        refused("hpn_bam_view_emit on a session that emits text", ctx.bam_view_emit, 0, 1, True)
        refused("hpn_bam_view_blocks on a session that emits text", ctx.bam_view_blocks, 1)
        refused("hpn_bam_view_payload_dev on a session that emits text", ctx.bam_view_payload)
        refused("hpn_bam_view_stored_dev on a session that emits text", ctx.bam_view_stored)
        refused("hpn_bam_view_order: %d entries asked for, the output has %d records" % (res.n_out + 1, res.n_out), ctx.bam_view_order, res.n_out + 1)
        assert ctx.bam_view_text(0, 1 << 30)[1] == want
        # a text call on a BAM session and on a count session
        for emit, says in ((ctx.VIEW_BAM, "BAM"), (ctx.VIEW_COUNT, "the count only")):
            ctx.bam_view_begin(emit)
            feed(ctx, ctx.bam_view_add_raw_dev, b"".join(recs), ())
            assert ctx.bam_view_finish().n_out == len(recs)
            refused("hpn_bam_view_text_emit on a session that emits " + says, ctx.bam_view_text, 0, 1)
        refused("hpn_bam_view_emit on a session that emits the count only", ctx.bam_view_emit, 0, 1, True)
        # a killed session says so on every later call
        bad = view_ref.parse(inputs["aux_float"])
        ctx.bam_view_begin(ctx.VIEW_TEXT, target_names=names)
        info = feed(ctx, ctx.bam_view_add_raw_dev, b"".join(bad.recs), ())
        assert info.bad_record == 20 and info.reason == 1
        assert ctx.bam_view_add_raw_dev(None).bad_record == 20
        res = ctx.bam_view_finish()
        assert (res.bad_record, res.reason, res.n_out) == (20, 1, 0)
        for f, args in ((ctx.bam_view_text, (0, 1)), (ctx.bam_view_order, (0,))):
            refused("a record lies outside the domain, nothing was kept", f, *args)
        # a second session after a killed one is clean
        assert whole_text().n_out == len(recs) and ctx.bam_view_text(0, 1 << 30)[1] == want
    finally:
        ctx.close()
