"""GPU: k_bedgraph_text on every formatting path and seam.  The inputs are run lists designed in bedgraph_paths.py (and proved
to be what they are meant to be by test_bedgraph_paths_host.py); the device's text is compared with "%s\\t%d\\t%d\\t%d\\n" over
the DESIGNED runs and with the reference's fprintf over the same list, never with runs read back from the device.  A wrong byte
is reported with its line, its wave and the path the kernel took for that wave."""
import ctypes as C

import numpy as np
import pytest

import bedgraph_paths as BP

pytestmark = pytest.mark.gpu
W = 1 << 20                       # (the window sums are not what is tested: few windows)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def scan(ctx, inp):
    """The designed runs through the depth kernels: they must come back as designed."""
    runs, _ = ctx.depth_target(BP.soa_for_runs(inp.runs, inp.refs), 0, inp.tlen, W)
    assert np.array_equal(runs, inp.runs), (len(runs), len(inp.runs))


def device_text_info(ctx):
    d_text, nb = C.c_void_p(), C.c_uint64(0)
    assert ctx.L.hpn_depth_bedgraph_dev(ctx.h, C.byref(d_text), C.byref(nb)) == 0
    return d_text, nb.value


@pytest.mark.parametrize("key", BP.KEYS)
def test_text_of_the_designed_runs_under_every_name(ctx, key):
    inp = BP.inputs()[key]
    scan(ctx, inp)
    for name in inp.names:                                        # several names in a row on the same runs
        want = BP.fmt_text(name, inp.runs)
        assert BP.oracle_text(name, inp.runs) == want
        BP.check_text(ctx.depth_bedgraph(name), name, inp.runs, want)


def test_a_new_text_replaces_the_one_before(ctx):
    """hpn_depth_bedgraph_format replaces the text: a short text behind a long one, and an empty one behind a text, leave nothing of
    the text before readable and n_bytes shrinks."""
    ins = BP.inputs()
    inp = ins["tail16"]
    scan(ctx, inp)
    long_name, short_name = "L" * 200, "c"
    BP.check_text(ctx.depth_bedgraph(long_name), long_name, inp.runs)
    n_long = device_text_info(ctx)[1]
    assert n_long == len(BP.fmt_text(long_name, inp.runs))
    BP.check_text(ctx.depth_bedgraph(short_name), short_name, inp.runs)
    n_short = device_text_info(ctx)[1]
    assert n_short == len(BP.fmt_text(short_name, inp.runs)) < n_long
    buf = np.zeros(n_long, np.uint8)
    assert ctx.L.hpn_depth_bedgraph_read(ctx.h, 0, buf.ctypes.data, n_long) != 0          # the long text is gone
    assert ctx.L.hpn_depth_bedgraph_read(ctx.h, n_short, buf.ctypes.data, 1) != 0
    one = ins["count01"]                                         # fewer runs on the same context: one line
    scan(ctx, one)
    BP.check_text(ctx.depth_bedgraph("chr10"), "chr10", one.runs)
    assert device_text_info(ctx)[1] == len(BP.fmt_text("chr10", one.runs))
    none = ins["count00"]
    scan(ctx, none)
    assert ctx.depth_bedgraph_format("chr10") == 0 and ctx.depth_bedgraph("chr10") == b""
    assert device_text_info(ctx)[1] == 0
    assert ctx.L.hpn_depth_bedgraph_read(ctx.h, 0, buf.ctypes.data, 1) != 0
    scan(ctx, inp)                                               # and a long text behind the empty one
    BP.check_text(ctx.depth_bedgraph(long_name), long_name, inp.runs)


def test_read_at_odd_offsets_and_through_the_device_pointer(ctx):
    inp = BP.inputs()["words_tail127"]
    scan(ctx, inp)
    want = BP.fmt_text("chr10", inp.runs)
    n = ctx.depth_bedgraph_format("chr10")
    assert n == len(want)
    for off, ln in [(0, 0), (0, 1), (1, 1), (3, 17), (7, 4097), (n - 1, 1), (n, 0), (n // 2 + 1, n - n // 2 - 1), (13, n - 13), (0, n)]:
        buf = np.full(ln + 2, 0xEE, np.uint8)
        assert ctx.L.hpn_depth_bedgraph_read(ctx.h, off, buf[1:].ctypes.data, ln) == 0, (off, ln)
        assert buf[1:ln + 1].tobytes() == want[off:off + ln], (off, ln)
        assert buf[0] == 0xEE and buf[ln + 1] == 0xEE, (off, ln)     # nothing beside what was asked for
    assert ctx.L.hpn_depth_bedgraph_read(ctx.h, n - 1, buf.ctypes.data, 2) != 0
    d_text, nb = device_text_info(ctx)
    assert nb == n and d_text.value
    out = np.zeros(n, np.uint8)
    assert ctx.L.hpn_memcpy_d2h(ctx.h, out.ctypes.data, d_text, n) == 0
    ctx.sync()
    BP.check_text(out.tobytes(), "chr10", inp.runs, want)
