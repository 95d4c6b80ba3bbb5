"""K1 `k_tally_scan`: every compiled variant (HPN_K1_VARIANT = unroll * 100 + nt * 10 + sched, HPN_K1_WG_PER_CU) against the
oracle.  The A/B scripts choose between these; only 811 ships.  One child process per variant: the switches live in the
test-hooks library (host/knobs.hpp).  Bit-exact."""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

VARIANTS = [("410", None), ("411", None), ("800", None), ("801", None), ("810", None), ("811", None), ("812", None), ("1610", None),
            ("1611", None), ("812", "1")]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def _env(variant, wg):
    env = {"HPN_K1_VARIANT": variant}
    if wg is not None:
        env["HPN_K1_WG_PER_CU"] = wg
    return env


def _batches():
    rng = np.random.default_rng(812)

    def make(lens):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        return rng.integers(0, 128, int(off[-1]), dtype=np.uint8), off

    # 70,000 x 36 bp: ten chunks of byte tiles and three of pair tiles, so variant 812 places a pair chunk after every three byte
    # chunks (`every` = 4) and both kinds interleave
    yield "70000 x 36", make(np.full(70000, 36))
    qual, off = make(rng.integers(1, 301, 40000))
    yield "40000 x 1..300", (qual, off)
    yield "20011 x 150", make(np.full(20011, 150))
    yield "window off[3:-5] of 40000 x 1..300", (qual, off[3:-5])
    yield "empty", (np.zeros(0, np.uint8), np.zeros(1, np.uint64))


@pytest.mark.parametrize("variant,wg", VARIANTS)
def test_scan_variant(request, variant, wg):
    from conftest import in_hooks_build
    if in_hooks_build(request, _env(variant, wg)):
        return
    ctx = request.getfixturevalue("ctx")
    for name, (qual, off) in _batches():
        rc, want = orc.count_soa(qual, off)
        assert rc == 0
        s = want.summary()
        got = ctx.fastq_tally(qual, off)
        assert np.array_equal(got.seqlen, want.seqlen), f"variant {variant} wg {wg}: {name}: seqlen"
        assert (got.total, got.q20, got.q30) == (s.sum, s.q20, s.q30), f"variant {variant} wg {wg}: {name}: total/q20/q30"


def test_unknown_variant_is_an_error(request):
    """A number that names no compiled kernel comes back as an error from the launch: nothing runs, nothing is defaulted."""
    from conftest import in_hooks_build
    if in_hooks_build(request, _env("813", None)):
        return
    import highperformancengs_amd as hp
    from highperformancengs_amd import _lib
    ctx = request.getfixturevalue("ctx")
    qual, off = np.full(3600, 40, np.uint8), np.arange(0, 3601, 36, dtype=np.uint64)
    with pytest.raises(hp.HpnError) as e:
        ctx.fastq_tally(qual, off)
    assert e.value.status == _lib.E_HIP
    # the histogram kernel does not go through that switch
    got = ctx.fastq_tally(qual, off, qual_hist=True)
    assert got.total == 3600 and got.seqlen[36] == 100
