"""GPU: the device DEFLATE decoders (k_bgzf_inflate, k_gz_sym_inflate: kernels/inflate_core.hpp; the block-start search
k_gz_find_starts) on streams zlib's deflate never writes -- tests/deflate_cases.py, built with tests/deflate_craft.py and held
to zlib's inflate by tests/test_deflate_craft_host.py.  zlib's inflate is the oracle: every accept stream must come out as
zlib's bytes with status 0, every reject stream must be reported, for its block or stretch alone.  Exact equality throughout."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import deflate_cases as cases
import deflate_craft as dc
from conftest import golden_path

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
CHUNK = np.dtype([("in_off", "<u8"), ("end_bit", "<u8"), ("in_len", "<u4"), ("start_bit", "<u4")])
NONE = (1 << 64) - 1
GAP = 64            # bytes of 0xAA between the output ranges of two blocks
REJECT_ROOM = 40000  # what a refused block is allowed to fill before it is refused


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import highperformancengs_amd as hp
    c = hp.Context(0)
    yield c
    c.close()


def _sound(k):
    """zlib-written neighbours: text, at several levels."""
    fq = cases.fastq_text()
    piece = fq[1000 * k:1000 * k + 3000 + 511 * (k % 7)]
    c = zlib.compressobj(1 + k % 9, zlib.DEFLATED, -15)
    return c.compress(piece) + c.flush(), piece


# ---- k_bgzf_inflate: every case a block of ONE launch ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bgzf_launch(ctx):
    """sound, case, sound, case, ... sound: (kind, name, stream, in_len, out_len, want) per block and what the launch left."""
    blocks = []
    for k, c in enumerate(cases.accept_cases()):
        blocks.append(("sound", "zlib%d" % k) + _sound(k))
        junk = bytes([0x55, 0xff, 0, 0x1f, 0x8b, 8, 0, 3]) if k % 3 == 0 else b""      # bytes behind the final block, inside in_len
        blocks.append(("accept", c.name, c.stream + junk, c.want))
    for k, r in enumerate(cases.reject_cases()):
        blocks.append(("sound", "zlib_r%d" % k) + _sound(100 + k))
        blocks.append(("reject", r.name, r.stream, None))
    blocks.append(("sound", "zlib_last") + _sound(7))
    table = np.zeros((len(blocks), 3), np.uint64)
    # (the compressed bytes in block order, but the stream that is cut short last: zeros follow it, which read as a valid
    # distance and an end-of-block code -- the hardest form of that case)
    comp, at = b"", {}
    for i in sorted(range(len(blocks)), key=lambda i: blocks[i][1] == "input_ends_inside_extra_bits"):
        at[i] = len(comp)
        comp += blocks[i][2]
    outo, spans = 0, []
    for i, (kind, name, stream, want) in enumerate(blocks):
        n = len(want) if want is not None else REJECT_ROOM
        table[i] = (at[i], len(stream) | (n << 32), outo)
        spans.append((outo, n))
        outo += n + GAP
    d_comp = torch.from_numpy(np.frombuffer(comp + bytes(64), np.uint8).copy()).cuda()
    d_blocks = torch.from_numpy(table.view(np.int64)).cuda()
    d_out = torch.full((outo + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(blocks),), 999, dtype=torch.int32, device="cuda")
    ctx.bgzf_inflate_dev(d_comp, d_blocks, len(blocks), d_out, d_status)
    ctx.sync()
    return blocks, spans, d_out.cpu().numpy(), d_status.cpu().numpy()


def test_bgzf_blocks_other_encoders_write(bgzf_launch):
    blocks, spans, out, status = bgzf_launch
    wrong = []
    for (kind, name, stream, want), (o, n), st in zip(blocks, spans, status):
        if kind == "reject":
            continue
        if st != 0:
            wrong.append((name, "status", int(st)))
        elif out[o:o + n].tobytes() != want:
            got = out[o:o + n].tobytes()
            first = next(i for i in range(n) if got[i] != want[i])
            wrong.append((name, "bytes differ from", first, "of", n))
    assert not wrong, wrong


# The decoder's code (include/hpngs.h) each reject stream is built to reach.  7 -- a code-length symbol that is no symbol -- has no
# stream: a code-length code that passed the completeness test (6) fills all 128 entries of its table.  12 and 16 (room, ISIZE)
# are test_bgzf_inflate_gpu.py's.
REFUSALS = {"btype_3": 3, "stored_nlen_mismatch": 1, "hlit_field_30": 5, "hlit_field_31": 5, "hdist_field_30": 5, "hdist_field_31": 5,
            "code_length_code_oversubscribed": 6, "code_length_code_incomplete": 6, "repeat_as_first_length": 8, "run_overshoots_by_1": 9,
            "no_end_of_block_code": 10, "literal_code_oversubscribed": 11, "literal_code_incomplete_two_codes": 11,
            "distance_code_incomplete_two_of_2_bits": 11, "unused_half_of_a_single_distance_code": 13,
            "length_without_any_distance_code": 13, "fixed_literal_length_symbol_286": 15, "fixed_literal_length_symbol_287": 15,
            "fixed_distance_symbol_30": 13, "fixed_distance_symbol_31": 13, "distance_one_beyond_the_start": 14,
            "input_ends_inside_extra_bits": 17}


def test_bgzf_blocks_rfc1951_forbids(bgzf_launch):
    """A nonzero status -- the one the stream was built for -- for that block only, its neighbours untouched, nothing written
    behind any block's output range."""
    blocks, spans, out, status = bgzf_launch
    wrong = []
    for i, ((kind, name, stream, want), (o, n), st) in enumerate(zip(blocks, spans, status)):
        if not (out[o + n:o + n + GAP] == 0xAA).all():
            wrong.append((name, "wrote behind its output range"))
        if kind != "reject":
            continue
        if st != REFUSALS[name]:                           # (0: taken)
            wrong.append((name, "status", int(st), "not", REFUSALS[name]))
        for j in (i - 1, i + 1):                            # its neighbours: untouched
            (k2, n2, s2, w2), (o2, m2) = blocks[j], spans[j]
            if status[j] != 0 or out[o2:o2 + m2].tobytes() != w2:
                wrong.append((name, "neighbour", n2, int(status[j])))
    assert not wrong, wrong
    assert (out[spans[-1][0] + spans[-1][1]:] == 0xAA).all()


# ---- k_gz_sym_inflate ----------------------------------------------------------------------------------------------------------
def _gz(ctx, comp, starts, ends, cap, total, window=None):
    """Stretches [starts[k], ends[k]) of comp (ends[k] None: open-ended) -> (info, text, window_out)."""
    n = len(starts)
    tab = np.zeros(n, CHUNK)
    for k in range(n):
        tab[k]["in_off"] = starts[k]
        tab[k]["in_len"] = len(comp) - starts[k]
        tab[k]["end_bit"] = (ends[k] - starts[k]) * 8 if ends[k] is not None else NONE
    d_comp = torch.from_numpy(np.frombuffer(comp + bytes(128), np.uint8).copy()).cuda()
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    d_text = torch.full((total + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    d_wout = torch.zeros(32768, dtype=torch.uint8, device="cuda")
    d_win = torch.from_numpy(np.frombuffer(window, np.uint8).copy()).cuda() if window is not None else None
    info = ctx.gz_inflate_dev(d_comp, d_tab, n, (cap + 15) // 8 * 8, d_text, total + 64, d_win, d_wout)
    text = d_text[:int(info.n_bytes)].cpu().numpy().tobytes() if not info.status else b""
    return info, text, d_wout.cpu().numpy().tobytes()


def _flushed(piece, level):
    """zlib-written, ending on a byte behind a non-final block (a sync flush), referring to nothing in front of it."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(piece) + c.flush(zlib.Z_SYNC_FLUSH)


def test_gz_single_stretches_other_encoders_write(ctx):
    """Each accept stream as ONE open-ended stretch, the gzip trailer behind its final block."""
    wrong = []
    for c in cases.accept_cases():
        trailer = zlib.crc32(c.want).to_bytes(4, "little") + (len(c.want) & 0xffffffff).to_bytes(4, "little")
        info, text, wout = _gz(ctx, c.stream + trailer, [0], [None], len(c.want) + 8, len(c.want))
        if info.status != 0:
            wrong.append((c.name, "status", info.status))
        elif text != c.want or wout != (bytes(32768) + c.want)[-32768:]:
            wrong.append((c.name, "text" if text != c.want else "window_out"))
        elif info.final_chunk != 1 or (info.end_bit + 7) // 8 != len(c.stream):
            wrong.append((c.name, "end", info.final_chunk, info.end_bit, len(c.stream) * 8))
    assert not wrong, wrong


def test_gz_crafted_stretches_between_zlib_written_ones(ctx):
    """ONE stream, one launch: zlib-written stretch, crafted stretch, zlib-written stretch, crafted stretch ... cut where the
    sync-flush markers are.  Every crafted stretch is decoded with the history in front of it unknown."""
    fq = cases.fastq_text()
    comp, starts, pieces = b"", [], []
    for k, c in enumerate(cases.accept_cases()):
        piece = fq[700 * k:700 * k + 2000 + 333 * (k % 5)]
        for stream, text in ((_flushed(piece, 1 + k % 9), piece), (c.open_stream, c.want)):
            starts.append(len(comp))
            comp += stream
            pieces.append(text)
    last = zlib.compressobj(6, zlib.DEFLATED, -15)
    starts.append(len(comp))
    comp += last.compress(fq[:5000]) + last.flush()
    pieces.append(fq[:5000])
    whole = b"".join(pieces)
    assert zlib.decompress(comp, -15) == whole
    info, text, wout = _gz(ctx, comp, starts, starts[1:] + [None], max(len(p) for p in pieces) + 8, len(whole))
    assert info.status == 0, (info.status, info.bad_chunk, ([c.name for c in cases.accept_cases()] * 2)[info.bad_chunk // 2])
    assert info.final_chunk == len(pieces)
    if text != whole:
        at, names = 0, []
        for k, p in enumerate(pieces):
            if text[at:at + len(p)] != p:
                names.append(cases.accept_cases()[k // 2].name if k % 2 else "zlib-written %d" % k)
            at += len(p)
        assert False, names
    assert wout == whole[-32768:]


def test_gz_stretches_rfc1951_forbids(ctx):
    """Each reject stream as a single open-ended stretch, and -- its bad block not a final one -- as the middle stretch between two
    zlib-written ones: a nonzero status that names the stretch."""
    fq = cases.fastq_text()
    front, back = _flushed(fq[:3000], 6), zlib.compressobj(6, zlib.DEFLATED, -15)
    back = back.compress(fq[3000:9000]) + back.flush()
    wrong = []
    for r in cases.reject_cases():
        info, _, _ = _gz(ctx, r.stream, [0], [None], REJECT_ROOM, REJECT_ROOM)   # (no window handed in: the call starts the stream)
        if info.status == 0 or info.bad_chunk != 0:
            wrong.append((r.name, "alone", info.status, info.bad_chunk))
        if r.open_stream is None:
            continue
        comp = front + r.open_stream + back
        starts = [0, len(front), len(front) + len(r.open_stream)]
        info, _, _ = _gz(ctx, comp, starts, starts[1:] + [None], REJECT_ROOM, 3 * REJECT_ROOM)
        if info.status == 0 or info.bad_chunk != 1:
            wrong.append((r.name, "in the middle", info.status, info.bad_chunk))
    assert not wrong, wrong


@pytest.mark.parametrize("how", ["walk", "walk_of_many", "lds", "groups"])
def test_gz_match_in_front_of_the_stream(request, how):
    """dist == bytes written + 1 where the history is real: a crafted stretch behind zlib-written ones whose match reaches ONE
    byte in front of the stream's first (zlib: invalid distance too far back) is status 25 for that stretch -- it read zeros and
    the call reported success before.  The same match one byte shorter, to the stream's very first byte, is fine, and so is the
    longer one where the caller hands a window in (zlib: the same stream with that window as its dictionary).  Every form of the
    walk over the histories makes the check: k_gz_windows with 256 threads and -- more than six stretches per CU -- with 1024,
    k_gz_windows_lds, and k_gz_win_chain of the three-step form."""
    if how in ("lds", "groups"):
        from conftest import in_hooks_build
        if in_hooks_build(request, {"HPN_GZ_WINDOWS": how}):
            return
    ctx = request.getfixturevalue("ctx")
    fq = cases.fastq_text()
    fronts = [fq[:3000]] if how != "walk_of_many" else [fq[2 * k:2 * k + 2] for k in range(1700)]
    before = sum(len(f) for f in fronts)
    back = zlib.compressobj(6, zlib.DEFLATED, -15)
    back = back.compress(fq[3000:9000]) + back.flush()
    window = bytes(np.random.default_rng(25).integers(0, 256, 32768, dtype=np.uint8))
    for delta, win in ((1, None), (0, None), (1, window)):
        w = dc.BitWriter()
        text = list(b"in the middle")
        dc.fixed_block(w, text + [(5, before + len(text) + delta)] + text, False)
        dc.stored_block(w, b"")
        comp, starts = b"", []
        for stream in [_flushed(f, 6) for f in fronts] + [w.getvalue(), back]:
            starts.append(len(comp))
            comp += stream
        d = zlib.decompressobj(-15, zdict=win) if win is not None else zlib.decompressobj(-15)
        try:
            want = d.decompress(comp)
        except zlib.error as e:
            assert "too far back" in str(e) and delta == 1 and win is None
            want = None
        info, got, _ = _gz(ctx, comp, starts, starts[1:] + [None], 8192, before + 8192, window=win)
        if want is None:
            assert (info.status, info.bad_chunk) == (25, len(fronts)), (how, info.status, info.bad_chunk)
        else:
            assert info.status == 0 and got == want, (how, delta, info.status, info.bad_chunk)


# ---- k_gz_find_starts ----------------------------------------------------------------------------------------------------------
def test_block_starts_of_another_encoders_stream_are_found(ctx):
    """280 KB of FASTQ text re-encoded with joint code-length runs in blocks of 150 to 20000 symbols: a slice that holds
    a dynamic block's start -- the builder knows where every one is -- reports a position at or before it from which zlib
    decodes on (test_gz_inflate_gpu.py::test_block_starts_found_on_the_device's contract)."""
    text, toks = cases.fastq_text(), cases.fastq_tokens()
    comp, block_bits = dc.encode_stream(text, (20000, 150, 3000, 700, 9000), rle="joint", tokens=toks)
    assert zlib.decompress(comp, -15) == text and 200_000 <= len(text) and len(block_bits) >= 8
    d_comp = torch.from_numpy(np.frombuffer(comp + bytes(512), np.uint8).copy()).cuda()
    slices, want = [], []
    for s in block_bits[1:-1]:                              # (the first block starts the stream, the last one is final: not proposed)
        for back in (0, 1, 3, 5 * 8 + 1, 300 * 8 + 5):
            if s - back < 0:
                continue
            slices.append((s - back, back + 40 * 8))
            want.append(s)
    found = ctx.gz_find_starts_dev(d_comp, len(comp), slices)
    bits = np.unpackbits(np.frombuffer(comp, np.uint8), bitorder="little")
    wrong = []
    for (lo, n), w, f in zip(slices, want, found):
        f = int(f)
        if not lo <= f <= w:
            wrong.append((lo, w, f if f != NONE else "nothing"))
            continue
        if f != w:                                          # an earlier start inside the slice: it must be a true one
            d = zlib.decompressobj(-15)
            try:
                d.decompress(np.packbits(bits[f:], bitorder="little").tobytes())
            except zlib.error as e:                         # a match reaching in front of the start is the only excuse
                if "distance too far back" not in str(e):
                    wrong.append((lo, w, f, str(e)))
    assert not wrong, (len(wrong), len(slices), wrong[:8])


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bam,block", [("e.bam", 200), ("rand.bam", 30011)])
def test_bam2depth_on_a_bam_another_encoder_wrote(bam, block, tmp_path):
    """The BAM's records in BGZF blocks of another size whose DEFLATE streams come from the builder (joint runs, several dynamic
    blocks per BGZF block): bam2depth writes what it writes for the original, on the device routes and on the host's."""
    src = golden_path("bam", bam)
    crafted = tmp_path / "crafted_src"
    crafted.mkdir()
    cases.repack_bam_foreign(src, str(crafted / bam), block)
    outs = {}
    for tag, where in (("original", os.path.dirname(src)), ("crafted", str(crafted))):
        for route, env in (("device", {"HPN_TIMING": "1"}), ("device_chunks", {"HPN_TIMING": "1", "HPN_BAM_CHUNK": "65600"}),
                           ("host", {"HPN_BAM_GPU": "0"})):
            d = tmp_path / (tag + "_" + route)
            d.mkdir()
            shutil.copy(os.path.join(where, bam), d / bam), shutil.copy(os.path.join(where, bam + ".bai"), d / (bam + ".bai"))
            p = subprocess.run([os.path.join(BIN, "bam2depth"), "-w", "100", "-o", "d", bam], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               env={**os.environ, **env})
            assert p.returncode == 0, p.stderr.decode()
            if route != "host":
                assert b"[hpn] GPU ingest" in p.stderr and b"abandoned" not in p.stderr and b"host ingest" not in p.stderr, p.stderr.decode()
            outs[tag, route] = (p.stdout, open(d / "d.1.depth", "rb").read(), open(d / (bam + ".1.bedGraph"), "rb").read())
    assert len(outs["original", "device"][1]) > 0
    for key, got in outs.items():
        assert got == outs["original", "device"], key


@pytest.mark.parametrize("members", [1, 3])
def test_fastq_count_on_a_gzip_another_encoder_wrote(members, tmp_path):
    """A golden .fq.gz's text as one crafted member and as three: fastq_count's report is the one for the golden file, on the
    device routes (block starts found by the host and by the device) and on the host routes."""
    import gzip
    name = "syn_var_b.fq.gz"
    text = gzip.open(golden_path("fastq", name), "rb").read()
    shutil.copy(golden_path("fastq", name), tmp_path / "golden.fq.gz")
    cut = [len(text) * k // members + (17 if 0 < k < members else 0) for k in range(members + 1)]
    blob = b""
    for k in range(members):
        piece = text[cut[k]:cut[k + 1]]
        stream, _ = dc.encode_stream(piece, (5000, 300, 12000), rle="joint", chain=3)
        blob += dc.gzip_member(stream, piece)
    (tmp_path / "crafted.fq.gz").write_bytes(blob)
    assert gzip.decompress(blob) == text

    def report(path, env):
        p = subprocess.run([os.path.join(BIN, "fastq_count"), "-H", "-L", path], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env={**os.environ, "HPN_TIMING": "1", **env})
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout.replace(path.encode(), b"FILE"), p.stderr
    want, _ = report("golden.fq.gz", {"HPN_NO_MGZ": "1", "HPN_NO_BGZF": "1"})
    assert len(want) > 100
    for env in ({"HPN_GZ_GPU_FORCE": "1"}, {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_FIND": "device"},
                {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "5", "HPN_GZ_FIND": "host"},
                {"HPN_GZ_GPU": "0"}, {"HPN_PGZ_FORCE": "1", "HPN_PGZ_CHUNK": "3000", "HPN_GZ_THREADS": "3"}, {"HPN_NO_MGZ": "1", "HPN_TEXT": "0"}):
        got, err = report("crafted.fq.gz", env)
        assert got == want, env
        if "HPN_GZ_GPU_FORCE" in env:
            assert b"[hpn] gzip on the GPU" in err, (env, err.decode())
