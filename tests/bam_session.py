"""What the GPU tests of the record-store sessions (hpn_bam_sort_*, _rmdup_*, _merge_*, _fixmate_*) do alike through the ABI: the
inflated stream cut into batches by the test itself -- BGZF blocks made that end exactly where a batch is to end, one
hpn_bgzf_inflate_dev + hpn_bam_raw_index_dev + _add_raw_dev round per batch, the unfinished record (hpn_raw_info.tail_bytes)
carried in front of the next --, the output fetched slice by slice with every answer of a slice checked against the others, and
the blocks bamsort_ref cuts of the same records.  A family is named as the API's methods name it: "sort", "rmdup", "merge",
"fixmate"."""
import zlib

import numpy as np

import bam_layouts as BL
import bamsort_ref

FULL = bamsort_ref.FULL
FAMILIES = ("sort", "rmdup", "merge", "fixmate")
TID_ZERO = ("sort", "rmdup", "merge")      # the families whose blocks' tid the tests hold to 0


def feed(ctx, add, stream, cuts):
    """the records of `stream` through add -- the family's ctx.bam_*_add_raw_dev -- in batches that end at the stream offsets `cuts`;
    the last info, or the first that names a record outside the domain"""
    import torch
    cuts = sorted({c for c in cuts if 0 < c < len(stream)} | {len(stream)}) if stream else []
    front, at, info = b"", 0, None
    for end in cuts:
        piece = stream[at:end]
        at = end
        members = [BL.bgzf_member(piece[i:i + 60000], 1) for i in range(0, len(piece), 60000)]
        table, comp, outo = np.zeros((len(members), 3), np.uint64), [], len(front)
        pos = 0
        for k, mem in enumerate(members):
            a, n, isz = BL.blocks(mem)[0]
            table[k] = (pos + a, n | (isz << 32), outo)
            comp.append(mem)
            pos += len(mem)
            outo += isz
        nb = len(members)
        d_comp = torch.from_numpy(np.frombuffer(b"".join(comp) + bytes(64), np.uint8).copy()).cuda()
        d_blocks = torch.from_numpy(table.view(np.int64)).cuda()
        d_out = torch.zeros(outo + 64, dtype=torch.uint8, device="cuda")
        if front:
            d_out[:len(front)] = torch.from_numpy(np.frombuffer(front, np.uint8).copy()).cuda()
        d_status = torch.zeros(nb, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.bgzf_inflate_dev(d_comp, d_blocks, nb, d_out, d_status)
        raw = ctx.bam_raw_index_dev(d_out, d_blocks, nb, 0, d_status)
        assert raw.flags & 3 == 0, raw.flags
        whole = front + piece
        front = whole[len(whole) - raw.tail_bytes:] if raw.tail_bytes else b""
        if raw.n_records:
            info = add(d_out)
            if info.bad_record >= 0:
                return info
    assert front == b""
    return info


def emit_all(ctx, family, n, slice_records, stored=False):
    """the family's n output records in slices -> ([(payload, crc)] of every block, the stored image if asked for)"""
    emit, blocks_of, payload = (getattr(ctx, "bam_%s_%s" % (family, what)) for what in ("emit", "blocks", "payload"))
    blocks, image, first = [], b"", 0
    while True:
        cnt = min(slice_records, n - first)
        last = first + cnt == n
        info = emit(first, cnt, last)
        assert info.n_records == cnt and info.bad_record == -1
        bl = blocks_of(info.n_blocks)
        assert len(bl) == info.n_blocks
        pay = payload()
        assert len(pay) == info.payload_bytes
        for b in bl:
            assert family not in TID_ZERO or b.tid == 0
            assert 0 < b.len <= FULL and b.off + b.len <= len(pay)
            blocks.append((pay[b.off:b.off + b.len], b.crc))
        if stored:
            img = getattr(ctx, "bam_%s_stored" % family)()
            assert len(img) == sum(b.len + 31 for b in bl)
            image += img
        assert (info.open_bytes == 0) if last else (info.open_bytes < FULL)
        first += cnt
        if last:
            return blocks, image


def blocks_of_records(out):
    """the records of the output, as bytes, in its order -> [(payload, crc)] of the blocks bam_write1 cuts"""
    return [(p, zlib.crc32(p) & 0xffffffff) for p in bamsort_ref.cut(b"", out)]


def expected_blocks(recs, order):
    return blocks_of_records([recs[i] for i in order])


def every_boundary_and_inside(recs):
    cuts, at = set(), 0
    for r in recs:
        cuts |= {at + 1, at + 9, at + len(r) // 2, at + len(r) - 1, at + len(r)}
        at += len(r)
    return cuts
