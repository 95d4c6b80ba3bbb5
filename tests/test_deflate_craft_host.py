"""CPU: DEFLATE streams zlib's deflate never writes (tests/deflate_craft.py, tests/deflate_cases.py) -- the builder against
zlib's inflate, the two table bounds the device decoders' LDS tables are sized by, and the host decoders (fast_inflate.hpp in
its 8-bit form behind mgz_reader.hpp and in its 16-bit placeholder form behind pgz_reader.hpp) against zlib, byte for byte.

zlib's INFLATE is the oracle throughout: it accepts all of RFC 1951, its deflate uses a corner of it (code lengths of the
two alphabets run-length coded apart, no code with fewer than two symbols, 15-bit codes for the rarest symbols only)."""
import gzip
import os
import subprocess
import zlib

import numpy as np

import deflate_cases as cases
import deflate_craft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "highperformancengs_amd", "bin", "hpn_ingest_dump")


# ---- a. the builder is right -------------------------------------------------------------------------------------------------
def test_every_accept_stream_is_zlibs_too():
    wrong = []
    for c in cases.accept_cases():
        for form, stream in (("final", c.stream), ("open", c.open_stream)):
            d = zlib.decompressobj(-15)
            try:
                out = d.decompress(stream)
            except zlib.error as e:
                wrong.append((c.name, form, str(e)))
                continue
            if out != c.want or d.eof != (form == "final") or d.unused_data:
                wrong.append((c.name, form, len(out), len(c.want), d.eof))
    assert not wrong, wrong


def test_every_reject_stream_is_refused_by_zlib():
    taken = []
    for r in cases.reject_cases():
        try:
            zlib.decompress(r.stream, -15)
            taken.append(r.name)
        except zlib.error:
            pass
    assert not taken, taken
    assert len(cases.reject_cases()) == 22


def test_the_accept_list_covers_what_it_names():
    """What the cases are FOR, read back from the streams' own headers: a run symbol that crosses from the literal/length
    lengths into the distance lengths at every start the list names, HLIT / HDIST / HCLEN at their ends, 15-bit codes for
    284 and distance 29, a stored block of 65535 bytes at every bit phase."""
    names = {c.name for c in cases.accept_cases()}
    for sym, rep in ((16, 6), (16, 3), (17, 10), (17, 3), (18, 25), (18, 11)):
        for k in {0, 1, 2, rep - 1, rep}:
            assert "run%d_rep%d_starts%d_before" % (sym, rep, k) in names
    by = {c.name: c for c in cases.accept_cases()}

    def header(stream, at=0):
        v = int.from_bytes(stream[at:at + 4], "little")
        return (v >> 1) & 3, ((v >> 3) & 31) + 257, ((v >> 8) & 31) + 1, ((v >> 13) & 15) + 4
    assert header(by["hlit257_hdist1_hclen5"].stream) == (2, 257, 1, 5)
    assert header(by["hclen_field4"].stream) == (2, 257, 1, 8)
    assert header(by["table_room_852_and_400"].stream, 5 + 32768) == (2, 286, 30, 19)
    lit, dst = cases._wide_codes()
    assert lit[284] == 15 and dst[29] == 15 and lit[65] == 1 and sorted(lit)[-4:] == [15] * 4
    assert dc.kraft(lit) == 32768 and dc.kraft(dst) == 32768
    assert len(by["stored_len65535_phase0"].want) == 65535 + 6
    assert {len(by["stored_len65535_phase%d" % p].want) - 65535 for p in range(8)} == set(range(8))


def test_hclen_4_admits_no_valid_block():
    """With the lengths of 16, 17, 18 and 0 alone every code length is 0: no end-of-block code.  (Why the shortest HCLEN among
    the accept cases is 5.)"""
    w = dc.BitWriter()
    cl = [0] * 19
    cl[18] = cl[0] = 1
    dc.dynamic_block(w, [0] * 257, [0], [], True, rle="joint", cl_lens=cl, eob=False)
    assert (int.from_bytes(w.getvalue()[:4], "little") >> 13) & 15 == 0
    try:
        zlib.decompress(w.getvalue() + bytes(8), -15)
        assert False, "taken"
    except zlib.error as e:
        assert "end-of-block" in str(e)


# ---- b. the two table bounds -------------------------------------------------------------------------------------------------
def test_table_need_reproduces_the_literal_bound():
    lens = dc.lengths_from_counts(dc.LIT_852)
    assert len(lens) == 286 and dc.kraft(lens) == 32768
    assert dc.table_need(lens, 9) == 852
    assert dc.table_need(lens[::-1], 9) == 852          # (which symbol has which length does not matter)


def test_table_need_reproduces_the_distance_bound():
    lens = dc.lengths_from_counts(dc.DIST_400)
    assert len(lens) == 30 and dc.kraft(lens) == 32768
    assert dc.table_need(lens, 8) == 400


def test_no_complete_code_of_30_symbols_needs_more_than_400():
    assert dc.worst_table_need(30, 8) == 400
    # the enumeration itself, on sizes small enough to walk every code without the shortcut
    for n, root, longest in ((8, 2, 6), (10, 3, 7)):
        brute = max(dc.table_need([l for l, c in enumerate(v, 1) for _ in range(c)], root)
                    for v, left, rem in dc._count_vectors(1, longest, 1, n, longest, []))
        assert dc.worst_table_need(n, root, longest) == brute


# ---- c. the host decoders ----------------------------------------------------------------------------------------------------
def _cat(path, **env):
    r = subprocess.run([DUMP, "cat", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env={**os.environ, "HPN_READER_STATS": "1", **env})
    assert r.returncode == 0, r.stderr
    stats = dict(kv.split("=") for kv in r.stderr.decode().split() if "=" in kv)
    return r.stdout, stats, b"damaged" in r.stderr


def _zlib_members(raw):
    """What zlib makes of a file of gzip members (None: it refuses one)."""
    out, at = b"", 0
    try:
        while at < len(raw):
            d = zlib.decompressobj(31)
            out += d.decompress(raw[at:])
            if not d.eof:
                return None
            at = len(raw) - len(d.unused_data)
    except zlib.error:
        return None
    return out


CONFIGS = [{"HPN_GZ_THREADS": "1"}, {"HPN_GZ_THREADS": "4"}, {"HPN_FAST_INFLATE": "0", "HPN_GZ_THREADS": "3"},
           {"HPN_PGZ_FORCE": "1", "HPN_PGZ_CHUNK": "3000", "HPN_GZ_THREADS": "3"}]

# Crafted members the quick decoder is KNOWN to hand back to zlib, with the reason: none.
KNOWN_HAND_BACKS = {}


def _reencoded_fastq():
    fq = cases.fastq_text()
    stream, starts = dc.encode_stream(fq, (3000, 700, 20000, 150), rle="joint", tokens=cases.fastq_tokens())
    assert dc.zlib_inflate(stream) == fq
    return dc.gzip_member(stream, fq)


def test_crafted_members_through_the_host_readers(tmp_path):
    """Every accept stream as a gzip member of its own: the member reader's quick decoder takes it (no hand-back to zlib), the
    two-pass reader (16-bit placeholders, chunks of 3000 compressed bytes) delivers the same bytes."""
    handed_back, wrong = [], []
    for c in cases.accept_cases():
        p = tmp_path / (c.name + ".gz")
        p.write_bytes(dc.gzip_member(c.stream, c.want, name=c.name.encode() if len(c.name) % 2 else None))
        out, st, damaged = _cat(str(p), HPN_NO_PGZ="1", HPN_GZ_THREADS="2")
        assert st["reader"] == "mgz"
        if out != c.want or damaged:
            wrong.append((c.name, "member reader", len(out), damaged))
        if st["handed_back"] != "0" and c.name not in KNOWN_HAND_BACKS:
            handed_back.append(c.name)
        out, st, damaged = _cat(str(p), **CONFIGS[3])
        assert st["reader"] == "pgz"
        if out != c.want or damaged or st["crc_failed"] != "0":
            wrong.append((c.name, "two-pass reader", len(out), damaged, st))
        for env in CONFIGS[:3]:                             # (whichever reader the tools would pick for the file)
            out, st, damaged = _cat(str(p), **env)
            if out != c.want or damaged:
                wrong.append((c.name, env, st["reader"], len(out), damaged))
    assert not wrong, wrong
    assert not handed_back, ("the quick decoder handed streams back that zlib accepts", handed_back)


def test_reencoded_fastq_through_the_two_pass_reader(tmp_path):
    """FASTQ text as another encoder writes it -- joint code-length runs, blocks of 150 to 20000 symbols -- is found, cut into
    chunks and decoded with the history unknown like zlib's own output: no fallback, and the chunks are used."""
    fq = cases.fastq_text()
    p = tmp_path / "foreign.fq.gz"
    p.write_bytes(_reencoded_fastq())
    for chunk, threads in (("3000", "3"), ("20000", "1"), ("20000", "4")):
        out, st, damaged = _cat(str(p), HPN_PGZ_FORCE="1", HPN_PGZ_CHUNK=chunk, HPN_GZ_THREADS=threads)
        assert out == fq and not damaged
        assert st["reader"] == "pgz" and st["fallback"] == "0" and st["crc_failed"] == "0" and int(st["accepted"]) > 2, st
    for env in CONFIGS[:3]:
        out, st, damaged = _cat(str(p), HPN_NO_PGZ="1", **env)
        assert out == fq and not damaged and st["handed_back"] == "0", (env, st)


def test_files_mixing_crafted_and_zlib_written_members(tmp_path):
    rng = np.random.default_rng(12)
    fq = cases.fastq_text()
    members, want = [], b""
    for k, c in enumerate(cases.accept_cases()):
        members.append(dc.gzip_member(c.stream, c.want))
        want += c.want
        if k % 3 == 0:
            a = int(rng.integers(0, len(fq) - 50000))
            piece = fq[a:a + int(rng.integers(0, 50000))]
            members.append(gzip.compress(piece, int(rng.integers(1, 10))))
            want += piece
    members.insert(7, _reencoded_fastq())
    want = _zlib_members(b"".join(members))
    assert want is not None
    p = tmp_path / "mixed.gz"
    p.write_bytes(b"".join(members))
    for env in CONFIGS:
        out, st, damaged = _cat(str(p), **env)
        assert out == want and not damaged, (env, len(out), len(want), st)
        if "HPN_FAST_INFLATE" not in env and st["reader"] == "mgz":
            assert st["handed_back"] == "0", (env, st)


def test_rejected_members_with_the_quick_decoder_on_and_off(tmp_path):
    """A member zlib refuses, alone and between two sound members: the delivered bytes do not depend on the quick decoder."""
    fq = cases.fastq_text()
    a, b = gzip.compress(fq[:70000], 6), gzip.compress(fq[70000:90000], 1)
    differ = []
    for r in cases.reject_cases():
        bad = dc.gzip_member(r.stream, b"")
        for form, blob in (("alone", bad), ("between", a + bad + b)):
            p = tmp_path / ("%s_%s.gz" % (r.name, form))
            p.write_bytes(blob)
            outs = [_cat(str(p), **env) for env in ({"HPN_GZ_THREADS": "4"}, {"HPN_FAST_INFLATE": "0", "HPN_GZ_THREADS": "4"},
                                                    {"HPN_NO_PGZ": "1", "HPN_GZ_THREADS": "1"})]
            if not (outs[0][0] == outs[1][0] == outs[2][0]) or len({o[2] for o in outs}) != 1:
                differ.append((r.name, form, [len(o[0]) for o in outs], [o[2] for o in outs]))
            if form == "between" and not outs[0][0].startswith(fq[:70000]):
                differ.append((r.name, form, "the sound member in front is not delivered"))
    assert not differ, differ


def test_bam_another_encoder_wrote_through_the_host_reader(tmp_path):
    """The golden BAMs' records in BGZF blocks of another size, every block's DEFLATE stream from the builder: the host's BAM
    reader decodes the records it decodes from the original."""
    for bam, block in (("e.bam", 200), ("rand.bam", 30011)):
        src = os.path.join(ROOT, "tests", "golden", "bam", bam)
        dst = str(tmp_path / bam)
        n = cases.repack_bam_foreign(src, dst, block)
        assert n > 0 and gzip.open(dst, "rb").read() == gzip.open(src, "rb").read()
        a = subprocess.run([DUMP, "bam", src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
        b = subprocess.run([DUMP, "bam", dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
        assert a == b and len(a) > 8, bam
