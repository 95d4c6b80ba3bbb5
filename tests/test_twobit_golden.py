"""CPU: the Python restatement of fastq2twobit and twoBit2seq (twobit_ref.py: framing, the reverse order, the header, the codes,
the zero padding; the header, floor(body / packedLen) records from a zeroed buffer) equals every output and stderr line recorded
from the compiled reference (tests/golden/twobit/), and has no answer where the reference has none."""
import atexit
import gzip
import hashlib
import json
import os
import shutil
import tempfile
import zlib

import pytest

import twobit_inputs
import twobit_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "twobit", "manifest.json")))
CASES = MANIFEST["cases"]
BY_ID = {c["id"]: c for c in CASES}
OWN = "twobit/inputs/"
_made = []


def input_path(rel):
    """A case's input file: a file of tests/golden/fastq/, or one of tests/twobit_inputs.py -- those are made once per process in
    a temporary directory and held to the digests the recorder stored."""
    if not rel.startswith(OWN):
        return os.path.join(GOLDEN, rel)
    if not _made:
        _made.append(tempfile.mkdtemp(prefix="twobit_inputs_"))
        atexit.register(shutil.rmtree, _made[0], ignore_errors=True)
        twobit_inputs.materialize(_made[0], MANIFEST["inputs"])
    return os.path.join(_made[0], rel[len(OWN):])


def read_input(rel):
    raw = open(input_path(rel), "rb").read()
    return gzip.decompress(raw) if rel.endswith(".gz") else raw


def case_input(case):
    """The bytes a case's tool reads (a pack case: the inflated text): b"" for a missing file, the restatement's packing of
    another case's input for a round trip -- held to the digest of what the reference read."""
    if case["from"]:
        data = twobit_ref.pack(read_input(BY_ID[case["from"]]["in"]))[0]
        assert hashlib.sha256(data).hexdigest() == case["in_sha256"], case["id"]
        return data
    return read_input(case["in"]) if case["in"] else b""


def by_name(case):
    name = False
    for a in case["args"]:
        name = True if a == "-n" else False if a == "-s" else name
    return name


def output_name(case):
    """The file a case's tool writes, or None for standard output."""
    o = [case["args"][i + 1] for i, a in enumerate(case["args"]) if a == "-o"]
    prefix = o[-1] if o else ("-" if case["tool"] == "pack" else "out")
    if prefix.startswith("-"):
        return None
    return prefix + (".decompress" if case["tool"] == "unpack" else "_sort_by_name.fq" if by_name(case) else "_sort_by_seq.fq")


def expected(case):
    """(stdout, files, stderr) of a case the reference answers, from the restatement."""
    data = case_input(case)
    out, err = twobit_ref.pack(data, by_name(case))[:2] if case["tool"] == "pack" else twobit_ref.unpack(data)
    name = output_name(case)
    return (out, {}, err) if name is None else (b"", {name: out}, err)


def check_blob(o, text, what):
    assert len(text) == o["size"], what
    assert hashlib.sha256(text).hexdigest() == o["sha256"], what
    if o["text"] is not None:
        assert text == o["text"].encode("latin-1"), what


def check_outputs(case, stdout, files):
    """stdout: bytes; files: {file name: bytes}.  Everything the reference wrote equals them."""
    assert sorted(files) == sorted(o["name"] for o in case["outputs"]), case["id"]
    check_blob(case["stdout"], stdout, "stdout")
    for o in case["outputs"]:
        check_blob(o, files[o["name"]], o["name"])


SAME = [c for c in CASES if c["expect"] == "same"]
REFUSE = [c for c in CASES if c["expect"] == "refuse"]


@pytest.mark.parametrize("case", SAME, ids=[c["id"] for c in SAME])
def test_restatement_equals_the_reference(case):
    stdout, files, err = expected(case)
    check_outputs(case, stdout, files)
    assert err == case["stderr"]


@pytest.mark.parametrize("case", REFUSE, ids=[c["id"] for c in REFUSE])
def test_restatement_has_no_answer_where_the_reference_has_none(case):
    with pytest.raises((twobit_ref.NoAnswer, zlib.error, gzip.BadGzipFile, EOFError)):
        expected(case)


def test_the_goldens_cover_what_they_claim():
    same = lambda tool: [c for c in SAME if c["tool"] == tool]
    assert len(same("pack")) >= 30 and len(same("unpack")) >= 30      # nothing hides behind `refuse`
    assert all(c["rc"] == 0 for c in SAME)
    # refuse: a crash, a constructed high byte, or a header with packedLen == 0 in a file of two or more bytes -- nothing else
    for c in REFUSE:
        if c["endless"]:
            data = case_input_unchecked(c)
            assert c["tool"] == "unpack" and len(data) >= 2 and data[1] == 0, c["id"]
        else:
            assert c["constructed"] or c["rc"] in (-11, -6), c["id"]
    assert {c["id"] for c in REFUSE} >= {"p_trunc_fq", "p_longname_fq", "p_badcrc_fq_gz", "p_hi_last", "p_hi_first", "p_hi_mid", "u_zero_zero", "u_p0_data",
                                          "u_seqlen0", "rt_len1022"}
    assert all(BY_ID[u]["expect"] == "usage" and BY_ID[u]["rc"] == 1 for u in ("p_opt_r", "p_no_arguments", "p_help", "u_opt_z", "u_no_arguments", "u_help"))
    # the worked examples
    assert BY_ID["p_example"]["outputs"][0]["text"].encode("latin-1") == bytes.fromhex("09039c9c000f50809c80")
    assert BY_ID["u_issue_a"]["outputs"][0]["text"] == "TCAGT\nTCAGT\nGACTT\nTTTTT\n" and BY_ID["u_issue_b"]["outputs"][0]["text"] == "TCA\n"
    # the header is modulo 256, an empty last record gives 00 00, no record gives no byte
    head = lambda cid: BY_ID[cid]["outputs"][0]["text"].encode("latin-1")[:2]
    assert (head("p_len256"), head("p_len257"), head("p_len1022"), head("p_len255")) == (b"\x00\x40", b"\x01\x41", b"\xfe\x00", b"\xff\x40")
    assert head("p_mixed") == b"\x00\x00" and BY_ID["p_len0"]["outputs"][0]["size"] == 2
    assert BY_ID["p_missing_file"]["outputs"][0]["size"] == BY_ID["p_empty_fq"]["outputs"][0]["size"] == 0
    # -s / -n only name the output; a leading '-' (and no -o, for the packer) is standard output
    assert BY_ID["p_opt_n"]["outputs"][0]["name"] == BY_ID["p_opt_s_n"]["outputs"][0]["name"] == "o_sort_by_name.fq"
    assert BY_ID["p_opt_n"]["outputs"][0]["sha256"] == BY_ID["p_plain12"]["outputs"][0]["sha256"]
    assert BY_ID["p_no_o"]["outputs"] == BY_ID["p_o_dash"]["outputs"] == BY_ID["u_o_dash"]["outputs"] == [] and BY_ID["p_no_o"]["stdout"]["size"] == 10
    assert BY_ID["u_no_o"]["outputs"][0]["name"] == "out.decompress"
    # a partial record is dropped; files of 0, 1 and 2 bytes give nothing
    assert BY_ID["u_partial"]["outputs"][0]["size"] == 5 * 151 and BY_ID["u_partial_only"]["outputs"][0]["size"] == 0
    assert [BY_ID["u_bytes%d" % k]["outputs"][0]["size"] for k in (0, 1, 2)] == [0, 0, 0]


def case_input_unchecked(case):
    if case["from"]:
        return twobit_ref.pack(read_input(BY_ID[case["from"]]["in"]))[0]
    return read_input(case["in"])


def test_restatement_units():
    ex = twobit_inputs.own_inputs()["example.fq"]
    out, err, n = twobit_ref.pack(ex)
    assert (out.hex(), n) == ("09039c9c000f50809c80", 3) and err.startswith("name: 0\tseq: 1\ndone read file at T s\nlist count: 3\n")
    assert twobit_ref.pack(b"")[0] == b"" and twobit_ref.pack(b"@a\n\n+\n\n")[0] == b"\x00\x00"
    assert twobit_ref.pack_seq(b"CcAaGgTtUuNn\r.") == bytes([0b01011010, 0b11110000, 0, 0])
    with pytest.raises(twobit_ref.NoAnswer):
        twobit_ref.pack(b"@a\nAC\x80T\n+\nIIII\n")
    with pytest.raises(twobit_ref.NoAnswer):
        twobit_ref.pack(b"@a\nACGT\n+\nIIII\n@b\nAC\n")
    assert twobit_ref.first_high([b"AC", b"A\xff", b"\x80"]) == 1
    assert twobit_ref.unpack(b"\x05\x01\x1b\x1b\xe4\x00")[0] == b"TCAGT\nTCAGT\nGACTT\nTTTTT\n"
    assert twobit_ref.unpack(b"\x03\x02\x1b\x1b\xe4")[0] == b"TCA\n"
    assert twobit_ref.unpack(b"\x00\x01abc")[0] == b"\n\n\n" and twobit_ref.unpack(b"\x05")[0] == b"" and twobit_ref.unpack(b"\x05\x02")[0] == b""
    with pytest.raises(twobit_ref.NoAnswer):
        twobit_ref.unpack(b"\x00\x00")
    # a round trip gives the sequences back, last first, every other letter as T
    assert twobit_ref.unpack(twobit_ref.pack(b"@a\nACGTN\n+\nIIIII\n@b\nggcca\n+\nIIIII\n")[0])[0] == b"GGCCA\nACGTT\n"
