"""CPU: the Python restatement of gzfastq_mrle (mrle_ref.py: framing, the savings of pass 1, the flag byte, literals and run
tokens, the decoder, the packed file's length bytes modulo 256, and the two stdio streams on one descriptor) equals every output
and stderr line recorded from the compiled reference (tests/golden/mrle/), and has no answer where the reference has none."""
import atexit
import gzip
import json
import os
import shutil
import tempfile
import zlib

import pytest

import mrle_inputs
import mrle_ref
from test_twobit_golden import check_blob

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "mrle", "manifest.json")))
CASES = MANIFEST["cases"]
BY_ID = {c["id"]: c for c in CASES}
OWN = "mrle/inputs/"
_made = []


def input_path(rel):
    """A case's input file: a file of tests/golden/fastq/, or one of tests/mrle_inputs.py -- those are made once per process in a
    temporary directory and held to the digests the recorder stored."""
    if not rel.startswith(OWN):
        return os.path.join(GOLDEN, rel)
    if not _made:
        _made.append(tempfile.mkdtemp(prefix="mrle_inputs_"))
        atexit.register(shutil.rmtree, _made[0], ignore_errors=True)
        mrle_inputs.materialize(_made[0], MANIFEST["inputs"])
    return os.path.join(_made[0], rel[len(OWN):])


def read_input(rel):
    raw = open(input_path(rel), "rb").read()
    return gzip.decompress(raw) if rel.endswith(".gz") else raw


def by_name(case):
    name = False
    for a in case["args"]:
        name = True if a == "-n" else False if a == "-s" else name
    return name


def output_name(case):
    """The file a case's tool writes its packed stream to, or None: the packed stream shares standard output with the text."""
    o = [case["args"][i + 1] for i, a in enumerate(case["args"]) if a == "-o"]
    prefix = o[-1] if o else "-"
    return None if prefix.startswith("-") else prefix + ("_sort_by_name.fq" if by_name(case) else "_sort_by_seq.fq")


def expected(case):
    """(stdout, files, stderr) of a case the reference answers, from the restatement."""
    (packed, text, shared), err, _ = mrle_ref.mrle(read_input(case["in"]) if case["in"] else b"", by_name(case))
    name = output_name(case)
    return (shared, {}, err) if name is None else (text, {name: packed}, err)


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
    with pytest.raises((mrle_ref.NoAnswer, zlib.error, gzip.BadGzipFile, EOFError)):
        expected(case)


def enc(cid, k=0):
    """The k-th record's encoded bytes in a recorded packed file of records shorter than 256 encoded bytes."""
    data = BY_ID[cid]["outputs"][0]["text"].encode("latin-1")
    for _ in range(k):
        data = data[1 + data[0]:]
    return data[1:1 + data[0]]


def test_the_goldens_cover_what_they_claim():
    assert len(SAME) >= 40 and all(c["rc"] == 0 for c in SAME)      # nothing hides behind `refuse`
    assert sum(output_name(c) is None for c in SAME) >= 20      # the shared descriptor
    # refuse: a crash, a damaged stream, or a constructed out-of-domain byte -- nothing else
    for c in REFUSE:
        assert c["why"] in ("crash", "damaged stream", "out-of-domain byte"), c["id"]
        if c["why"] == "crash":
            assert c["rc"] in (-11, -6), c["id"]
        elif c["why"] == "damaged stream":
            with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
                read_input(c["in"])
        else:      # what the input itself shows
            quals = [r[2] for r in mrle_ref.records(read_input(c["in"]))]
            assert mrle_ref.first_bad(quals) is not None, c["id"]
    assert {c["id"]: c["why"] for c in REFUSE}.items() >= {"g_trunc_fq": "crash", "g_longname_fq": "crash", "g_badcrc_fq_gz": "damaged stream",
                                                           "g_crlf_fq": "out-of-domain byte", "g_t_fq": "out-of-domain byte", "f_bad_first": "out-of-domain byte",
                                                           "f_bad_mid": "out-of-domain byte", "s_bad_last": "out-of-domain byte"}.items()
    assert all(BY_ID[u]["expect"] == "usage" and BY_ID[u]["rc"] == 1 for u in ("opt_r", "no_arguments", "help"))
    # the worked examples, from the recorded packed file
    want = ["20 46 07", "00 46 46 23 23 46 46", "38 46 02 2f 37 37 3c 02 42 03", "20 46 fe", "20 46 ff 00", "20 46 ff ff 00", "01 23 ff ff 59"]
    assert [enc("f_examples", k) for k in range(7)] == [bytes.fromhex(w) for w in want]
    # the length byte wraps: F# x 300 encodes to 601 bytes behind the byte 0x59
    sizes = mrle_ref.mrle(read_input(OWN + "sizes.fq"))[0][0]
    assert sizes[:1] == b"\xff" and sizes[256:257] == b"\x00" and sizes[513:514] == b"\x01" and sizes[771:772] == b"\x59" and sizes[772:1373] == b"\x00" + b"F#" * 300
    check_blob(BY_ID["f_sizes"]["outputs"][0], sizes, "sizes")
    # an empty line is the flag byte alone; no record, no byte
    assert enc("f_one_empty") == b"\x00" and BY_ID["f_one_empty"]["stdout"]["text"] == "\n"
    assert BY_ID["missing_file"]["outputs"][0]["size"] == BY_ID["g_empty_fq"]["outputs"][0]["size"] == 0
    # -s / -n only name the output; a leading '-' (and no -o) puts the packed stream on standard output
    assert BY_ID["opt_n"]["outputs"][0]["name"] == BY_ID["opt_s_n"]["outputs"][0]["name"] == "o_sort_by_name.fq"
    assert BY_ID["opt_n"]["outputs"][0]["sha256"] == BY_ID["f_plain12"]["outputs"][0]["sha256"]
    assert BY_ID["no_o"]["outputs"] == BY_ID["o_dash_x"]["outputs"] == [] and BY_ID["no_o"]["stdout"] == BY_ID["s_reads150"]["stdout"]
    # one descriptor: under 4,096 bytes of text only the packed bytes arrive; a full buffer waits; one byte more flushes the block
    assert BY_ID["s_text4095"]["stdout"]["text"] == BY_ID["f_text4095"]["outputs"][0]["text"]
    assert BY_ID["s_text4096"]["stdout"]["size"] == BY_ID["f_text4096"]["outputs"][0]["size"]
    assert BY_ID["s_text4097"]["stdout"]["size"] == 4096 + BY_ID["f_text4097"]["outputs"][0]["size"]
    assert BY_ID["s_text8192"]["stdout"]["size"] == 4096 + BY_ID["f_text8192"]["outputs"][0]["size"]
    assert BY_ID["s_packed4096"]["stdout"]["size"] == 4096 and BY_ID["f_packed4096"]["outputs"][0]["size"] == 4096


def test_restatement_units():
    for line, want in ((b"FFFFFFFF", "20 46 07"), (b"FF##FF", "00 46 46 23 23 46 46"), (b"FFF/77<<<BBBB", "38 46 02 2f 37 37 3c 02 42 03"), (b"F" * 255, "20 46 fe"),
                       (b"F" * 256, "20 46 ff 00"), (b"F" * 511, "20 46 ff ff 00"), (b"#" * 600, "01 23 ff ff 59"), (b"", "00")):
        e = mrle_ref.encode(line)
        assert e == bytes.fromhex(want) and mrle_ref.decode(e, len(line)) == line
    assert mrle_ref.savings(b"F" * 256 + b"#" + b"F") == [-1, 0, 0, 0, 0, 256 - 2 - 1 - 1]
    e = mrle_ref.encode(b"F#" * 300)
    assert len(e) == 601 and mrle_ref.streams([b"F#" * 300])[0][:1] == b"\x59"
    assert len(mrle_ref.encode(b"F#" * 511)) == 1023      # at most len + 1
    with pytest.raises(mrle_ref.NoAnswer):
        mrle_ref.encode(b"IIII")
    with pytest.raises(mrle_ref.NoAnswer):
        mrle_ref.mrle(b"@a\nACGT\n+\nFFFF\n@b\nAC\n")
    assert mrle_ref.first_bad([b"FF", b"F#I", b"!"]) == 1
    # two streams on one descriptor: a block leaves when a call does not fit; a buffer that is exactly full waits
    t, p = lambda n: (0, b"t" * n), lambda n: (1, b"p" * n)
    assert mrle_ref.shared([t(4095), p(3)]) == b"ppp"
    assert mrle_ref.shared([t(4096), p(3)]) == b"ppp"
    assert mrle_ref.shared([t(4096), p(3), t(1)]) == b"t" * 4096 + b"ppp"
    assert mrle_ref.shared([t(4000), p(4096), t(97), p(1)]) == b"t" * 4096 + b"p" * 4096 + b"p"
    assert mrle_ref.shared([p(4096)]) == b"p" * 4096 and mrle_ref.shared([t(0), p(0)]) == b""
