"""CPU: the Python restatement of gzfastq_uniqQ (uniqq_ref.py: framing, the per-key lists, both orders, the table's size)
equals every output and stderr line recorded from the compiled reference (tests/golden/uniqq/manifest.json); and
bin/gzfastq_uniqQ answers -h as the reference does, before it looks for a device."""
import atexit
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import tempfile
import zlib

import pytest

import uniq_ref
import uniqq_inputs
import uniqq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "uniqq", "manifest.json")))
CASES = MANIFEST["cases"]
RUNS = [c for c in CASES if c["expect"] != "usage"]
_made = []


def input_path(rel):
    """A case's input file: a file of tests/golden/fastq/, or one of tests/uniqq_inputs.py -- those are made once per
    process in a temporary directory and held to the digests the recorder stored."""
    if not rel.startswith("uniqq/inputs/"):
        return os.path.join(GOLDEN, rel)
    if not _made:
        _made.append(tempfile.mkdtemp(prefix="uniqq_inputs_"))
        atexit.register(shutil.rmtree, _made[0], ignore_errors=True)
        uniqq_inputs.materialize(_made[0], MANIFEST["inputs"])
    return os.path.join(_made[0], rel[len("uniqq/inputs/"):])


def read_input(rel):
    raw = open(input_path(rel), "rb").read()
    return gzip.decompress(raw) if rel.endswith(".gz") else raw


def by_count(case):
    """-S and -C each cancel the other: the last one given wins, -S is the default."""
    flags = [f for f in case["flags"] if f in ("-S", "-C")]
    return bool(flags) and flags[-1] == "-C"


def to_stdout(case):
    return case["out"] is None or case["out"].startswith("-")


def check_blob(o, text, what):
    assert len(text) == o["size"], what
    assert hashlib.sha256(text).hexdigest() == o["sha256"], what
    if o["text"] is not None:
        assert text == o["text"].encode("latin-1"), what


def check_recorded(case, out_text, stdout=None, files=None):
    """out_text: what the run wrote as its one output.  Held to the recorded file or the recorded standard output."""
    if to_stdout(case):
        assert case["outputs"] == []
        check_blob(case["stdout"], out_text, case["id"])
    else:
        assert [o["name"] for o in case["outputs"]] == ["o_sortKeyUniq.fq"] and case["stdout"]["size"] == 0
        check_blob(case["outputs"][0], out_text, case["id"])
    if files is not None:
        assert sorted(files) == [o["name"] for o in case["outputs"]]
        assert stdout == (out_text if to_stdout(case) else b"")


def expected(case):
    """(output bytes, masked stderr, table) from the restatement."""
    return uniqq_ref.simulate(read_input(case["in1"]), by_count(case))


@pytest.mark.parametrize("case", RUNS, ids=[c["id"] for c in RUNS])
def test_restatement_equals_the_reference(case):
    if case["expect"] == "refuse":
        with pytest.raises((uniq_ref.NoAnswer, zlib.error, gzip.BadGzipFile, EOFError)):
            expected(case)
        return
    out, err, r = expected(case)
    check_recorded(case, out)
    assert err == case["stderr"]


def test_the_goldens_cover_what_they_claim():
    by_id = {c["id"]: c for c in CASES}
    fastq = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
             "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]
    for f in fastq:
        for flag in "SC":
            assert by_id["%s_%s" % (f.replace(".", "_"), flag)]["flags"] == ["-" + flag]
    assert {c["id"][:-2] for c in CASES if c["expect"] == "refuse"} == {"trunc_fq", "longname_fq", "badcrc_fq_gz", "badcrc_mid_fq_gz", "badisize_fq_gz"}
    assert "= -nan%)" in by_id["empty_fq_S"]["stderr"] and "hash size: 0\n" in by_id["empty_fq_S"]["stderr"]
    # -C's ties cross every doubling of the table: at each U many keys share a count
    for u, size in ((3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (64, 64), (65, 128), (1025, 2048)):
        c = by_id["ties_u%d_C" % u]
        assert c["flags"] == ["-C"] and "unique reads number = %d(" % u in c["stderr"] and "hash size: %d\n" % size in c["stderr"]
        r = uniqq_ref.collapse(read_input(c["in1"]))
        counts = [len(r.members[k]) for k in r.table_order]
        assert sorted(set(counts)) == [2, 3] and min(counts.count(2), counts.count(3)) >= u // 2 and r.count_order != r.key_order
    for u in (4, 5, 8, 9, 16, 17):
        r = uniqq_ref.collapse(read_input(by_id["equal_u%d_C" % u]["in1"]))
        assert {len(m) for m in r.members.values()} == {2} and r.count_order == r.table_order != r.key_order
    r = uniqq_ref.collapse(read_input(by_id["widths_S"]["in1"]))
    assert sorted(len(m) for m in r.members.values()) == [1, 9, 10, 99, 100]
    r = uniqq_ref.collapse(read_input(by_id["ragged_group_S"]["in1"]))
    assert all(len({len(n) for n, q in m}) > 3 and len({len(q) for n, q in m}) > 3 for m in r.members.values())
    assert any(len(q) + 1 < len(k) for k, m in r.members.items() for n, q in m)       # short quality lines are regular
    assert any(len(q) + 1 < len(k) for k, m in uniqq_ref.collapse(read_input(by_id["short_quals_C"]["in1"])).members.items() for n, q in m)
    assert b"\r\n" in read_input(by_id["crlf_dups_S"]["in1"]) and not read_input(by_id["nonl_dups_S"]["in1"]).endswith(b"\n")
    assert not read_input(by_id["lone_line_C"]["in1"]).endswith(b"\n") and max(read_input(by_id["hibytes_C"]["in1"])) > 127
    assert by_id["stdin_C"]["stdin"] and by_id["stdin_gzip_S"]["stdin"]
    for cid in ("stdout_no_o_S", "stdout_no_o_no_flag", "stdout_dash_x_C"):
        assert by_id[cid]["outputs"] == [] and by_id[cid]["stdout"]["size"] > 0
    strip = lambda o: {k: v for k, v in o.items() if k != "name"}
    assert by_id["stdout_no_o_S"]["stdout"] == by_id["stdout_no_o_no_flag"]["stdout"] == strip(by_id["widths_S"]["outputs"][0])
    assert by_id["stdout_dash_x_C"]["stdout"] == strip(by_id["widths_C"]["outputs"][0])
    # the last flag wins
    assert strip(by_id["flags_S_C"]["outputs"][0]) == strip(by_id["ties_u17_C"]["outputs"][0]) != strip(by_id["flags_C_S"]["outputs"][0])
    assert by_id["no_arguments"]["rc"] == by_id["help"]["rc"] == 1


def test_restatement_units():
    out, err, r = uniqq_ref.simulate(b"@a 1\nACGT\n+\nIIII\n@b 1\nGG\n+\n55\n@c 1\nACGT\n+\nKKKK\n@d 1\nTT\n+\nAA\n@e 1\nACGT\n+\nMMMM\n")
    assert out.startswith(b"@e 1\t3\nACGT\n+\nMMMM\nKKKK\nIIII\n") and (r.n, r.u, r.hash_size, r.max_count) == (5, 3, 4, 3)
    assert uniqq_ref.simulate(b"@a\nACGT\n+\nII\n@b\nACGT\n+\nJ\n")[0] == b"@b\t2\nACGT\n+\nJ\nII\n"
    assert uniqq_ref.simulate(b"@a\nAC\n+\nII\n@tail")[0] == b"@a\t1\nAC\n+\nII\n"       # a lone line without '\n' is no record
    assert uniqq_ref.simulate(b"@a\nAC\n+\nII")[0] == b"@a\t1\nAC\n+\nI\n"              # the last line loses a real byte
    assert uniqq_ref.simulate(b"")[1].startswith("unique reads number = 0(0 / 0 = -nan%)\nhash size: 0\n")
    for bad in (b"@a\nAC\n+\nII\n@b\n", b"@a\nAC\n", b"@a\n" + b"A" * 1023 + b"\n+\nI\n", b"@a\nA\0C\n+\nIII\n"):
        with pytest.raises(uniq_ref.NoAnswer):
            uniqq_ref.simulate(bad)


def test_the_tool_prints_its_usage_without_a_device(tmp_path):
    exe = os.path.join(ROOT, "highperformancengs_amd", "bin", "gzfastq_uniqQ")
    for args in ([], ["-h"], ["-?"]):
        p = subprocess.run([exe] + args, cwd=tmp_path, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and b"Usage" in p.stderr and b"-C" in p.stderr and b"-S" in p.stderr and p.stdout == b"", args
    assert os.listdir(tmp_path) == []
