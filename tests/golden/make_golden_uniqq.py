#!/usr/bin/env python3
"""Records what the reference gzfastq_uniqQ does: tests/golden/uniqq/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  The reference tool
is compiled into a TEMPORARY directory -- gzfastq_uniqQ.c with list.c, hiredis/sds.c and hiredis/dict.c -- run on the
cases below, and its output (the file, or standard output), stderr (the run times masked) and exit status or signal
are stored as data.  No reference text is stored.  Outputs of up to 2 KiB are kept in the manifest (bytes as the code
points 0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of tests/golden/fastq/ come from
tests/uniqq_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the tests make them again
and check it.  Re-running reproduces the file byte for byte.

What a case expects of the tool here ("expect"):
  same     the reference finished: bytes, stderr and status are the tool's.
  refuse   the reference crashed while reading: the tool leaves with status 2.
  usage    no argument, or -h: usage on stderr, status 1 (the usage text is the tool's own).
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import uniqq_inputs  # noqa: E402  (tests/uniqq_inputs.py)

OUT = os.path.join(HERE, "uniqq")
INLINE_LIMIT = 2 << 10
TIMES = re.compile(rb"at \d+\.\d{3} s")
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_uniq.py's list


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "gzfastq_uniqQ_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", ref, "-I", os.path.join(ref, "hiredis"), os.path.join(ref, "gzfastq_uniqQ.c"),
                           os.path.join(ref, "list.c"), os.path.join(ref, "hiredis", "sds.c"), os.path.join(ref, "hiredis", "dict.c"), "-o", exe, "-lz"])
    return exe


def cases():
    c = []

    def add(cid, in1, flags, out="o", stdin=False, dups=False, hash_size=None):
        """flags: the order flags as given; out: the -o argument (None: none); stdin: the input comes on standard input, no -1."""
        c.append({"id": cid, "in1": in1, "flags": flags, "out": out, "stdin": stdin, "dups": dups, "hash_size": hash_size})

    for f in FASTQ:
        for flag in ("S", "C"):
            add("%s_%s" % (f.replace(".", "_"), flag), "fastq/" + f, ["-" + flag])
    for u in uniqq_inputs.TIE_US:
        size = 4
        while size < u:
            size *= 2
        add("with_u%d_C" % u, "uniqq/inputs/with_u%d.fq" % u, ["-C"], dups=True, hash_size=size)
        add("ties_u%d_C" % u, "uniqq/inputs/ties_u%d.fq" % u, ["-C"], dups=True, hash_size=size)
    for u in (4, 5, 8, 9, 16, 17):
        add("equal_u%d_C" % u, "uniqq/inputs/equal_u%d.fq" % u, ["-C"], dups=True)
    for name in ("widths", "ragged_group", "short_quals", "crlf_dups", "nonl_dups", "lone_line", "hibytes", "dups5000", "refine"):
        for flag in ("S", "C"):
            add("%s_%s" % (name, flag), "uniqq/inputs/%s.fq" % name, ["-" + flag], dups=True)
    add("stdin_C", "uniqq/inputs/dups5000.fq", ["-C"], stdin=True, dups=True)
    add("stdin_gzip_S", "fastq/multi.fq.gz", ["-S"], stdin=True)
    add("stdout_no_o_S", "uniqq/inputs/widths.fq", ["-S"], out=None, dups=True)
    add("stdout_no_o_no_flag", "uniqq/inputs/widths.fq", [], out=None, dups=True)
    add("stdout_dash_x_C", "uniqq/inputs/widths.fq", ["-C"], out="-x", dups=True)
    add("flags_S_C", "uniqq/inputs/ties_u17.fq", ["-S", "-C"], dups=True)
    add("flags_C_S", "uniqq/inputs/ties_u17.fq", ["-C", "-S"], dups=True)
    add("no_arguments", None, [], out=None)
    add("help", None, ["-h"], out=None)
    return c


def blob(text):
    o = {"size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None}
    if text and len(text) <= INLINE_LIMIT:
        o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
    return o


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = uniqq_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len("uniqq/inputs/"):]) if rel.startswith("uniqq/inputs/") else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            cmd = [exe] + (["-1", where(c["in1"])] if c["in1"] and not c["stdin"] else []) + c["flags"] + (["-o", c["out"]] if c["out"] else [])
            stdin = open(where(c["in1"]), "rb") if c["stdin"] else subprocess.DEVNULL
            p = subprocess.run(cmd, cwd=work, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, "MALLOC_CHECK_": "0"})
            err = TIMES.sub(b"at T s", p.stderr)
            if c["in1"] is None:
                assert p.returncode == 1 and b"Usage" in p.stderr and not p.stdout and not os.listdir(work), c["id"]
                expect, err = "usage", b""
            elif p.returncode == 0:
                expect = "same"
            else:
                assert p.returncode in (-6, -11), (c["id"], p.returncode)
                expect, err = "refuse", b""
            entry = {"id": c["id"], "in1": c["in1"], "flags": c["flags"], "out": c["out"], "stdin": c["stdin"], "rc": p.returncode,
                     "expect": expect, "stderr": err.decode("latin-1"), "stdout": None, "outputs": []}
            if expect == "same":
                entry["stdout"] = blob(p.stdout)
                for fn in sorted(os.listdir(work)):
                    entry["outputs"].append(dict(blob(open(os.path.join(work, fn), "rb").read()), name=fn))
                to_stdout = c["out"] is None or c["out"].startswith("-")
                assert [o["name"] for o in entry["outputs"]] == ([] if to_stdout else ["o_sortKeyUniq.fq"]), c["id"]
                assert to_stdout or not p.stdout, c["id"]
            m = re.search(r"unique reads number = (\d+)\(\d+ / (\d+) = ", entry["stderr"])
            if c["dups"]:
                assert m and 0 < int(m.group(1)) < int(m.group(2)), (c["id"], entry["stderr"])
            if c["hash_size"] is not None:
                assert ("hash size: %d\n" % c["hash_size"]) in entry["stderr"], (c["id"], entry["stderr"])
            manifest.append(entry)
            print("%-24s rc %4d  %-8s %s" % (c["id"], p.returncode, expect, (m.group(0) if m else "")))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
