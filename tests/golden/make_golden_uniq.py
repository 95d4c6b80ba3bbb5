#!/usr/bin/env python3
"""Records what the reference gzfastq_uniq does: tests/golden/uniq/.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  The reference tool
is compiled into a TEMPORARY directory -- gzfastq_uniq.c with hiredis/sds.c and hiredis/dict.c -- run on the inputs
below, and its outputs, stderr (the run times masked) and exit status or signal are stored as data.  No reference text
is stored.  Outputs of up to 2 KiB are kept in the manifest (bytes as the code points 0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of tests/golden/fastq/
come from tests/uniq_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the tests make
them again and check it.  Re-running reproduces the directory byte for byte.

What a case expects of the tool here ("expect"):
  same     the reference finished: bytes, stderr and status are the tool's.
  refuse   the reference has no answer (it crashed while READING, it was given no -o, or it reads outside its buffers:
           "ub" below): the tool leaves with status 2.
  diverge  the reference finished reading and crashed while WRITING: its dead split() of the name into a two-pointer
           array overruns on names of more than two fields.  The tool writes such names like any other; what the
           reference had flushed before it died is stored as "partial" outputs (a prefix of the right answer), the
           rest is pinned by tests/uniq_ref.py.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import uniq_inputs  # noqa: E402  (tests/uniq_inputs.py)

OUT = os.path.join(HERE, "uniq")
INLINE_LIMIT = 2 << 10
TIMES = re.compile(rb"at \d+\.\d{3} s")


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "gzfastq_uniq_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", ref, "-I", os.path.join(ref, "hiredis"), os.path.join(ref, "gzfastq_uniq.c"),
                           os.path.join(ref, "hiredis", "sds.c"), os.path.join(ref, "hiredis", "dict.c"), "-o", exe, "-lz"])
    return exe


def cases():
    c = []

    def add(cid, in1, in2=None, dups=False, out=True, ub=False, hash_size=None, u=None):
        c.append({"id": cid, "in1": in1, "in2": in2, "dups": dups, "out": out, "ub": ub, "hash_size": hash_size, "u": u})

    for f in ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
              "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]:
        add(f.replace(".", "_"), "fastq/" + f)
    add("dups5000", "uniq/inputs/dups5000.fq", dups=True)
    add("refine", "uniq/inputs/refine.fq", dups=True)
    add("equal_sums", "uniq/inputs/equal_sums.fq", dups=True)
    add("hibytes", "uniq/inputs/hibytes.fq", dups=True)
    add("crlf_dups", "uniq/inputs/crlf_dups.fq", dups=True)
    add("nonl_dups", "uniq/inputs/nonl_dups.fq", dups=True)
    add("lone_line", "uniq/inputs/lone_line.fq", dups=True)
    add("shortq", "uniq/inputs/shortq.fq", ub=True)
    add("fields3", "uniq/inputs/fields3.fq", dups=True)
    add("nul_bytes", "uniq/inputs/nul_bytes.fq", dups=True)
    add("no_dash_o", "uniq/inputs/equal_sums.fq", out=False)
    for u in (3, 5, 9, 17, 33, 65, 129, 1025):
        add("u%d" % u, "uniq/inputs/u%d.fq" % u, dups=True)
    for u in (4, 8, 16, 32, 64, 128, 1024):
        add("u%d_plain" % u, "uniq/inputs/u%d_plain.fq" % u, dups=True, hash_size=u, u=u)
        add("u%d_behind" % u, "uniq/inputs/u%d_behind.fq" % u, dups=True, hash_size=2 * u, u=u)
    for u in (4, 8, 16, 64):
        add("pu%d_plain" % u, "uniq/inputs/pu%d_plain_1.fq" % u, "uniq/inputs/pu%d_plain_2.fq" % u, dups=True, hash_size=u, u=u)
        add("pu%d_behind" % u, "uniq/inputs/pu%d_behind_1.fq" % u, "uniq/inputs/pu%d_behind_2.fq" % u, dups=True, hash_size=2 * u, u=u)
    add("pe_ab", "uniq/inputs/pe_a.fq", "uniq/inputs/pe_b.fq", dups=True)
    add("pe_equal_mates", "uniq/inputs/pe_a.fq", "uniq/inputs/pe_same.fq", dups=True)
    add("pe_ambiguous", "uniq/inputs/pe_amb_1.fq", "uniq/inputs/pe_amb_2.fq", dups=True)
    add("pe_badmid", "uniq/inputs/pe_a.fq", "uniq/inputs/pe_b_badmid.fq", dups=True)
    add("pe_mate_short", "uniq/inputs/pe_a.fq", "uniq/inputs/pe_b_short.fq", dups=True)
    add("pe_mate_long", "uniq/inputs/pe_a.fq", "uniq/inputs/pe_b_long.fq", dups=True)
    add("pe_nospace_equal", "uniq/inputs/pe_ns_a.fq", "uniq/inputs/pe_ns_eq.fq", dups=True)
    add("pe_nospace_unequal", "uniq/inputs/pe_ns_a.fq", "uniq/inputs/pe_ns_ne.fq", dups=True)
    add("pe_gzip_and_plain", "uniq/inputs/pe_a.fq", "uniq/inputs/pe_b.fq.gz", dups=True)
    add("pe_syn_var", "fastq/syn_var_a.fq", "fastq/syn_var_b.fq.gz")
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = uniq_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len("uniq/inputs/"):]) if rel.startswith("uniq/inputs/") else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            cmd = [exe, "-1", where(c["in1"])] + (["-2", where(c["in2"])] if c["in2"] else []) + (["-o", "o"] if c["out"] else [])
            p = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, "MALLOC_CHECK_": "0"})
            err = TIMES.sub(b"at T s", p.stderr)
            loaded = b"Finished load hash at T s\n" in err
            if p.returncode == 0 and not c["ub"]:
                expect = "same"
            elif p.returncode < 0 and loaded and c["out"]:
                expect = "diverge"
            else:
                expect = "refuse"
            assert p.returncode <= 0 and (p.returncode == 0 or p.returncode in (-6, -11)), (c["id"], p.returncode)
            if expect != "same":   # only what the reference printed while it was still sound
                err = err[:err.index(b"Finished load hash at T s\n") + 26] if loaded else b""
            entry = {"id": c["id"], "in1": c["in1"], "in2": c["in2"], "out": c["out"], "rc": p.returncode, "expect": expect,
                     "stderr": err.decode("latin-1"), "outputs": []}
            for fn in sorted(os.listdir(work)) if expect != "refuse" else []:
                text = open(os.path.join(work, fn), "rb").read()
                o = {"name": fn, "size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None, "partial": expect == "diverge"}
                if text and (len(text) <= INLINE_LIMIT or (expect == "diverge" and len(text) <= 16 << 10)):
                    o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
                elif expect == "diverge":
                    continue   # (a prefix cannot be pinned by a digest)
                entry["outputs"].append(o)
            m = re.search(r"unique reads number = (\d+)\(\d+ / (\d+) = ", entry["stderr"])
            if c["dups"]:
                assert m and 0 < int(m.group(1)) < int(m.group(2)), (c["id"], entry["stderr"])
            if c["hash_size"] is not None:
                assert expect == "same" and ("hash size: %d\n" % c["hash_size"]) in entry["stderr"], (c["id"], entry["stderr"])
                assert int(m.group(1)) == c["u"], (c["id"], entry["stderr"])
            manifest.append(entry)
            print("%-22s rc %4d  %-8s %s" % (c["id"], p.returncode, expect, (m.group(0) if m else "")))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    total = sum(os.path.getsize(os.path.join(dp, fn)) for dp, _, fs in os.walk(OUT) for fn in fs)
    print("%d cases, %d bytes under %s" % (len(manifest), total, OUT))


if __name__ == "__main__":
    main()
