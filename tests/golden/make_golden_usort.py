#!/usr/bin/env python3
"""Records what the reference gzfastq_uniq_sort does: tests/golden/usort/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  The reference tool is
compiled into a TEMPORARY directory -- gzfastq_uniq_sort.c with hashtbl.c -- and run on the cases below, each in a directory of
its own into which the inputs are copied as r1.fq / r2.fq (.gz kept), so that the names it prints and derives its outputs from
do not depend on where this runs.  Its outputs AFTER GUNZIP (the compressed bytes depend on the zlib build), stderr (the run
times masked) and exit status or signal are stored as data.  No reference text is stored and nothing compiled stays.  Outputs
of up to 2 KiB are kept in the manifest (bytes as the code points 0 .. 255), larger ones as length + SHA-256 only.  The inputs
that are not files of tests/golden/fastq/ come from tests/usort_inputs.py (fixed seeds) and are NOT stored: the manifest holds
their SHA-256, and the tests make them again and check it.  Re-running reproduces the file byte for byte.

What a case expects of the tool here ("expect"):
  same     the reference finished: the gunzipped bytes, stderr and status are the tool's.
  refuse   the reference crashed (signal), or its result is undefined by construction ("constructed": a pair's key shorter
           than strLen, a joined key of more than 1023 bytes -- nothing of the reference's run is kept then): status 2.
  usage    no argument, or -h: usage on stderr, status 1 (the usage text is the tool's own).
"""
import gzip
import hashlib
import json
import os
import re
import shutil
import signal
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import usort_inputs  # noqa: E402  (tests/usort_inputs.py)

OUT = os.path.join(HERE, "usort")
INLINE_LIMIT = 2 << 10
TIMES = re.compile(rb"at \d+\.\d{3} s")
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_uniq.py's list
SE, PE = ["-1", "{1}", "-o", "o"], ["-1", "{1}", "-2", "{2}", "-o", "o"]


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "gzfastq_uniq_sort_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", ref, os.path.join(ref, "gzfastq_uniq_sort.c"), os.path.join(ref, "hashtbl.c"), "-o", exe, "-lz"])
    return exe


def cases():
    c = []

    def add(cid, in1, in2=None, args=None, constructed=False):
        c.append({"id": cid, "in1": in1, "in2": in2, "args": (PE if in2 else SE) if args is None else args, "constructed": constructed})

    own = lambda name: "usort/inputs/" + name
    for f in FASTQ:
        add(f.replace(".", "_"), "fastq/" + f)
    add("pe_syn_var", "fastq/syn_var_a.fq", "fastq/syn_var_b.fq.gz")      # pairs of them that have equal names
    add("pe_t_plain_gzip", "fastq/t.fq", "fastq/t.fq.gz")
    add("pe_syn_100_twice", "fastq/syn_100.fq.gz", "fastq/syn_100.fq.gz")
    add("pe_multi_twice", "fastq/multi.fq.gz", "fastq/multi.fq.gz")
    for n in (9, 10, 11):
        add("e%d" % n, own("n%d.fq" % n))
    for name in ("lone_only", "lone10", "lone_nl", "widths", "half", "keylens", "empty_first", "crlf12", "nonl12", "shortq12", "hibytes", "dups5000"):
        add(name, own(name + ".fq"))
    for u in usort_inputs.TIE_US:
        add("ties_u%d" % u, own("ties_u%d.fq" % u))
    add("pairs_mixed", own("pm_1.fq"), own("pm_2.fq"))
    add("pairs_dups", own("pd_1.fq"), own("pd_2.fq"))
    add("pe30", own("pe30_1.fq"), own("pe30_2.fq"))
    add("pe30_bad15", own("pe30_1.fq"), own("pe30_2bad15.fq"))
    add("pe30_mate_short", own("pe30_1.fq"), own("pe30_2short.fq"))
    add("pe30_mate_long", own("pe30_1.fq"), own("pe30_2long.fq"))
    add("pe_key_1023", own("p1023_1.fq"), own("p1023_2.fq"))
    add("pe_short_key", own("pshort_1.fq"), own("pshort_2.fq"), constructed=True)
    add("pe_long_key", own("plong_1.fq"), own("plong_2.fq"), constructed=True)
    add("o_before_1", own("widths.fq"), args=["-o", "o", "-1", "{1}"])
    add("o_before_1_pairs", own("pe30_1.fq"), own("pe30_2.fq"), args=["-o", "o", "-1", "{1}", "-2", "{2}"])
    add("no_o", own("widths.fq"), args=["-1", "{1}"])
    add("o_twice", own("widths.fq"), args=["-o", "a", "-1", "{1}", "-o", "b"])
    add("no_arguments", None, args=[])
    add("help", None, args=["-h"])
    return c


def blob(text):
    o = {"size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None}
    if text and len(text) <= INLINE_LIMIT:
        o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
    return o


def local_name(rel, k):
    return None if rel is None else "r%d.fq%s" % (k, ".gz" if rel.endswith(".gz") else "")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = usort_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len("usort/inputs/"):]) if rel.startswith("usort/inputs/") else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            names = [local_name(c["in1"], 1), local_name(c["in2"], 2)]
            for rel, name in zip((c["in1"], c["in2"]), names):
                if rel:
                    shutil.copy(where(rel), os.path.join(work, name))
            cmd = [exe] + [a.replace("{1}", names[0] or "").replace("{2}", names[1] or "") for a in c["args"]]
            p = subprocess.run(cmd, cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, "MALLOC_CHECK_": "0"})
            err = TIMES.sub(b"at T s", p.stderr)
            rc = p.returncode
            if c["in1"] is None:
                assert rc == 1 and b"Usage" in p.stderr and not p.stdout and not os.listdir(work), c["id"]
                expect, err = "usage", b""
            elif c["constructed"]:
                expect, err, rc = "refuse", b"", None
            elif rc == 0:
                expect = "same"
            else:
                assert rc in (-signal.SIGFPE, -signal.SIGSEGV, -signal.SIGABRT), (c["id"], rc)
                expect, err = "refuse", b""
            entry = {"id": c["id"], "in1": c["in1"], "in2": c["in2"], "args": c["args"], "name1": names[0], "name2": names[1], "rc": rc,
                     "constructed": c["constructed"], "expect": expect, "stderr": err.decode("latin-1"), "outputs": []}
            if expect == "same":
                assert not p.stdout, c["id"]
                for fn in sorted(set(os.listdir(work)) - set(names)):
                    assert fn.endswith(".gz"), (c["id"], fn)
                    entry["outputs"].append(dict(blob(gzip.decompress(open(os.path.join(work, fn), "rb").read())), name=fn))
                assert len(entry["outputs"]) == (2 if c["in2"] else 1), c["id"]
            manifest.append(entry)
            m = re.search(r"unique reads number = (\d+)\n", entry["stderr"])
            print("%-22s rc %5s  %-8s %s" % (c["id"], rc, expect, (m.group(0).strip() if m else "")))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
