#!/usr/bin/env python3
"""Records what the reference's gzfastq_mrle does: tests/golden/mrle/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  gzfastq_mrle.c is compiled
with list.c into a TEMPORARY directory and run on the cases below, each in a directory of its own under a limit of 5 s, its
standard output captured through a PIPE (with a prefix that begins with '-' the packed file and the decoded text share that
descriptor, and what arrives depends on stdio's buffers: tests/mrle_ref.py, shared).  Output bytes, stderr (the run times masked)
and exit status or signal are stored as data.  No reference text is stored and nothing compiled stays.  Outputs of up to 2 KiB are
kept in the manifest (bytes as the code points 0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of
tests/golden/fastq/ come from tests/mrle_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the
tests make them again and check it.  Re-running reproduces the file byte for byte.

What a case expects of the tool here ("expect"), with the reason in "why":
  same     the reference finished with status 0 on an input of the codec's domain: its bytes, stderr and status are the tool's.
  refuse   "crash": the reference ended on a signal; "damaged stream": the gzip stream fails its CRC-32 / ISIZE check, which the
           reference never looks at; "out-of-domain byte": a quality byte outside  # / 7 < B F  -- the codec indexes an 8-entry
           table on its stack at 255 there, reading and writing it, so nothing of that run is kept whatever its status was.  This
           covers crlf.fq (a '\\r' ends every quality line) and the files of tests/golden/fastq/ whose quality is 'I'.  Status 2.
  usage    no argument, -h, or an unknown option: usage on stderr, status 1 (the usage text is the tool's own).
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
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mrle_inputs  # noqa: E402  (tests/mrle_inputs.py)
import mrle_ref  # noqa: E402
from uniq_ref import NoAnswer, records  # noqa: E402

OUT = os.path.join(HERE, "mrle")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 5
TIMES = re.compile(rb"at \d+\.\d{3} s")
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_uniq.py's list
OWN = "mrle/inputs/"
FILE_ARGS = ["-i", "{in}", "-o", "o"]


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "gzfastq_mrle_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", ref, os.path.join(ref, "gzfastq_mrle.c"), os.path.join(ref, "list.c"), "-o", exe, "-lz"])
    return exe


def cases():
    c = []

    def add(cid, inp, args=None, stdin=None):
        """args: the command line behind the program's name; "{in}" stands for the input's path.  stdin: None or "file" (the input
        is the process's standard input)."""
        c.append({"id": cid, "in": inp, "args": FILE_ARGS if args is None else args, "stdin": stdin})

    for f in FASTQ:
        add("g_" + f.replace(".", "_"), "fastq/" + f)
    names = sorted(n[:-3] for n in mrle_inputs.own_inputs())
    for name in names:
        add("f_" + name, OWN + name + ".fq")
    for name in names:      # the packed file and the text on one descriptor
        add("s_" + name, OWN + name + ".fq", ["-i", "{in}", "-o", "-"])
    add("opt_n", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-n"])
    add("opt_s_n", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-s", "-n"])
    add("opt_n_s", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-n", "-s"])
    add("o_twice", OWN + "plain12.fq", ["-o", "a", "-i", "{in}", "-o", "b"])
    add("no_o", OWN + "reads150.fq", ["-i", "{in}"])
    add("o_dash_x", OWN + "reads150.fq", ["-i", "{in}", "-o", "-x", "-n"])
    add("opt_r", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-r", "5"])
    add("stdin_file", OWN + "mixed.fq", ["-o", "o"], "file")
    add("stdin_dash", OWN + "mixed.fq", ["-i", "-", "-o", "o"], "file")
    add("stdin_shared", OWN + "reads150.fq", ["-s"], "file")
    add("missing_file", None, ["-i", "no_such_file.fq", "-o", "o"])
    add("no_arguments", None, [])
    add("help", None, ["-h"])
    return c


def blob(text):
    o = {"size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None}
    if text and len(text) <= INLINE_LIMIT:
        o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
    return o


def classify(raw, is_gz):
    """None when the input lies in the codec's domain, else why it does not -- decided from the INPUT alone."""
    if is_gz:
        try:
            raw = gzip.decompress(raw)
        except (zlib.error, gzip.BadGzipFile, EOFError):
            return "damaged stream"
    try:
        quals = [r[2] for r in records(raw)]
    except NoAnswer:
        return "crash"
    return "out-of-domain byte" if mrle_ref.first_bad(quals) is not None else None


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = mrle_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len(OWN):]) if rel.startswith(OWN) else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            path = where(c["in"]) if c["in"] else None
            raw = open(path, "rb").read() if path else b""
            cmd = [exe] + [path if a == "{in}" else a for a in c["args"]]
            p = subprocess.run(cmd, cwd=work, stdin=open(path, "rb") if c["stdin"] == "file" else subprocess.DEVNULL, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, env={**os.environ, "MALLOC_CHECK_": "0"}, timeout=TIME_LIMIT)
            rc, stdout = p.returncode, p.stdout
            files = {fn: open(os.path.join(work, fn), "rb").read() for fn in sorted(os.listdir(work))}
            files.pop("no_such_file.fq", None)     # (the reference creates a missing input: O_CREAT)
            err = TIMES.sub(b"at T s", p.stderr)
            why = classify(raw, bool(c["in"]) and c["in"].endswith(".gz"))
            if rc == 1 and b"Usage" in p.stderr:
                assert not stdout and not files, c["id"]
                expect, why = "usage", None
            elif why == "crash":
                assert rc in (-signal.SIGSEGV, -signal.SIGABRT, -signal.SIGBUS), (c["id"], rc)
                expect = "refuse"
            elif why:
                expect, rc = "refuse", (rc if rc < 0 else None)      # nothing of an undefined run is kept
            else:
                assert rc == 0, (c["id"], rc)
                expect = "same"
            entry = {"id": c["id"], "in": c["in"], "args": c["args"], "stdin": c["stdin"], "rc": rc, "expect": expect, "why": why,
                     "in_sha256": hashlib.sha256(raw).hexdigest() if path else None, "stderr": err.decode("latin-1") if expect == "same" else "",
                     "stdout": None, "outputs": []}
            if expect == "same":
                assert len(files) <= 1, c["id"]
                entry["stdout"] = blob(stdout)
                entry["outputs"] = [dict(blob(text), name=fn) for fn, text in files.items()]
            manifest.append(entry)
            print("%-26s rc %5s  %-7s %-18s stdout:%d %s" % (c["id"], rc, expect, why, len(stdout), " ".join("%s:%d" % (k, len(v)) for k, v in files.items())))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
