#!/usr/bin/env python3
"""Records what the reference's pick_pair does: tests/golden/pair/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  pick_pair.c is compiled into a
TEMPORARY directory and run on the cases of tests/pair_inputs.py, each in a directory of its own under a limit of 5 s.  The inputs
are COPIED into that directory as a.fq / b.fq (a.fq.gz / b.fq.gz for gzip fixtures) and named without a path, so that a prefix
taken from -1 stays inside it.  The four outputs are stored INFLATED; with them stderr (the run times masked) and the exit status
or signal.  No reference text is stored and nothing compiled stays.  Outputs of up to 2 KiB are kept in the manifest (bytes as the
code points 0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of tests/golden/fastq/ come from
tests/pair_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the tests make them again and check it.
Re-running reproduces the file byte for byte.

What a case expects of the tool here ("expect"):
  same     the reference finished with status 0: its inflated outputs, stderr and status are the tool's.
  refuse   the reference crashed (signal): status 2, no outputs.
  damaged  an input is a gzip stream with a CRC-32 / ISIZE / data error: the tool refuses it (status 2) whatever the reference made
           of the bytes in front of the error -- nothing of its run is kept.
  usage    no argument, -h, or an unknown option: usage on stderr, status 1 (the usage text is the tool's own).
  missing  an input cannot be opened: "open file NAME failed", status 1, no outputs.
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
import pair_inputs  # noqa: E402  (tests/pair_inputs.py)

OUT = os.path.join(HERE, "pair")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 5
TIMES = re.compile(rb"at \d+\.\d{3} s")
OWN = pair_inputs.OWN
DEFAULT_ARGS = ["-1", "{a}", "-2", "{b}", "-o", "o"]


def blob(text):
    o = {"size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None}
    if text and len(text) <= INLINE_LIMIT:
        o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
    return o


def damaged(raw, gz):
    if not gz:
        return False
    try:
        gzip.decompress(raw)
        return False
    except (zlib.error, gzip.BadGzipFile, EOFError):
        return True


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pick_pair_ref")
        subprocess.check_call(["gcc", "-O2", "-w", os.path.join(ref, "pick_pair.c"), "-o", exe, "-lz"])
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = pair_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len(OWN):]) if rel.startswith(OWN) else os.path.join(HERE, rel)
        for c in pair_inputs.cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            local, raw, bad = {}, {}, False
            for side in ("a", "b"):
                if c[side]:
                    local[side] = side + (".fq.gz" if c[side].endswith(".gz") else ".fq")
                    raw[side] = open(where(c[side]), "rb").read()
                    bad = bad or damaged(raw[side], c[side].endswith(".gz"))
                    open(os.path.join(work, local[side]), "wb").write(raw[side])
            args = [local.get(a[1:-1], a) if a in ("{a}", "{b}") else a for a in (c["args"] if c["args"] is not None else DEFAULT_ARGS)]
            p = subprocess.run([exe] + args, cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               env={**os.environ, "MALLOC_CHECK_": "0"}, timeout=TIME_LIMIT)
            rc, err = p.returncode, TIMES.sub(b"at T s", p.stderr)
            assert p.stdout == b"", c["id"]
            files = {fn: open(os.path.join(work, fn), "rb").read() for fn in sorted(os.listdir(work)) if fn not in local.values()}
            if rc == 1 and b"Usage" in p.stderr:
                assert not files, c["id"]
                expect = "usage"
            elif rc == 1 and err.startswith(b"open file ") and c["route"] is None:
                assert not files, c["id"]
                expect = "missing"
            elif bad:
                expect, rc = "damaged", None
            elif rc == 0:
                expect = "same"
            else:
                assert rc in (-signal.SIGSEGV, -signal.SIGABRT, -signal.SIGBUS), (c["id"], rc)
                expect = "refuse"
            entry = {"id": c["id"], "a": c["a"], "b": c["b"], "args": args, "rc": rc, "expect": expect, "route": c["route"],
                     "a_sha256": hashlib.sha256(raw["a"]).hexdigest() if "a" in raw else None,
                     "b_sha256": hashlib.sha256(raw["b"]).hexdigest() if "b" in raw else None,
                     "stderr": err.decode("latin-1") if expect in ("same", "missing") else "", "outputs": []}
            if expect == "same":
                assert len(files) == 4 and all(fn.endswith(".fq.gz") for fn in files), (c["id"], sorted(files))
                entry["outputs"] = [dict(blob(gzip.decompress(data)), name=fn) for fn, data in files.items()]
            manifest.append(entry)
            print("%-26s rc %5s  %-7s %-8s %s" % (c["id"], rc, expect, c["route"], " ".join("%s:%d" % (o["name"], o["size"]) for o in entry["outputs"])))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
