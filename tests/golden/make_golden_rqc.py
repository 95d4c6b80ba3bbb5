#!/usr/bin/env python3
"""Records what the reference's R plugin does: tests/golden/rqc/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  Rgzfastq_uniq.c and hashtbl.c
are compiled UNCHANGED, against the stand-in R.h / Rdefines.h of tests/golden/rshim/ and with its driver.c (which calls
qsort_hash_count as .Call would and dumps every element of the returned list), into a TEMPORARY directory, and run on the cases
below, each in a directory of its own under a limit of 5 s.  Stored as data: exit status or signal, stderr (the run times masked)
and the list -- element 1 inline up to 2 KiB, else its length and SHA-256; the matrices and the length vector as SHA-256 and, when
few, their non-zero cells; gc as SHA-256 of the raw doubles and the bit patterns of the first 8.  No reference text is stored and
nothing compiled stays.  The inputs that are not files of tests/golden/fastq/ come from tests/rqc_inputs.py (fixed seeds) and are
NOT stored: the manifest holds their SHA-256, and the tests make them again and check it.  Re-running reproduces the file byte for
byte.

What a case expects of the library and the tool here ("expect"), with the reason in "why":
  same     the plugin finished with status 0 on an input of its domain: its list and stderr lines are ours.
  refuse   "crash": the run ended on a signal; "damaged stream": the gzip stream fails its CRC-32 / ISIZE check, which the plugin
           never looks at; "out of domain": a sequence length outside 1..300, a quality line beyond 300 or a byte >= 128 -- the
           plugin writes outside its arrays there, so nothing of that run is kept whatever its status was; "mate short": mate 2
           runs out first (it dereferences NULL).  HPN_E_DOMAIN / status 2.
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

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rqc_inputs  # noqa: E402  (tests/rqc_inputs.py)
import rqc_ref  # noqa: E402

OUT = os.path.join(HERE, "rqc")
SHIM = os.path.join(HERE, "rshim")
INLINE_LIMIT = 2 << 10
CELL_LIMIT = 48
TIME_LIMIT = 5
TIMES = re.compile(rb"at \d+\.\d{3} s")
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_mrle.py's list
OWN = "rqc/inputs/"
REASONS = {rqc_ref.BAD_LENGTH: "out of domain", rqc_ref.BAD_QUALITY: "out of domain", rqc_ref.BAD_BYTE: "out of domain", rqc_ref.MATE_SHORT: "mate short"}


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "rqc_ref_driver")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", SHIM, "-I", ref, os.path.join(ref, "Rgzfastq_uniq.c"), os.path.join(ref, "hashtbl.c"),
                           os.path.join(SHIM, "driver.c"), "-o", exe, "-lz"])
    return exe


def cases():
    c = [{"id": "g_" + f.replace(".", "_"), "in": ["fastq/" + f]} for f in FASTQ]
    c.append({"id": "g_pair_t", "in": ["fastq/t.fq", "fastq/t.fq.gz"]})
    c.append({"id": "g_pair_syn_var", "in": ["fastq/syn_var_a.fq", "fastq/syn_var_b.fq.gz"]})
    for name, mates in sorted(rqc_inputs.own_inputs().items()):
        c.append({"id": name, "in": [OWN + "%s.%d.fq" % (name, m + 1) for m, t in enumerate(mates) if t is not None]})
    return c


def element(k, raw):
    """Element k (0-based) of the list, from its raw cells."""
    o = {"bytes": len(raw), "sha256": hashlib.sha256(raw).hexdigest()}
    if k == 0:
        o["values"] = np.frombuffer(raw, "<i4").tolist() if len(raw) <= INLINE_LIMIT else None
    elif k % 4 == 1:
        o["first"] = np.frombuffer(raw[:64], "<u8").tolist()      # the first doubles' bit patterns
    else:
        a = np.frombuffer(raw, "<i4")
        nz = np.nonzero(a)[0]
        o["cells"] = [[int(i), int(a[i])] for i in nz] if len(nz) <= CELL_LIMIT else None
    return o


def classify(raws, gz):
    """None when the input lies in the plugin's domain, else (why, record, mate, reason) -- decided from the INPUT alone."""
    texts = []
    for raw, is_gz in zip(raws, gz):
        if is_gz:
            try:
                raw = gzip.decompress(raw)
            except (zlib.error, gzip.BadGzipFile, EOFError):
                return ("damaged stream", None, None, None)
        texts.append(raw)
    try:
        rqc_ref.tally(*texts)
    except rqc_ref.NoAnswer as e:
        return (REASONS[e.reason], e.record, e.mate, e.reason)
    except rqc_ref._NoAnswer:
        return ("crash", None, None, None)
    return None


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = rqc_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len(OWN):]) if rel.startswith(OWN) else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            paths = [where(r) for r in c["in"]]
            raws = [open(p, "rb").read() for p in paths]
            p = subprocess.run([exe] + paths, cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               env={**os.environ, "MALLOC_CHECK_": "0"}, timeout=TIME_LIMIT)
            rc = p.returncode
            why = classify(raws, [r.endswith(".gz") for r in c["in"]])
            entry = {"id": c["id"], "in": c["in"], "in_sha256": [hashlib.sha256(r).hexdigest() for r in raws], "rc": rc, "expect": "same", "why": None,
                     "bad": None, "stderr": "", "list": []}
            if why is None:
                assert rc == 0, (c["id"], rc, p.stderr)
                n = int(p.stdout.split()[1])
                assert n == (9 if len(paths) > 1 else 5), (c["id"], p.stdout)
                entry["stderr"] = TIMES.sub(b"at T s", p.stderr).decode("latin-1")
                entry["list"] = [element(k, open(os.path.join(work, "e%d.bin" % k), "rb").read()) for k in range(n)]
            else:
                entry["expect"], entry["why"] = "refuse", why[0]
                if why[1] is not None:
                    entry["bad"] = {"record": why[1], "mate": why[2], "reason": why[3]}
                if why[0] in ("crash", "mate short"):
                    assert rc in (-signal.SIGSEGV, -signal.SIGABRT, -signal.SIGBUS), (c["id"], rc)
                else:
                    entry["rc"] = rc if rc < 0 else None      # nothing of an undefined run is kept
            manifest.append(entry)
            print("%-22s rc %5s  %-7s %-14s %s" % (c["id"], rc, entry["expect"], entry["why"], entry["stderr"].split("\n")[2] if entry["stderr"] else ""))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
