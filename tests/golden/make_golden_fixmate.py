#!/usr/bin/env python3
"""Records what the reference's `samtools fixmate` does: tests/golden/fixmate/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of tests/golden/make_golden_bai.py, into a TEMPORARY
directory, bam_mate.c of the same tarball beside it, and both are linked to a driver of our own that calls bam_mating(argc, argv)
-- the function behind `samtools fixmate`.  Every case runs in a directory of its own under a limit of 20 s with its input
written there as in.bam, once without and once with -r.  Status, stderr, the directory's listing afterwards and the output (size +
SHA-256; whole, base64, up to 2 KiB) are stored as data.  No reference text is stored and nothing compiled stays.  The inputs come
from tests/fixmate_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, the tests make them again and
check it.

"expect" is `same` for every case the reference finishes inside its own memory; `refuse` where it crashed, ran past the limit or
reads memory that is not its own (UNDEFINED below: what it writes then is whatever lay there), with the reason in "why".  Before
anything is written the sequential restatement tests/fixmate_ref.py is held to every finished run."""
import base64
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fixmate_inputs  # noqa: E402  (tests/fixmate_inputs.py)
import fixmate_ref  # noqa: E402
import make_golden_bai  # noqa: E402  (the recipe: sources, flags)

OUT = os.path.join(HERE, "fixmate")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 20
DRIVER = "int bam_mating(int argc, char *argv[]);\nint main(int argc, char *argv[])\n{\n    return bam_mating(argc, argv);\n}\n"
UNDEFINED = {"op_eleven_carried": "BAM_CIGAR_STR is read past its NUL (op 11 in a CT field)",
             "tid_beyond_header": "target_len is read past its end (refID 3 of 3 targets)"}


def build_reference(ref, tmp):
    make_golden_bai.build_reference(ref, tmp)          # libbam.a under tmp/samtools-0.1.19
    sam = os.path.join(tmp, "samtools-0.1.19")
    subprocess.check_call(["gcc", "-c", "-g", "-O2", "-w"] + make_golden_bai.SAM_DFLAGS + ["-I.", "bam_mate.c", "-o", "bam_mate.o"], cwd=sam)
    drv = os.path.join(tmp, "fixmate_driver.c")
    with open(drv, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "fixmate")          # (argv[0] is `fixmate`, as samtools hands it to bam_mating)
    subprocess.check_call(["gcc", "-O2", "-w", drv, os.path.join(sam, "bam_mate.o"), "-o", exe, "-L", sam, "-lbam", "-lpthread", "-lm", "-lz"])
    return exe


def cases(inputs):
    """id, input (None: no input is written), args, out ('out.bam', 'stdout' or None), stdin (the input comes through a pipe)"""
    c = []
    for n in sorted(inputs):
        c.append({"id": n, "input": n, "args": ["in.bam", "out.bam"]})
        c.append({"id": n + "_r", "input": n, "args": ["-r", "in.bam", "out.bam"]})
    c.append({"id": "mixed_stdout", "input": "mixed", "args": ["in.bam", "-"], "out": "stdout"})
    c.append({"id": "mixed_stdin", "input": "mixed", "args": ["-", "out.bam"], "stdin": True})
    c.append({"id": "mixed_pipe_r", "input": "mixed", "args": ["-r", "-", "-"], "out": "stdout", "stdin": True})
    c.append({"id": "one_argument", "input": "mixed", "args": ["in.bam"], "out": None})
    c.append({"id": "one_argument_r", "input": "mixed", "args": ["-r", "in.bam"], "out": None})
    c.append({"id": "no_arguments", "input": None, "args": [], "out": None})
    c.append({"id": "missing_input", "input": None, "args": ["nope.bam", "out.bam"]})
    for e in c:
        e.setdefault("out", "out.bam")
        e.setdefault("stdin", False)
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    manifest = []
    inputs = fixmate_inputs.own_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        for c in cases(inputs):
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            data = inputs[c["input"]] if c["input"] else None
            given = [fixmate_inputs.materialize(work, c["input"], data)] if c["input"] else []
            why = UNDEFINED.get(c["input"]) if len(c["args"]) >= 2 else None
            try:
                feed = {"input": data} if c["stdin"] else {"stdin": subprocess.DEVNULL}
                p = subprocess.run([exe] + c["args"], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT, **feed)
                rc, err, out = p.returncode, p.stderr.decode("latin-1"), p.stdout
                if rc < 0:
                    why = "the reference ends with signal %d" % -rc
            except subprocess.TimeoutExpired:
                rc, err, out = None, "", b""
                why = "the reference runs past %d s" % TIME_LIMIT
            listing = sorted(fn for fn in os.listdir(work) if fn not in given)
            got = None
            remove = "-r" in c["args"]
            if why is None:
                assert rc in (0, 1), (c["id"], rc)
                if c["out"] == "stdout":
                    got = out
                    assert listing == [], (c["id"], listing)
                else:
                    assert out == b"" and listing in ([], ["out.bam"]), (c["id"], listing)
                    if listing:
                        got = open(os.path.join(work, "out.bam"), "rb").read()
                if c["out"] is not None and data is not None:       # the restatement against the recording
                    want, want_err, want_rc = fixmate_ref.fixmate(data, remove)
                    if c["stdin"]:      # (a finding: the check for the EOF marker cannot seek in a pipe and says the marker is absent)
                        want_err = fixmate_ref.MSG_NO_EOF
                    assert want_rc == rc, (c["id"], want_rc, rc)
                    assert want_err == err, (c["id"], want_err, err)
                    assert want == got, (c["id"], None if want is None else len(want), None if got is None else len(got))
                else:
                    assert (rc, err, got) == (1, fixmate_ref.USAGE, None), (c["id"], rc, err)
            else:
                err, rc, listing, got = "", None, [], None
            route = "host"
            if why is None and rc == 0 and c["input"] and not c["stdin"] and c["out"] == "out.bam":
                route = fixmate_ref.route(data)
            e = {"id": c["id"], "input": c["input"], "args": c["args"], "out": c["out"], "stdin": c["stdin"], "rc": rc, "stderr": err, "listing": listing,
                 "expect": "refuse" if why else "same", "why": why, "route": route, "bam": None}
            if got is not None:
                e["bam"] = {"size": len(got), "sha256": hashlib.sha256(got).hexdigest(),
                            "b64": base64.b64encode(got).decode() if len(got) <= INLINE_LIMIT else None}
            manifest.append(e)
            print("%-28s rc %5s  %-6s %-6s %8s bytes  %s" % (c["id"], rc, e["expect"], e["route"], "-" if got is None else len(got),
                                                           (why or err.strip().replace("\n", " | "))[:100]))
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(fixmate_inputs.digests(), sort_keys=True))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
