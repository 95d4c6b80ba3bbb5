#!/usr/bin/env python3
"""Records what the reference's `samtools rmdup` does: tests/golden/rmdup/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of tests/golden/make_golden_bai.py, into a TEMPORARY
directory; bam_rmdup.c and bam_rmdupse.c of the same tarball are compiled beside it and linked to a driver of our own that calls
bam_rmdup(argc, argv) -- the function behind `samtools rmdup`.  Every case runs in a directory of its own under a limit of 20 s
with its input copied there as in.bam.  Status, stderr, the directory's listing afterwards and the output (size + SHA-256; whole,
base64, up to 2 KiB) are stored as data.  No reference text is stored and nothing compiled stays.  The inputs come from
tests/rmdup_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, the tests make them again and check it.

"expect" is `same` for every case the reference finishes; `refuse` only where it crashed or ran past the limit, with the reason
in "why".  Before anything is written the sequential restatement tests/rmdup_ref.py is held to every finished run."""
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
import make_golden_bai  # noqa: E402  (the recipe: sources, flags)
import rmdup_inputs  # noqa: E402  (tests/rmdup_inputs.py)
import rmdup_ref  # noqa: E402

OUT = os.path.join(HERE, "rmdup")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 20
DRIVER = "int bam_rmdup(int argc, char *argv[]);\nint main(int argc, char *argv[])\n{\n    return bam_rmdup(argc, argv);\n}\n"


def build_reference(ref, tmp):
    make_golden_bai.build_reference(ref, tmp)          # libbam.a under tmp/samtools-0.1.19
    sam = os.path.join(tmp, "samtools-0.1.19")
    drv = os.path.join(tmp, "rmdup_driver.c")
    with open(drv, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "rmdup")          # (argv[0] is `rmdup`, as samtools hands it to bam_rmdup)
    subprocess.check_call(["gcc", "-O2", "-w"] + make_golden_bai.SAM_DFLAGS + ["-I", sam, drv, os.path.join(sam, "bam_rmdup.c"), os.path.join(sam, "bam_rmdupse.c"),
                           "-o", exe, "-L", sam, "-lbam", "-lpthread", "-lm", "-lz"])
    return exe


def cases():
    c = [{"id": n, "input": n, "opts": []} for n in rmdup_inputs.names_of_inputs()]
    for n in ("mixed", "se_reverse", "tails", "first_unplaced", "no_records"):
        c.append({"id": n + "_s", "input": n, "opts": ["-s"]})
        c.append({"id": n + "_S", "input": n, "opts": ["-S"]})
    c.append({"id": "missing_input", "input": None, "opts": [], "args": ["nope.bam", "out.bam"]})
    c.append({"id": "one_argument", "input": "mixed", "opts": [], "args": ["in.bam"]})
    c.append({"id": "no_arguments", "input": None, "opts": [], "args": []})
    for e in c:
        e.setdefault("args", e["opts"] + ["in.bam", "out.bam"])
        e["out"] = None if len(e["args"]) < 2 else "out.bam"
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = rmdup_inputs.materialize(made)
        inputs = rmdup_inputs.own_inputs()
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            data = inputs[c["input"]] if c["input"] else None
            if data is not None:
                with open(os.path.join(work, "in.bam"), "wb") as fh:
                    fh.write(data)
            why = None
            try:
                p = subprocess.run([exe] + c["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT)
                rc, err, out = p.returncode, p.stderr.decode("latin-1"), p.stdout
                if rc < 0:
                    why = "the reference ends with signal %d" % -rc
            except subprocess.TimeoutExpired:
                rc, err, out = None, "", b""
                why = "the reference runs past %d s" % TIME_LIMIT
            listing = sorted(fn for fn in os.listdir(work) if fn != "in.bam")
            got, route = None, "host"
            if why is None:
                assert rc in (0, 1) and out == b"" and listing in ([], [c["out"]]), (c["id"], rc, listing)
                if listing:
                    got = open(os.path.join(work, c["out"]), "rb").read()
                if data is not None and c["out"]:       # the restatement against the recording
                    want, want_err, _ = rmdup_ref.rmdup(data, **rmdup_ref.options(c["opts"]))
                    assert want_err == err, (c["id"], want_err, err)
                    assert want == got, (c["id"], len(want), None if got is None else len(got))
                    route = "host" if c["opts"] else rmdup_ref.route(data)
            else:
                err, rc, listing = "", None, []
            e = {"id": c["id"], "input": c["input"], "opts": c["opts"], "args": c["args"], "out": c["out"], "rc": rc, "stderr": err, "listing": listing,
                 "expect": "refuse" if why else "same", "why": why, "route": route, "bam": None}
            if got is not None:
                e["bam"] = {"size": len(got), "sha256": hashlib.sha256(got).hexdigest(),
                            "b64": base64.b64encode(got).decode() if len(got) <= INLINE_LIMIT else None}
            manifest.append(e)
            print("%-20s rc %5s  %-6s %-6s %8s bytes  %s" % (c["id"], rc, e["expect"], e["route"], "-" if got is None else len(got),
                                                           (why or err.strip().replace("\n", " | "))[:110]))
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
