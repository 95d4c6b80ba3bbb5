#!/usr/bin/env python3
"""Records what the reference's `samtools index` does: tests/golden/bai/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of oracle/Makefile, into a TEMPORARY directory and
linked to a driver of our own that calls its bam_index(argc, argv) -- the function behind `samtools index`.  Every case runs in
a directory of its own under a limit of 20 s with its input copied there as in.bam.  Status, stderr and the index (whole, base64,
up to 2 KiB; else size + SHA-256) are stored as data.  No reference text is stored and nothing compiled stays.  The inputs that
are not fixtures of tests/golden/bam/ come from tests/bai_inputs.py (fixed seeds) and are NOT stored: the manifest holds their
SHA-256, the tests make them again and check it.

"expect" is `same` for every case the reference finishes; `refuse` (the tool leaves with status 2) only where it crashed or ran
past the limit, with the reason in "why".  Before anything is written the sequential restatement tests/bai_ref.py is held to
every recorded run."""
import base64
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bai_inputs  # noqa: E402  (tests/bai_inputs.py)
import bai_ref  # noqa: E402

OUT = os.path.join(HERE, "bai")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 20
LIBBAM_SRC = ("bgzf.c kstring.c bam_aux.c bam.c bam_import.c sam.c bam_index.c bam_pileup.c bam_lpileup.c bam_md.c razf.c faidx.c bedidx.c "
              "knetfile.c bam_sort.c sam_header.c bam_reheader.c kprobaln.c bam_cat.c").split()      # oracle/Makefile
SAM_DFLAGS = ["-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE64_SOURCE", "-D_USE_KNETFILE"]
DRIVER = "int bam_index(int argc, char *argv[]);\nint main(int argc, char *argv[])\n{\n    return bam_index(argc, argv);\n}\n"


def build_reference(ref, tmp):
    with tarfile.open(os.path.join(ref, "samtools-0.1.19.tar.bz2")) as t:
        t.extractall(tmp)
    sam = os.path.join(tmp, "samtools-0.1.19")
    objs = []
    for f in LIBBAM_SRC:
        subprocess.check_call(["gcc", "-c", "-g", "-O2", "-w"] + SAM_DFLAGS + ["-I.", f, "-o", f[:-2] + ".o"], cwd=sam)
        objs.append(f[:-2] + ".o")
    subprocess.check_call(["ar", "-csr", "libbam.a"] + objs, cwd=sam)
    drv = os.path.join(tmp, "index_driver.c")
    with open(drv, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "index")          # (argv[0] is `index`, as samtools hands it to bam_index)
    subprocess.check_call(["gcc", "-O2", "-w", drv, "-o", exe, "-L", sam, "-lbam", "-lpthread", "-lm", "-lz"])
    return exe


def cases():
    c = [{"id": n, "input": n, "args": ["in.bam"], "out": "in.bam.bai"} for n in bai_inputs.names()]
    c.append({"id": "explicit_out", "input": "mixed", "args": ["in.bam", "out.index"], "out": "out.index"})
    c.append({"id": "missing_input", "input": None, "args": ["nope.bam"], "out": "nope.bam.bai"})
    c.append({"id": "no_arguments", "input": None, "args": [], "out": None})
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = bai_inputs.materialize(made)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            data = None
            if c["input"]:
                data = open(bai_inputs.path_of(c["input"], made), "rb").read()
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
            made_files = sorted(fn for fn in os.listdir(work) if fn != "in.bam")
            bai = None
            if why is None:
                assert not out and rc in (0, 1), (c["id"], rc, out)
                assert made_files in ([], [c["out"]]), (c["id"], made_files)
                if made_files:
                    bai = open(os.path.join(work, c["out"]), "rb").read()
                if data is not None:       # the restatement against the recording
                    got_bai, got_err = bai_ref.index(data)
                    assert got_err == err, (c["id"], got_err, err)
                    assert got_bai == bai, (c["id"], None if got_bai is None else len(got_bai), None if bai is None else len(bai))
            else:
                err, rc = "", None
            e = {"id": c["id"], "input": c["input"], "args": c["args"], "out": c["out"], "rc": rc, "stderr": err, "expect": "refuse" if why else "same",
                 "why": why, "bai": None}
            if bai is not None:
                e["bai"] = {"size": len(bai), "sha256": hashlib.sha256(bai).hexdigest(),
                            "b64": base64.b64encode(bai).decode() if len(bai) <= INLINE_LIMIT else None}
            manifest.append(e)
            print("%-24s rc %5s  %-6s %8s bytes  %s" % (c["id"], rc, e["expect"], "-" if bai is None else len(bai), (why or err.strip().replace("\n", " | "))[:110]))
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
