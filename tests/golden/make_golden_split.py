#!/usr/bin/env python3
"""Records what the reference's bamSplitChr does: tests/golden/split/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of oracle/Makefile, and bamSplitChr.c against it, all
into a TEMPORARY directory; every case runs in a directory of its own under a limit of 20 s with its inputs copied there as
in.bam (in2.bam) + .bai.  Status, stderr (times masked, the program's name as PROG) and, per output file, name, size, SHA-256, the
blocks' ISIZE fields, the SHA-256 of the inflated bytes and -- up to 2 KiB -- the whole file (base64) are stored as data.  No
reference text is stored and nothing compiled stays.  The inputs that are not fixtures of tests/golden/bam/ come from
tests/split_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, the tests make them again and check it.

The input of 300 targets (t300) is NOT recorded -- 600 files for its two levels --: the tests hold the tool and the ABI on it to
tests/split_ref.py, which the recorded `same` cases pin to the compiled reference (the manifest's "note" says the same).

What a case expects of the tool here ("expect"), with the reason in "why":
  same     the input lies inside the tool's domain (tests/split_ref.py classify: decided from the input alone) or the run ends
           before any record is read (a missing file, a missing index): status, masked stderr, file names and bytes are the tool's.
  refuse   outside the domain -- the reference's outputs depend on the index's chunk lists there: status 2, no output left.
  usage    -h or no argument: usage on stderr (the text is the tool's own), status 1.
"""
import base64
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import split_inputs  # noqa: E402  (tests/split_inputs.py)
import split_ref  # noqa: E402

OUT = os.path.join(HERE, "split")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 20
TIMES = re.compile(r"at \d+\.\d{3} s")
LIBBAM_SRC = ("bgzf.c kstring.c bam_aux.c bam.c bam_import.c sam.c bam_index.c bam_pileup.c bam_lpileup.c bam_md.c razf.c faidx.c bedidx.c "
              "knetfile.c bam_sort.c sam_header.c bam_reheader.c kprobaln.c bam_cat.c").split()      # oracle/Makefile
SAM_DFLAGS = ["-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE64_SOURCE", "-D_USE_KNETFILE"]
LEVEL0 = ["edges", "edges64", "oversize", "opts", "rand", "hdr_ff00", "hdr_ff01", "multiblock", "repack97", "all_empty"]
LEVEL1 = ["edges", "edges64", "oversize", "opts"]


def build_reference(ref, tmp):
    with tarfile.open(os.path.join(ref, "samtools-0.1.19.tar.bz2")) as t:
        t.extractall(tmp)
    sam = os.path.join(tmp, "samtools-0.1.19")
    objs = []
    for f in LIBBAM_SRC:
        subprocess.check_call(["gcc", "-c", "-g", "-O2", "-w"] + SAM_DFLAGS + ["-I.", f, "-o", f[:-2] + ".o"], cwd=sam)
        objs.append(f[:-2] + ".o")
    subprocess.check_call(["gcc", "-c", "-g", "-O2", "-w"] + SAM_DFLAGS + ["-DBGZF_CACHE", "-I.", "bgzf.c", "-o", "bgzf.o"], cwd=sam)
    subprocess.check_call(["ar", "-csr", "libbam.a"] + objs, cwd=sam)
    exe = os.path.join(tmp, "bamSplitChr_ref")
    subprocess.check_call(["gcc", "-O3", "-g", "-w", "-I", ref, "-I", sam, os.path.join(ref, "bamSplitChr.c"), "-o", exe, "-L", sam, "-lbam",
                           "-lpthread", "-lm", "-lz"])
    return exe


def cases():
    c = []

    def add(cid, inputs, args, bai=True):
        c.append({"id": cid, "inputs": inputs, "args": args, "bai": bai})

    names = split_inputs.FIXTURES + sorted(split_inputs.own_inputs())
    for n in names:
        if n != "t300":      # (300 output files: held to tests/split_ref.py by the tests, not recorded)
            add("d_" + n, [n], ["-o", "o", "in.bam"])
    for n in LEVEL0:
        add("u_" + n, [n], ["-u", "x", "-o", "o", "in.bam"])
    for n in LEVEL1:
        add("1_" + n, [n], ["-1", "x", "-o", "o", "in.bam"])
    add("u_eats_o", ["opts"], ["-u", "-o", "out", "in.bam"])
    add("no_o", ["opts"], ["in.bam"])
    add("two_inputs", ["opts", "one_each"], ["-o", "P", "in.bam", "in2.bam"])
    add("two_inputs_u", ["opts", "one_each"], ["-u", "x", "-o", "P", "in.bam", "in2.bam"])
    add("name_overrun", ["long_name"], ["-o", "p" * 60, "in.bam"])      # 60 + 1 + 200 + 4 bytes into fn_out[256]
    add("no_bai", ["opts"], ["-o", "o", "in.bam"], bai=False)
    add("missing_input", [], ["-o", "o", "nope.bam"])
    add("help", [], ["-h"])
    add("no_arguments", [], [])
    return c


def place(case, made, work):
    """the case's inputs as in.bam, in2.bam (+ .bai) in `work`; returns their names there"""
    there = []
    for k, name in enumerate(case["inputs"]):
        src, dst = split_inputs.path_of(name, made), os.path.join(work, "in.bam" if k == 0 else "in%d.bam" % (k + 1))
        shutil.copyfile(src, dst)
        if case["bai"]:
            shutil.copyfile(src + ".bai", dst + ".bai")
        there.append(os.path.basename(dst))
    return there


def prefixes(args, there):
    """the prefix every input gets: the reference's option loop (-u and -1 take an argument), -o for the first input only"""
    o, k = None, 0
    while k < len(args) and args[k].startswith("-") and len(args[k]) == 2 and args[k][1] in "owrsu1":
        if args[k] == "-o":
            o = args[k + 1]
        k += 2
    ins = args[k:]
    return ins, [o if (i == 0 and o is not None) else p for i, p in enumerate(ins)]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = split_inputs.materialize(made)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            there = set(place(c, made, work))
            there |= {t + ".bai" for t in there}
            try:
                p = subprocess.run([exe] + c["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT)
                rc, err, out = p.returncode, p.stderr.decode("latin-1"), p.stdout
            except subprocess.TimeoutExpired:
                rc, err, out = None, "", b""
            files = {fn: open(os.path.join(work, fn), "rb").read() for fn in sorted(os.listdir(work)) if fn not in there}
            err = TIMES.sub("at T s", err).replace(os.path.basename(exe) + ":", "PROG:")
            ins, pre = prefixes(c["args"], there)
            why = None
            for path, prefix in zip(ins, pre):
                full = os.path.join(work, path)
                if not os.path.exists(full) or not os.path.exists(full + ".bai"):
                    break                     # the run ends here, before any record
                k = split_ref.classify(split_ref.read(full), open(full + ".bai", "rb").read(), prefix)
                if k:
                    why = "%s: %s" % (path, " ".join(str(x) for x in k))
                    break
            if rc == 1 and "Usage" in err:
                assert not files, c["id"]
                expect, err = "usage", ""
            elif why:
                expect, rc, err, files = "refuse", None, "", {}
            else:
                assert rc in (0, 1) and not out, (c["id"], rc)
                expect = "same"
            entry = {"id": c["id"], "inputs": c["inputs"], "args": c["args"], "bai": c["bai"], "rc": rc, "expect": expect, "why": why, "stderr": err,
                     "outputs": []}
            for fn, data in files.items():
                d = dict(split_ref.describe(data), name=fn, b64=None)
                if len(data) <= INLINE_LIMIT:
                    d["b64"] = base64.b64encode(data).decode()
                entry["outputs"].append(d)
            manifest.append(entry)
            print("%-28s rc %5s  %-7s %-40s %d files" % (c["id"], rc, expect, why, len(files)))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"note": "t300 (300 targets of 0 - 2 records) is not recorded here: the tests hold the tool and the ABI on it to tests/split_ref.py, '
                'which the same-cases below pin to the compiled reference",\n "zlib": %s,\n "inputs": %s,\n "cases": [\n' % (json.dumps(zlib.ZLIB_RUNTIME_VERSION), json.dumps(digests, sort_keys=True)))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
