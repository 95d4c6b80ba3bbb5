#!/usr/bin/env python3
"""Records what the reference gzfastq_sample does: tests/golden/sample/.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  The reference
sampler is compiled into a TEMPORARY directory -- gzfastq_sample.c with rng.c and common.c of the fastq-tools-0.7
tarball it ships, plus a one-line version.h -- run on the inputs below, and its DECOMPRESSED outputs, stderr (the
run times masked) and exit status are stored as data.  No reference text is stored.  Outputs above 16 KiB are kept
as length + SHA-256 only.  Re-running reproduces the directory byte for byte.
"""
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FASTQ = os.path.join(HERE, "fastq")
OUT = os.path.join(HERE, "sample")
INLINE_LIMIT = 16 << 10
TIMES = re.compile(rb"at \d+\.\d{3} s")


def build_reference(ref, tmp):
    with tarfile.open(os.path.join(ref, "fastq-tools-0.7.tar.gz")) as t:
        t.extractall(tmp)
    src = os.path.join(tmp, "fastq-tools-0.7", "src")
    with open(os.path.join(tmp, "version.h"), "w") as f:
        f.write('#define FASTQ_TOOLS_VERSION "0.7"\n')
    exe = os.path.join(tmp, "gzfastq_sample_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", tmp, "-I", src, "-I", ref, os.path.join(ref, "gzfastq_sample.c"),
                           os.path.join(src, "rng.c"), os.path.join(src, "common.c"), "-o", exe, "-lz"])
    return exe


def synth(seed, n, name, read_len=(20, 80)):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ln = int(rs.randint(read_len[0], read_len[1] + 1))
        seq = bytes(rs.choice(np.frombuffer(b"ACGTN", np.uint8), ln))
        qual = bytes(rs.randint(33, 74, ln).astype(np.uint8))
        out.append(name(rs, i) + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def long_name(rs, i):
    ln = int(rs.randint(100, 601))
    body = bytes(rs.randint(33, 127, ln).astype(np.uint8)).replace(b"@", b"a")
    return b"@" + body[:ln - 1]


def hibyte_name(rs, i):
    words = ["Probe-échantillon", "测序", "röd", "µL"]
    return ("@%s:%d:%d %s" % (words[i % 4], i, int(rs.randint(0, 1 << 30)), words[(i + 1) % 4])).encode("utf-8")


def illumina_name(rs, i):
    return b"@M01:77:000000000-AB1CD:1:%d:%d:%d 1:N:0:%d" % (1101 + i // 50, int(rs.randint(1000, 30000)), int(rs.randint(1000, 30000)), i % 12)


def own_inputs():
    """Inputs of this directory's own: long names (several wide loads per lane of the hash), bytes >= 0x80 in names
    (the hash takes them as signed chars), mates of equal, shorter and longer length."""
    a = synth(11, 60, illumina_name)
    b = synth(12, 60, lambda rs, i: illumina_name(rs, i).replace(b" 1:N", b" 2:N"))
    recs_b = b.split(b"\n")
    return {
        "longnames.fq": synth(7, 80, long_name),
        "hibyte.fq": synth(8, 40, hibyte_name),
        "mate_a.fq": a,
        "mate_b_equal.fq": b,
        "mate_b_short.fq": b"\n".join(recs_b[:4 * 37]) + b"\n",
        "mate_b_long.fq": b + synth(13, 9, lambda rs, i: b"@extra%d" % i),
    }


# (id, first input, mate or None, arguments, "mixed": kept and dropped records must both occur)
def cases():
    c = []

    def add(cid, in1, args, in2=None, mixed=False):
        c.append({"id": cid, "in1": in1, "in2": in2, "args": args, "mixed": mixed})

    add("syn100_s0.25", "fastq/syn_100.fq.gz", ["-s", "0.25"], mixed=True)
    add("syn100_s7.25", "fastq/syn_100.fq.gz", ["-s", "7.25"], mixed=True)
    add("syn100_s3.999", "fastq/syn_100.fq.gz", ["-s", "3.999"])
    add("syn100_snone", "fastq/syn_100.fq.gz", ["-s", "0.00000001"])
    add("syn100_n1", "fastq/syn_100.fq.gz", ["-n", "1"], mixed=True)
    add("syn100_n1000", "fastq/syn_100.fq.gz", ["-n", "1000"], mixed=True)
    add("syn100_nall", "fastq/syn_100.fq.gz", ["-n", "4000"])
    add("syn100_nover", "fastq/syn_100.fq.gz", ["-n", "4001"])
    add("syn100_fasta", "fastq/syn_100.fq.gz", ["-f", "-s", "0.25"], mixed=True)
    add("syn100_both", "fastq/syn_100.fq.gz", ["-s", "7.25", "-n", "1000"], mixed=True)
    add("syn100_q_o", "fastq/syn_100.fq.gz", ["-f", "-q", "-o", "ignored", "-s", "7.5"], mixed=True)
    add("vara_s11.5", "fastq/syn_var_a.fq", ["-s", "11.5"], mixed=True)
    add("vara_n100", "fastq/syn_var_a.fq", ["-n", "100"], mixed=True)
    add("vara_fasta_n50", "fastq/syn_var_a.fq", ["-f", "-n", "50"], mixed=True)
    add("varb_s0.5785", "fastq/syn_var_b.fq.gz", ["-s", "0.5785"], mixed=True)
    add("varb_n77", "fastq/syn_var_b.fq.gz", ["-n", "77"], mixed=True)
    for f in ["multi.fq.gz", "t.fq", "t.fq.gz", "nonl.fq", "crlf.fq", "len0.fq", "short.fq", "allzero.fq", "stale.fq", "empty.fq"]:
        stem = f.replace(".", "_")
        add(stem + "_sall", "fastq/" + f, ["-s", "3.999"])
        add(stem + "_s5.5", "fastq/" + f, ["-s", "5.5"])
        add(stem + "_n1", "fastq/" + f, ["-n", "1"])
        add(stem + "_fasta_n1", "fastq/" + f, ["-f", "-n", "1"])
    add("t_fq_n5", "fastq/t.fq", ["-n", "5"])
    add("t_fq_n6", "fastq/t.fq", ["-n", "6"])
    add("nonl_fasta_sall", "fastq/nonl.fq", ["-f", "-s", "3.999"])
    add("long_s0.5", "sample/inputs/longnames.fq", ["-s", "0.5"], mixed=True)
    add("long_fasta_s9.3", "sample/inputs/longnames.fq", ["-f", "-s", "9.3"], mixed=True)
    add("long_n20", "sample/inputs/longnames.fq", ["-n", "20"], mixed=True)
    add("hibyte_s0.5", "sample/inputs/hibyte.fq", ["-s", "0.5"], mixed=True)
    add("hibyte_s77.4", "sample/inputs/hibyte.fq", ["-s", "77.4"], mixed=True)
    for m in ["equal", "short", "long"]:
        add("mate_%s_s0.5" % m, "sample/inputs/mate_a.fq", ["-s", "0.5"], in2="sample/inputs/mate_b_%s.fq" % m, mixed=True)
        add("mate_%s_n10" % m, "sample/inputs/mate_a.fq", ["-n", "10"], in2="sample/inputs/mate_b_%s.fq" % m, mixed=True)
    add("mate_equal_fasta_s4.5", "sample/inputs/mate_a.fq", ["-f", "-s", "4.5"], in2="sample/inputs/mate_b_equal.fq", mixed=True)
    add("mate_long_nover", "sample/inputs/mate_a.fq", ["-n", "61"], in2="sample/inputs/mate_b_long.fq")
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "inputs"))
    os.makedirs(os.path.join(OUT, "expected"))
    for name, data in own_inputs().items():
        with open(os.path.join(OUT, "inputs", name), "wb") as f:
            f.write(data)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            cmd = [exe, "-1", os.path.join(HERE, c["in1"])] + (["-2", os.path.join(HERE, c["in2"])] if c["in2"] else []) + c["args"]
            p = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0 and not p.stdout, (c["id"], p.returncode)
            entry = {"id": c["id"], "in1": c["in1"], "in2": c["in2"], "args": c["args"], "rc": p.returncode,
                     "stderr": TIMES.sub(b"at T s", p.stderr).decode(), "outputs": []}
            for fn in sorted(os.listdir(work)):
                raw = open(os.path.join(work, fn), "rb").read()
                text = gzip.decompress(raw) if raw else b""
                o = {"name": fn, "empty_file": not raw, "size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "data": None}
                if text and len(text) <= INLINE_LIMIT:
                    o["data"] = "expected/%s__%s.txt" % (c["id"], fn)
                    with open(os.path.join(OUT, o["data"]), "wb") as f:
                        f.write(text)
                entry["outputs"].append(o)
            if c["mixed"]:
                m = re.search(r"pick out: (\d+) \(\d+/(\d+)=", entry["stderr"])
                assert m and 0 < int(m.group(1)) < int(m.group(2)), (c["id"], entry["stderr"])
            manifest.append(entry)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    total = sum(os.path.getsize(os.path.join(dp, fn)) for dp, _, fs in os.walk(OUT) for fn in fs)
    print("%d cases, %d bytes under %s" % (len(manifest), total, OUT))


if __name__ == "__main__":
    main()
