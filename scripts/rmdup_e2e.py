"""bam_rmdup end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x) with
duplicates added by this script: every record becomes the head of a proper pair (flag 0x63, isize 300, an RG tag of one of two
libraries) with its tail 150 bases further on, and every fifth pair is followed by a copy under another name and with lower
qualities (fixed seed for which).  Warm files.

The walls of the tool (three runs in one session) with its HPN_TIMING split -- inflate + record index / classify + store / groups +
names + placement / gather + cuts + crc / copies to the host / handing to the writer, and the writer's deflate time -- and the
route it names; one run with HPN_BAM_GPU=0 (the sequential host route), and whether the two routes' files are equal.  bam_sort's
wall on the same file in the same session is the yardstick: both inflate, gather and deflate about the same bytes.  The
reference's `samtools rmdup` is "not measured": the machine that runs this has no reference binary.  --profile adds ONE
rocprofv3 --kernel-trace --stats run of its own (no counters, the tool behind `--`).

    python scripts/rmdup_e2e.py [--reads 4e6] [--profile] [--out profiles/rmdup/e2e.json]
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
RG = "@RG\tID:one\tLB:libOne\n@RG\tID:two\tLB:libTwo\n"


def rmdup_line(stderr):
    m = re.search(r"\[hpn\] bam_rmdup: inflate \+ record index ([\d.]+) s, classify \+ store ([\d.]+) s, groups \+ names \+ placement ([\d.]+) s, "
                  r"gather \+ cuts \+ crc ([\d.]+) s, copies to the host ([\d.]+) s, handing to the writer ([\d.]+) s; (\d+) batches, (\d+) records in, "
                  r"(\d+) heads, (\d+) records out, (\d+) blocks; writer: ([\d.]+) s deflating \(all threads\), ([\d.]+) s waited for", stderr)
    out = {"route": "device" if "[hpn] bam_rmdup: device route\n" in stderr else "host"}
    if m:
        names = ("inflate_index_s", "classify_store_s", "decide_s", "gather_cuts_crc_s", "copies_s", "handing_s")
        out.update({k: float(m.group(i + 1)) for i, k in enumerate(names)})
        out.update({"batches": int(m.group(7)), "records_in": int(m.group(8)), "heads": int(m.group(9)), "records_out": int(m.group(10)),
                    "blocks": int(m.group(11)), "deflate_cpu_s": float(m.group(12)), "writer_waited_s": float(m.group(13))})
    return out


def inflate(path):
    data, parts, o = open(path, "rb").read(), [], 0
    while o < len(data):
        xlen, bsize = struct.unpack_from("<H", data, o + 10)[0], struct.unpack_from("<H", data, o + 16)[0] + 1
        parts.append(zlib.decompress(data[o + 12 + xlen:o + bsize - 8], -15))
        o += bsize
    return b"".join(parts)


def with_duplicates(raw, seed=1):
    """the inflated stream of a sorted BAM -> (the stream of the file described above, its record count)"""
    l_text, = struct.unpack_from("<i", raw, 4)
    n_ref, = struct.unpack_from("<i", raw, 8 + l_text)
    at = 12 + l_text
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    text = raw[8:8 + l_text] + RG.encode()
    head = raw[:4] + struct.pack("<i", len(text)) + text + raw[8 + l_text:at]
    rs = np.random.RandomState(seed)
    recs, keys = [], []

    def put(tid, pos, body):
        recs.append(struct.pack("<i", len(body)) + body)
        keys.append((tid << 32) | pos)

    k = 0
    while at < len(raw):
        size, = struct.unpack_from("<i", raw, at)
        tid, pos, bmn, fnc, l_seq = struct.unpack_from("<iiIIi", raw, at + 4)
        l_name, n_cig = bmn & 0xff, fnc & 0xffff
        name = raw[at + 36:at + 36 + l_name - 1]
        rest = raw[at + 36 + l_name:at + 4 + size]                      # CIGAR, bases, qualities, aux
        q0 = 4 * n_cig + (l_seq + 1) // 2
        aux = b"RGZ" + (b"one" if k & 1 else b"two") + b"\0"
        for copy in range(2 if rs.randint(0, 5) == 0 else 1):
            nm = name + (b"/dup" if copy else b"") + b"\0"
            qual = bytes(max(0, c - 1) for c in rest[q0:q0 + l_seq]) if copy else rest[q0:q0 + l_seq]
            tail_of = rest[:q0] + qual + rest[q0 + l_seq:] + aux
            fixed = lambda p, flag, mpos, isize: struct.pack("<iiIIiiii", tid, p, (bmn & ~0xff) | len(nm), (flag << 16) | n_cig, l_seq, tid, mpos, isize)
            put(tid, pos, fixed(pos, 0x63, pos + 150, 300) + nm + tail_of)
            put(tid, pos + 150, fixed(pos + 150, 0x93, pos, -300) + nm + tail_of)
        at += 4 + size
        k += 1
    order = np.argsort(np.array(keys, np.int64), kind="stable")
    return head + b"".join(recs[i] for i in order), len(recs)


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    from twobit_e2e import kernel_stats
    from uniq_e2e import timed
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmdup", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="rmdup_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    plain, bam = os.path.join(tmp, "s.bam"), os.path.join(tmp, "dups.bam")
    subprocess.check_call([synth, plain, str(n // 2), "2", str(n * 150 // 30 // 2), str(cores)])      # (every record becomes a pair)
    stream, records = with_duplicates(inflate(plain))
    with open(bam + ".raw", "wb") as f:
        f.write(stream)
    subprocess.check_call([synth, "--bgzip", bam + ".raw", bam, str(cores)])
    os.remove(bam + ".raw")
    tool = os.path.join(BIN, "bam_rmdup")
    result = {"reads": n, "records": records, "read_length": 150, "bam_bytes": os.path.getsize(bam), "contigs": 2, "reference": "not measured"}
    dirs = {k: os.path.join(tmp, k) for k in ("dev", "host", "sort", "prof")}      # (timed() empties its directory before every run)
    for d in dirs.values():
        os.makedirs(d)
    walls, err = timed([tool, bam, os.path.join(dirs["dev"], "x.bam")], dirs["dev"], {"HPN_TIMING": "1"}, reps=a.reps)
    result["device"] = {"wall_s": walls, **rmdup_line(err), "out_bytes": os.path.getsize(os.path.join(dirs["dev"], "x.bam"))}
    walls, err = timed([tool, bam, os.path.join(dirs["host"], "x.bam")], dirs["host"], {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}, reps=1)
    result["host_route"] = {"wall_s": walls, **rmdup_line(err)}
    result["device_equals_host_route"] = sha(os.path.join(dirs["dev"], "x.bam")) == sha(os.path.join(dirs["host"], "x.bam"))
    walls, err = timed([os.path.join(BIN, "bam_sort"), bam, os.path.join(dirs["sort"], "x")], dirs["sort"], {"HPN_TIMING": "1"}, reps=a.reps)
    result["bam_sort_same_file"] = {"wall_s": walls, "route": "device" if "[hpn] bam_sort: device route\n" in err else "host"}
    if a.profile:
        stats = kernel_stats([tool, bam, os.path.join(dirs["prof"], "x.bam")], dirs["prof"], os.path.join(tmp, "rocprof"), "rmdup")
        result["kernel_ms"] = stats
        result["rmdup_kernel_ms"] = round(sum(v["total_ms"] for k, v in stats.items() if "k_rm_" in k), 3)
        result["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
