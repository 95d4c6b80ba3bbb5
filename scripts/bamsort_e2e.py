"""bam_sort end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x) with its
records shuffled by this script (fixed seed; the header's SO set to unsorted), with warm files.

The walls of the tool at the default level and at -l 0 (three runs each in one session) with its HPN_TIMING split -- inflate +
record index / keys + store / sort + offsets / gather + cuts + crc / copies to the host / handing to the writer, and the writer's
deflate time -- and the route it names; the same at the default level with HPN_BAM_GPU=0 (the sequential host route), and whether
the two routes' files are equal.  The reference's `samtools sort` is "not measured": the machine that runs this has no reference
binary.  --profile adds ONE rocprofv3 --kernel-trace --stats run of its own (no counters, the tool behind `--`): the sort
kernels' totals beside the ingest's.

    python scripts/bamsort_e2e.py [--reads 4e6] [--profile] [--out profiles/bamsort/e2e.json]
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

from twobit_e2e import kernel_stats  # noqa: E402
from uniq_e2e import timed  # noqa: E402


def sort_line(stderr):
    m = re.search(r"\[hpn\] bam_sort: inflate \+ record index ([\d.]+) s, keys \+ store ([\d.]+) s, sort \+ offsets ([\d.]+) s, gather \+ cuts \+ crc ([\d.]+) s, "
                  r"copies to the host ([\d.]+) s, handing to the writer ([\d.]+) s; (\d+) batches, (\d+) records, (\d+) key bits, (\d+) blocks; "
                  r"writer: ([\d.]+) s deflating \(all threads\), ([\d.]+) s waited for", stderr)
    out = {"route": "device" if "[hpn] bam_sort: device route\n" in stderr else "host"}
    if m:
        names = ("inflate_index_s", "keys_store_s", "sort_offsets_s", "gather_cuts_crc_s", "copies_s", "handing_s")
        out.update({k: float(m.group(i + 1)) for i, k in enumerate(names)})
        out.update({"batches": int(m.group(7)), "records": int(m.group(8)), "key_bits": int(m.group(9)), "blocks": int(m.group(10)),
                    "deflate_cpu_s": float(m.group(11)), "writer_waited_s": float(m.group(12))})
    return out


def shuffle_bam(src, dst, synth, cores, seed=1):
    """the records of `src` in a random order (the header kept, SO:unsorted) -> `dst`, compressed by bam_synth --bgzip"""
    data = open(src, "rb").read()
    parts, o = [], 0
    while o < len(data):
        xlen, bsize = struct.unpack_from("<H", data, o + 10)[0], struct.unpack_from("<H", data, o + 16)[0] + 1
        parts.append(zlib.decompress(data[o + 12 + xlen:o + bsize - 8], -15))
        o += bsize
    raw = b"".join(parts)
    l_text, = struct.unpack_from("<i", raw, 4)
    n_ref, = struct.unpack_from("<i", raw, 8 + l_text)
    at = 12 + l_text
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    text = raw[8:8 + l_text].replace(b"SO:coordinate", b"SO:unsorted")
    head = raw[:4] + struct.pack("<i", len(text)) + text + raw[8 + l_text:at]
    offs = []
    while at < len(raw):
        offs.append(at)
        at += 4 + struct.unpack_from("<i", raw, at)[0]
    offs.append(at)
    order = np.random.RandomState(seed).permutation(len(offs) - 1)
    with open(dst + ".raw", "wb") as f:
        f.write(head)
        for i in order:
            f.write(raw[offs[i]:offs[i + 1]])
    subprocess.check_call([synth, "--bgzip", dst + ".raw", dst, str(cores)])
    os.remove(dst + ".raw")
    return len(offs) - 1


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bamsort", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="bamsort_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    sorted_bam, bam = os.path.join(tmp, "s.bam"), os.path.join(tmp, "shuffled.bam")
    subprocess.check_call([synth, sorted_bam, str(n), "2", str(n * 150 // 30 // 2), str(cores)])
    records = shuffle_bam(sorted_bam, bam, synth, cores)
    tool = os.path.join(BIN, "bam_sort")
    result = {"reads": n, "records": records, "read_length": 150, "bam_bytes": os.path.getsize(bam), "contigs": 2, "reference": "not measured"}
    dirs = {k: os.path.join(tmp, k) for k in ("dev", "dev0", "host", "prof")}      # (timed() empties its directory before every run)
    for d in dirs.values():
        os.makedirs(d)
    walls, err = timed([tool, bam, os.path.join(dirs["dev"], "x")], dirs["dev"], {"HPN_TIMING": "1"}, reps=a.reps)
    result["device"] = {"wall_s": walls, **sort_line(err), "out_bytes": os.path.getsize(os.path.join(dirs["dev"], "x.bam"))}
    walls, err = timed([tool, "-l", "0", bam, os.path.join(dirs["dev0"], "x")], dirs["dev0"], {"HPN_TIMING": "1"}, reps=a.reps)
    result["device_l0"] = {"wall_s": walls, **sort_line(err), "out_bytes": os.path.getsize(os.path.join(dirs["dev0"], "x.bam"))}
    walls, err = timed([tool, bam, os.path.join(dirs["host"], "x")], dirs["host"], {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}, reps=1)
    result["host_route"] = {"wall_s": walls, **sort_line(err)}
    result["device_equals_host_route"] = sha(os.path.join(dirs["dev"], "x.bam")) == sha(os.path.join(dirs["host"], "x.bam"))
    if a.profile:
        stats = kernel_stats([tool, bam, os.path.join(dirs["prof"], "x")], dirs["prof"], os.path.join(tmp, "rocprof"), "bamsort")
        result["kernel_ms"] = stats
        result["sort_kernel_ms"] = round(sum(v["total_ms"] for k, v in stats.items() if "k_sort_" in k), 3)
        result["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
