"""bam_index end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x), with
warm files.

The walls of the tool (three runs in one session) with its HPN_TIMING split -- inflate + record index / per-record pass + run
heads / lists + linear index -- and the route it names; the same three runs with HPN_BAM_GPU=0 (the sequential host route);
yardstick 1, `bam2depth -w 1000` of this build on the same file in the same session, reading it through the index the tool
just wrote (docs/kernels/bam_bai.md: the indexer reads the same bytes and writes far less, so it should not be slower);
yardstick 2, with --ref PATH, a compiled `samtools index` of samtools-0.1.19 (libbam + a driver that calls bam_index(argc, argv),
as tests/golden/make_golden_bai.py builds it) with its index compared byte for byte -- without it the result says "not
measured".  Whether the device route's index equals the host route's is recorded in any case.  --profile adds ONE rocprofv3
--kernel-trace --stats run of its own (no counters): the bai kernels' totals beside the ingest's.

    python scripts/bai_e2e.py [--reads 4e6] [--ref PATH] [--profile] [--out profiles/bai/e2e.json]
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")

from twobit_e2e import kernel_stats  # noqa: E402
from uniq_e2e import timed  # noqa: E402


def bai_line(stderr):
    m = re.search(r"\[hpn\] bam_index: inflate \+ record index ([\d.]+) s, per-record pass \+ run heads ([\d.]+) s, lists \+ linear index ([\d.]+) s; "
                  r"(\d+) batches, (\d+) records, (\d+) runs, (\d+) chunks", stderr)
    out = {"route": "device" if "[hpn] bam_index: device route\n" in stderr else "host"}
    if m:
        out.update({"inflate_index_s": float(m.group(1)), "records_pass_s": float(m.group(2)), "lists_s": float(m.group(3)), "batches": int(m.group(4)),
                    "records": int(m.group(5)), "runs": int(m.group(6)), "chunks": int(m.group(7))})
    return out


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--ref", default=None, help="a compiled `samtools index` of samtools-0.1.19 (absent: not measured)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bai", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="bai_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    bam = os.path.join(tmp, "s.bam")
    subprocess.check_call([synth, bam, str(n), "2", str(n * 150 // 30 // 2), str(cores)])
    if os.path.exists(bam + ".bai"):
        os.remove(bam + ".bai")            # (the generator's own index: not samtools')
    tool = os.path.join(BIN, "bam_index")
    result = {"reads": n, "read_length": 150, "bam_bytes": os.path.getsize(bam), "contigs": 2}
    dirs = {k: os.path.join(tmp, k) for k in ("dev", "host", "ref", "depth", "prof")}      # (timed() empties its directory before every run)
    for d in dirs.values():
        os.makedirs(d)
    walls, err = timed([tool, bam, os.path.join(dirs["dev"], "x.bai")], dirs["dev"], {"HPN_TIMING": "1"}, reps=a.reps)
    result["device"] = {"wall_s": walls, **bai_line(err), "index_bytes": os.path.getsize(os.path.join(dirs["dev"], "x.bai"))}
    walls, err = timed([tool, bam, os.path.join(dirs["host"], "x.bai")], dirs["host"], {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}, reps=a.reps)
    result["host_route"] = {"wall_s": walls, **bai_line(err)}
    result["device_equals_host_route"] = sha(os.path.join(dirs["dev"], "x.bai")) == sha(os.path.join(dirs["host"], "x.bai"))
    shutil.copyfile(os.path.join(dirs["dev"], "x.bai"), bam + ".bai")
    walls, _ = timed([os.path.join(BIN, "bam2depth"), "-w", "1000", "-o", os.path.join(dirs["depth"], "d"), bam], dirs["depth"], reps=a.reps)
    result["bam2depth_same_file_wall_s"] = walls
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    if ref:
        walls, _ = timed([ref, bam, os.path.join(dirs["ref"], "x.bai")], dirs["ref"], reps=a.reps)
        result["reference"] = {"wall_s": walls, "byte_equal": sha(os.path.join(dirs["ref"], "x.bai")) == sha(os.path.join(dirs["dev"], "x.bai"))}
    else:
        result["reference"] = "not measured"
    if a.profile:
        stats = kernel_stats([tool, bam, os.path.join(dirs["prof"], "x.bai")], dirs["prof"], os.path.join(tmp, "rocprof"), "bai")
        result["kernel_ms"] = stats
        result["bai_kernel_ms"] = round(sum(v["total_ms"] for k, v in stats.items() if "k_bai_" in k), 3)
        result["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
