"""bam_view end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x), with warm
files: three jobs -- SAM text to a file, `-b -F 0x400` to a file, `-c -f 2 -q 30` -- each three times on the device route and once
with HPN_BAM_GPU=0 (the sequential host route) in the same session, with the tool's HPN_TIMING stage split -- inflate + record
index / classify + store / scans + order / format or gather + scale + cuts + crc / copies to the host / fwrite or handing to the
writer: walls of synchronous calls, not kernel times -- the route it names, and whether the two routes' outputs are equal.  The
reference's `samtools view` is "not measured": the machine that runs this has no reference binary.

Every run of the tool is a step of its own under a time limit; a fault, an abort or a time limit ends the script there -- what was
measured up to then is written with "stopped" naming the step.

    python scripts/view_e2e.py [--reads 4e6] [--out profiles/view/e2e.json]
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
STEP_LIMIT_S = 240


class Stopped(Exception):
    pass


def step(name, cmd, cwd, env):
    """one run of the tool: (wall seconds, stderr, stdout); raises Stopped on a fault, an abort, a segmentation fault or the time limit"""
    for fn in os.listdir(cwd):
        os.remove(os.path.join(cwd, fn))
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise Stopped("%s: still running after %d s" % (name, STEP_LIMIT_S))
    wall = round(time.perf_counter() - t0, 3)
    err = p.stderr.decode("latin-1")
    if p.returncode in (134, 139, 124, 137, -6, -11, -9) or "illegal memory access" in err or "HSA_STATUS_ERROR" in err:
        raise Stopped("%s: status %d: %s" % (name, p.returncode, err[-500:]))
    if p.returncode != 0:
        raise Stopped("%s: status %d (no fault): %s" % (name, p.returncode, err[-500:]))
    return wall, err, p.stdout


def view_line(stderr):
    m = re.search(r"\[hpn\] bam_view: inflate \+ record index ([\d.]+) s, classify \+ store ([\d.]+) s, scans \+ order ([\d.]+) s, "
                  r"(?:format|gather \+ scale \+ cuts \+ crc) ([\d.]+) s, copies to the host ([\d.]+) s, (?:fwrite|handing to the writer) ([\d.]+) s; "
                  r"(\d+) batches, (\d+) records in, (\d+) kept, (\d+) text bytes, (\d+) blocks", stderr)
    out = {"route": "device" if "[hpn] bam_view: device route\n" in stderr else "host"}
    if m:
        names = ("inflate_index_s", "classify_store_s", "scans_order_s", "emit_s", "copies_s", "write_s")
        out.update({k: float(m.group(i + 1)) for i, k in enumerate(names)})
        out.update({"batches": int(m.group(7)), "records_in": int(m.group(8)), "kept": int(m.group(9)), "text_bytes": int(m.group(10)), "blocks": int(m.group(11))})
    return out


def sha(data):
    return hashlib.sha256(data).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="view_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    whole = os.path.join(tmp, "s.bam")
    subprocess.check_call([synth, whole, str(n), "2", str(n * 150 // 30 // 2), str(cores)])
    tool = os.path.join(BIN, "bam_view")
    result = {"reads": n, "read_length": 150, "input_bytes": os.path.getsize(whole), "contigs": 2, "reference": "not measured", "stopped": None, "jobs": {}}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    jobs = (("text", ["-o", "x.sam"], "x.sam"), ("bam_F0x400", ["-b", "-F", "0x400", "-o", "x.bam"], "x.bam"), ("count_f2_q30", ["-c", "-f", "2", "-q", "30"], None))
    try:
        for name, args, out in jobs:
            job = {}
            digests = {}
            for leg, env, reps in (("device", {"HPN_TIMING": "1"}, a.reps), ("host_route", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}, 1)):
                walls, err, stdout = [], "", b""
                for r in range(reps):
                    wall, err, stdout = step("%s %s run %d" % (name, leg, r), [tool] + args + [whole], work, env)
                    walls.append(wall)
                made = open(os.path.join(work, out), "rb").read() if out else stdout
                digests[leg] = sha(made)
                job[leg] = {"wall_s": walls, **view_line(err), "out_bytes": len(made)}
            job["device_equals_host_route"] = digests["device"] == digests["host_route"]
            result["jobs"][name] = job
    except Stopped as e:
        result["stopped"] = str(e)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(1 if result["stopped"] else 0)


if __name__ == "__main__":
    main()
