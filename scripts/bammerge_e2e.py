"""bam_merge end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x) dealt
into four coordinate-sorted quarters by this script (record k goes to quarter k mod 4, so every quarter spans both contigs and
the merge interleaves them everywhere), with warm files.

The walls of the tool at the default level and with -u (three runs each in one session) with its HPN_TIMING split -- inflate +
record index / keys + store / running maximum + sort + offsets / gather + cuts + crc / copies to the host / handing to the
writer, and the writer's deflate time -- and the route it names; the same at the default level with HPN_BAM_GPU=0 (the sequential
host route), and whether the two routes' files are equal.  (-u changes no byte in samtools-0.1.19's merge, nor here:
docs/kernels/bam_merge.md; the leg is kept to show that.)  The reference's `samtools merge` is "not measured": the machine that
runs this has no reference binary.

Every run of the tool is a step of its own under a time limit; a fault, an abort or a time limit ends the script there -- what was
measured up to then is written with "stopped" naming the step.

    python scripts/bammerge_e2e.py [--reads 4e6] [--out profiles/bammerge/e2e.json]
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
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
STEP_LIMIT_S = 240


class Stopped(Exception):
    pass


def step(name, cmd, cwd, env):
    """one run of the tool: (wall seconds, stderr); raises Stopped on a fault, an abort, a segmentation fault or the time limit"""
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
    return wall, err


def merge_line(stderr):
    m = re.search(r"\[hpn\] bam_merge: inflate \+ record index ([\d.]+) s, keys \+ store ([\d.]+) s, running maximum \+ sort \+ offsets ([\d.]+) s, "
                  r"gather \+ cuts \+ crc ([\d.]+) s, copies to the host ([\d.]+) s, handing to the writer ([\d.]+) s; (\d+) files, (\d+) batches, (\d+) records, "
                  r"(\d+) lifted, (\d+) key bits, (\d+) blocks; writer: ([\d.]+) s deflating \(all threads\), ([\d.]+) s waited for", stderr)
    out = {"route": "device" if "[hpn] bam_merge: device route\n" in stderr else "host"}
    if m:
        names = ("inflate_index_s", "keys_store_s", "runmax_sort_offsets_s", "gather_cuts_crc_s", "copies_s", "handing_s")
        out.update({k: float(m.group(i + 1)) for i, k in enumerate(names)})
        out.update({"files": int(m.group(7)), "batches": int(m.group(8)), "records": int(m.group(9)), "lifted": int(m.group(10)), "key_bits": int(m.group(11)),
                    "blocks": int(m.group(12)), "deflate_cpu_s": float(m.group(13)), "writer_waited_s": float(m.group(14))})
    return out


def deal_bam(src, dsts, synth, cores):
    """record k of the coordinate-sorted `src` -> dsts[k mod len(dsts)] (the header kept), compressed by bam_synth --bgzip"""
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
    head = raw[:at]
    outs = [open(d + ".raw", "wb") for d in dsts]
    for f in outs:
        f.write(head)
    k = 0
    while at < len(raw):
        end = at + 4 + struct.unpack_from("<i", raw, at)[0]
        outs[k % len(outs)].write(raw[at:end])
        at, k = end, k + 1
    for f, d in zip(outs, dsts):
        f.close()
        subprocess.check_call([synth, "--bgzip", d + ".raw", d, str(cores)])
        os.remove(d + ".raw")
    return k


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bammerge", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="bammerge_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    whole = os.path.join(tmp, "s.bam")
    subprocess.check_call([synth, whole, str(n), "2", str(n * 150 // 30 // 2), str(cores)])
    quarters = [os.path.join(tmp, "q%d.bam" % k) for k in range(4)]
    records = deal_bam(whole, quarters, synth, cores)
    tool = os.path.join(BIN, "bam_merge")
    result = {"reads": n, "records": records, "read_length": 150, "inputs": 4, "input_bytes": sum(os.path.getsize(q) for q in quarters), "contigs": 2,
              "reference": "not measured", "stopped": None}
    dirs = {k: os.path.join(tmp, k) for k in ("dev", "dev_u", "host")}      # (step() empties its directory before every run)
    for d in dirs.values():
        os.makedirs(d)
    try:
        for leg, opts, env, reps in (("device", [], {"HPN_TIMING": "1"}, a.reps), ("device_u", ["-u"], {"HPN_TIMING": "1"}, a.reps),
                                     ("host_route", [], {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}, 1)):
            d = dirs["host" if leg == "host_route" else "dev" if leg == "device" else "dev_u"]
            walls, err = [], ""
            for r in range(reps):
                wall, err = step("%s run %d" % (leg, r), [tool] + opts + [os.path.join(d, "x.bam")] + quarters, d, env)
                walls.append(wall)
            result[leg] = {"wall_s": walls, **merge_line(err), "out_bytes": os.path.getsize(os.path.join(d, "x.bam"))}
        result["device_equals_host_route"] = sha(os.path.join(dirs["dev"], "x.bam")) == sha(os.path.join(dirs["host"], "x.bam"))
        result["u_changes_no_byte"] = sha(os.path.join(dirs["dev"], "x.bam")) == sha(os.path.join(dirs["dev_u"], "x.bam"))
    except Stopped as e:
        result["stopped"] = str(e)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(1 if result["stopped"] else 0)


if __name__ == "__main__":
    main()
