"""bam_fixmate end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x) turned
into aligner output by this script: records 2k and 2k + 1 become a pair -- one name, flags 0x41 and 0x91, the mate fields unfilled
(-1, -1, 0) -- so the file is name-adjacent and every pair gets its CT field; with warm files.

The walls of the tool at the default level (three runs in one session) with its HPN_TIMING split -- inflate + record index /
classify + store / names + roles + order + patches / gather + patch + cuts + crc / copies to the host / handing to the writer, and
the writer's deflate time -- and the route it names; the same with HPN_BAM_GPU=0 (the sequential host route) in the same session,
and whether the two routes' files are equal.  The reference's `samtools fixmate` is "not measured": the machine that runs this has
no reference binary.

Every run of the tool is a step of its own under a time limit; a fault, an abort or a time limit ends the script there -- what was
measured up to then is written with "stopped" naming the step.

    python scripts/fixmate_e2e.py [--reads 4e6] [--out profiles/fixmate/e2e.json]
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


def fixmate_line(stderr):
    m = re.search(r"\[hpn\] bam_fixmate: inflate \+ record index ([\d.]+) s, classify \+ store ([\d.]+) s, names \+ roles \+ order \+ patches ([\d.]+) s, "
                  r"gather \+ patch \+ cuts \+ crc ([\d.]+) s, copies to the host ([\d.]+) s, handing to the writer ([\d.]+) s; (\d+) batches, (\d+) records in, "
                  r"(\d+) out, (\d+) pairs, (\d+) singletons, (\d+) CT fields \((\d+) bytes\), (\d+) blocks; writer: ([\d.]+) s deflating \(all threads\), "
                  r"([\d.]+) s waited for", stderr)
    out = {"route": "device" if "[hpn] bam_fixmate: device route\n" in stderr else "host"}
    if m:
        names = ("inflate_index_s", "classify_store_s", "names_roles_order_patches_s", "gather_patch_cuts_crc_s", "copies_s", "handing_s")
        out.update({k: float(m.group(i + 1)) for i, k in enumerate(names)})
        out.update({"batches": int(m.group(7)), "records_in": int(m.group(8)), "records_out": int(m.group(9)), "pairs": int(m.group(10)),
                    "singletons": int(m.group(11)), "ct_fields": int(m.group(12)), "ct_bytes": int(m.group(13)), "blocks": int(m.group(14)),
                    "deflate_cpu_s": float(m.group(15)), "writer_waited_s": float(m.group(16))})
    return out


def pair_up(src, dst, synth, cores):
    """records 2k and 2k + 1 of `src` -> a name-adjacent pair with unfilled mate fields in `dst` (the header kept), compressed by
    bam_synth --bgzip; returns the number of records"""
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
    unfilled = struct.pack("<iii", -1, -1, 0)
    k, name = 0, b""
    with open(dst + ".raw", "wb") as f:
        f.write(raw[:at])
        while at < len(raw):
            end = at + 4 + struct.unpack_from("<i", raw, at)[0]
            l_qname, n_cigar = raw[at + 12], struct.unpack_from("<H", raw, at + 16)[0]
            if k % 2 == 0:
                name = raw[at + 36:at + 36 + l_qname]
            body = (raw[at + 4:at + 12] + bytes([len(name)]) + raw[at + 13:at + 16] + struct.pack("<HH", n_cigar, 0x41 if k % 2 == 0 else 0x91) +
                    raw[at + 20:at + 24] + unfilled + name + raw[at + 36 + l_qname:end])
            f.write(struct.pack("<i", len(body)) + body)
            at, k = end, k + 1
    subprocess.check_call([synth, "--bgzip", dst + ".raw", dst, str(cores)])
    os.remove(dst + ".raw")
    return k


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixmate", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="fixmate_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    whole = os.path.join(tmp, "s.bam")
    subprocess.check_call([synth, whole, str(n), "2", str(n * 150 // 30 // 2), str(cores)])
    aligned = os.path.join(tmp, "aligned.bam")
    records = pair_up(whole, aligned, synth, cores)
    os.remove(whole)
    tool = os.path.join(BIN, "bam_fixmate")
    result = {"reads": n, "records": records, "read_length": 150, "input_bytes": os.path.getsize(aligned), "contigs": 2, "reference": "not measured",
              "stopped": None}
    dirs = {k: os.path.join(tmp, k) for k in ("dev", "host")}      # (step() empties its directory before every run)
    for d in dirs.values():
        os.makedirs(d)
    try:
        for leg, env, reps in (("device", {"HPN_TIMING": "1"}, a.reps), ("host_route", {"HPN_TIMING": "1", "HPN_BAM_GPU": "0"}, 1)):
            d = dirs["host" if leg == "host_route" else "dev"]
            walls, err = [], ""
            for r in range(reps):
                wall, err = step("%s run %d" % (leg, r), [tool, aligned, os.path.join(d, "x.bam")], d, env)
                walls.append(wall)
            result[leg] = {"wall_s": walls, **fixmate_line(err), "out_bytes": os.path.getsize(os.path.join(d, "x.bam"))}
        result["device_equals_host_route"] = sha(os.path.join(dirs["dev"], "x.bam")) == sha(os.path.join(dirs["host"], "x.bam"))
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
