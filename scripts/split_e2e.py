"""bamSplitChr end to end on the 4e6 x 150 bp BAM of bench.py's end-to-end legs (scripts/bam_synth.cpp: two contigs at 30x), at the
default level and at `-u x`, with warm files.

For each level: the walls of the tool (three runs in one session) with its HPN_TIMING split -- inflate + index / keys, cuts, CRC and
framing / copies to the host / handing blocks to the writer, and the writer's deflate seconds and what the main thread waited for
it --, and, where --ref names the compiled reference (bamSplitChr.c against libbam, as tests/golden/make_golden_split.py builds it),
its wall in the same session and whether every output file is byte-equal; where the zlib differs the files are compared block by
block instead (ISIZE sequence, CRC-32 fields against the inflated bytes, inflated bytes) and the result says which comparison was made.  `--profile` adds
ONE rocprofv3 --kernel-trace --stats run of its own (no counters) at `-u x`: the split kernels' totals, their algorithmic bytes as
a share of the HBM peak, and the runtime's device-to-device copy kernels of the same run beside k_split_stored.

    python scripts/split_e2e.py [--reads 4e6] [--ref PATH] [--profile] [--out profiles/split/e2e.json]
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")

from twobit_e2e import kernel_stats  # noqa: E402
from uniq_e2e import HBM_PEAK, digest_dir, timed  # noqa: E402


def split_line(stderr):
    m = re.search(r"\[hpn\] split: inflate \+ index ([\d.]+) s, keys \+ cuts \+ crc \+ framing ([\d.]+) s, copies to the host ([\d.]+) s, "
                  r"handing to the writer ([\d.]+) s; (\d+) batches, (\d+) blocks, (\d+) bytes copied", stderr)
    w = re.search(r"\[hpn\] writer: ([\d.]+) s deflating \(all threads\), ([\d.]+) s the main thread waited", stderr)
    z = re.search(r"\[hpn\] zlib (\S+)", stderr)
    out = {"on_device": bool(m) and "abandoned" not in stderr, "zlib": z.group(1) if z else None}
    if m:
        out.update({"inflate_index_s": float(m.group(1)), "split_s": float(m.group(2)), "copy_s": float(m.group(3)), "hand_s": float(m.group(4)),
                    "batches": int(m.group(5)), "blocks": int(m.group(6)), "bytes_copied": int(m.group(7))})
    if w:
        out.update({"writer_deflate_s_all_threads": float(w.group(1)), "writer_waited_s": float(w.group(2))})
    return out


def same_payload(a, b):
    import split_ref
    da, db = split_ref.describe(open(a, "rb").read()), split_ref.describe(open(b, "rb").read())
    return da["isize"] == db["isize"] and da["inflated_sha256"] == db["inflated_sha256"]      # (describe() checks every CRC-32 against its bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=4e6)
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "bamSplitChr"), help="compiled reference (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split", "e2e.json"))
    a = ap.parse_args()
    n = int(a.reads)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 16
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", "16")))
    tmp = tempfile.mkdtemp(prefix="split_e2e_")
    synth = os.path.join(tmp, "bam_synth")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "bam_synth.cpp"), "-o", synth, "-lz", "-lpthread"])
    contig = n * 150 // 30 // 2
    bam = os.path.join(tmp, "s.bam")
    subprocess.check_call([synth, bam, str(n), "2", str(contig), str(cores)])
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    tool = os.path.join(BIN, "bamSplitChr")
    result = {"reads": n, "read_length": 150, "bam_bytes": os.path.getsize(bam), "contigs": 2, "reference_binary": bool(ref), "levels": {}}
    work, keep = os.path.join(tmp, "work"), os.path.join(tmp, "ours")
    os.makedirs(work)
    for name, opt in (("default", []), ("uncompressed", ["-u", "x"])):
        walls, err = timed([tool] + opt + ["-o", os.path.join(work, "o"), bam], work, {"HPN_TIMING": "1"}, reps=a.reps)
        ours = digest_dir(work)
        r = {"wall_s": walls, **split_line(err), "outputs": {k: v[0] for k, v in ours.items()}}
        if ref:
            shutil.rmtree(keep, ignore_errors=True)
            shutil.copytree(work, keep)
            rw, _ = timed([ref] + opt + ["-o", os.path.join(work, "o"), bam], work)
            theirs = digest_dir(work)
            r["reference_wall_s"] = rw
            r["byte_equal"] = theirs == ours
            if not r["byte_equal"]:
                r["payload_equal"] = sorted(theirs) == sorted(ours) and all(same_payload(os.path.join(keep, f), os.path.join(work, f)) for f in ours)
        print(name, r, flush=True)
        result["levels"][name] = r
    if a.profile:
        stats = kernel_stats([tool, "-u", "x", "-o", os.path.join(work, "o"), bam], work, os.path.join(tmp, "prof"), "split")
        result["kernel_ms_uncompressed"] = stats
        u = result["levels"]["uncompressed"]
        N, payload, blocks = n, u.get("bytes_copied", 0), u.get("blocks", 0)
        rounds = 23
        # algorithmic bytes (docs/kernels/bam_split.md): keys: 12 bytes of each record and of its neighbour, an offset read, Q and key
        # written; next: Q and key read (the searches stay in cache), next and mark written; one doubling round: jump read twice, mark,
        # jump written; stored: every payload byte read and written + 31 bytes of framing a block
        must = {"k_split_keys": N * (24 + 8 + 8 + 4), "k_split_next": N * (8 + 4 + 4 + 4), "k_split_double": N * 16 * rounds,
                "k_split_stored": 2 * payload - 31 * blocks}
        model = {}
        for k, b in must.items():
            v = next((x for nm, x in stats.items() if k in nm), None)
            if v and v["total_ms"] > 0:
                model[k] = {"calls": v["calls"], "ms": v["total_ms"], "bytes": int(b), "GBps": round(b / (v["total_ms"] * 1e-3) / 1e9, 1),
                            "share_of_hbm_peak": round(b / (v["total_ms"] * 1e-3) / HBM_PEAK, 4)}
        result["kernel_model_uncompressed"] = model
        result["device_copy_kernels_same_run"] = {k: v for k, v in stats.items() if "copy" in k.lower()}
        result["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
