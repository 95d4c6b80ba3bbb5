"""gzfastq_sort end to end on the README's 8e6 x 150 bp input: plain text and one gzip member, by sequence and by name.

The input is uniq_e2e's: bench_extra's synthetic text with the sequence of three reads in ten overwritten by the sequence of
another read (22 % of the records repeat an earlier sequence).  For every file: the wall of fastq_count (the floor: same
ingest, no sort), the walls of `gzfastq_sort -s` and `-n` with the tool's HPN_TIMING split (reading and framing / ordering
and formatting / writing) and the refinement's `rounds` and `refined`, and, where --ref names a compiled reference
gzfastq_sort, its wall on the plain file in the same session and whether the outputs are equal.  `--profile` adds one
rocprofv3 --kernel-trace --stats run of its own (no counters) on the plain file by sequence.

    python scripts/sort_e2e.py [--reads 8e6] [--ref PATH] [--profile] [--out profiles/sort/e2e.json]
"""
import argparse
import csv
import glob
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

from uniq_e2e import digest_dir, timed  # noqa: E402


def split_seconds(stderr):
    m = re.search(r"\[hpn\] sort: reading and framing ([\d.]+) s, ordering and formatting ([\d.]+) s, writing ([\d.]+) s; (\d+) rounds, (\d+) records refined", stderr)
    return {"read_frame_s": float(m.group(1)), "order_format_s": float(m.group(2)), "write_s": float(m.group(3)), "rounds": int(m.group(4)),
            "refined": int(m.group(5))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--ref", default=None, help="compiled reference gzfastq_sort (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort", "e2e.json"))
    a = ap.parse_args()
    n, L = int(a.reads), 150
    import numpy as np
    import torch  # noqa: F401
    import highperformancengs_amd as hp
    import bench_extra

    ctx = hp.Context(0)
    raw = bench_extra._fastq_text(ctx, n, L, 40)
    ctx.close()
    rec = raw.size // n
    rows = raw.reshape(n, rec)
    rs = np.random.RandomState(1)
    dst = rs.choice(n, int(a.dup * n), replace=False)
    rows[dst, 13:13 + L] = rows[rs.randint(0, n, dst.size), 13:13 + L]
    tmp = tempfile.mkdtemp(prefix="sort_e2e_")
    files = {"plain": os.path.join(tmp, "reads.fq"), "gzip1": os.path.join(tmp, "one.fq.gz")}
    open(files["plain"], "wb").write(rows.tobytes())
    open(files["gzip1"], "wb").write(bench_extra._gz_single_member(rows.tobytes(), 256, 16))
    del raw, rows
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "duplicated_fraction": a.dup, "reference_binary": bool(ref), "files": {}}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    for kind, path in files.items():
        r = {"bytes": os.path.getsize(path)}
        r["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path], work, reps=a.reps)
        for mode, flag in (("by_seq", "-s"), ("by_name", "-n")):
            walls, err = timed([os.path.join(BIN, "gzfastq_sort"), "-i", path, "-o", "o", flag], work, {"HPN_TIMING": "1"}, reps=a.reps)
            m = {"wall_s": walls, **split_seconds(err), "outputs": {k: v[0] for k, v in digest_dir(work).items()}}
            print(kind, mode, m, flush=True)
            if ref and kind == "plain":   # (the reference reads gzip through zlib on one core: its plain-text wall is its best case)
                ours = digest_dir(work)
                rw, _ = timed([ref, "-i", path, "-o", "o", flag], work)
                m["reference_wall_s"] = rw
                m["equals_reference"] = digest_dir(work) == ours
                print(kind, mode, "reference", rw, m["equals_reference"], flush=True)
            r[mode] = m
        result["files"][kind] = r
    if a.profile:
        d = os.path.join(tmp, "prof")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sort", "--", os.path.join(BIN, "gzfastq_sort"), "-i",
                        files["plain"], "-o", "o", "-s"], cwd=work, env={**os.environ, "HPN_FULL_EXIT": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        stats = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
        result["kernel_ms_plain_by_seq"] = stats
        result["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
