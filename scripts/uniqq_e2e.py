"""gzfastq_uniqQ end to end on the README's 8e6 x 150 bp input with 22 % of its reads duplicates (scripts/uniq_e2e.py's file).

The input is bench_extra's synthetic text with the sequence of three reads in ten overwritten by the sequence of another
read.  On that one plain file, in one session: the walls of `gzfastq_uniqQ -S` and `-C` (three runs each) with the tool's
HPN_TIMING split (reading and keying / grouping and ordering / formatting and writing), the wall of `gzfastq_uniq`
single-end as the floor (same ingest and grouping, two outputs of one record per key), and, where --ref names a compiled
reference gzfastq_uniqQ, its wall on the same file and whether the outputs are equal.  `--profile` adds one
rocprofv3 --kernel-trace --stats run of its own (no counters) per order and sets the new kernels' times against the bytes
they have to move.

    python scripts/uniqq_e2e.py [--reads 8e6] [--ref PATH] [--profile] [--out profiles/uniqq/e2e.json]
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
from uniq_e2e import BIN, HBM_PEAK, digest_dir, timed  # noqa: E402


def split_seconds(stderr):
    m = re.search(r"\[hpn\] uniqQ: reading and keying ([\d.]+) s, grouping and ordering ([\d.]+) s, formatting and writing ([\d.]+) s; (\d+) hash clashes, largest group (\d+)", stderr)
    u = re.search(r"unique reads number = (\d+)\((\d+) / (\d+) =", stderr)
    return {"read_key_s": float(m.group(1)), "group_order_s": float(m.group(2)), "format_write_s": float(m.group(3)), "hash_clashes": int(m.group(4)),
            "largest_group": int(m.group(5)), "unique": int(u.group(1)), "records": int(u.group(3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--ref", default=None, help="compiled reference gzfastq_uniqQ (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniqq", "e2e.json"))
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
    tmp = tempfile.mkdtemp(prefix="uniqq_e2e_")
    path = os.path.join(tmp, "reads_1.fq")
    open(path, "wb").write(rows.tobytes())
    del raw, rows
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "duplicated_fraction": a.dup, "reference_binary": bool(ref), "bytes": os.path.getsize(path)}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    result["gzfastq_uniq_single_wall_s"], _ = timed([os.path.join(BIN, "gzfastq_uniq"), "-1", path, "-o", "o"], work, reps=a.reps)
    for flag in ("-S", "-C"):
        walls, err = timed([os.path.join(BIN, "gzfastq_uniqQ"), "-1", path, flag, "-o", "o"], work, {"HPN_TIMING": "1"}, reps=a.reps)
        m = {"wall_s": walls, **split_seconds(err), "outputs": {k: v[0] for k, v in digest_dir(work).items()}}
        print(flag, m, flush=True)
        if ref:
            ours = digest_dir(work)
            rw, _ = timed([ref, "-1", path, flag, "-o", "o"], work)
            m["reference_wall_s"] = rw
            m["equals_reference"] = digest_dir(work) == ours
            print(flag, "reference", rw, m["equals_reference"], flush=True)
        result[flag] = m
    if a.profile:
        N, U = result["-S"]["records"], result["-S"]["unique"]
        out_bytes = sum(result["-S"]["outputs"].values())
        # the bytes each new kernel has to move (N records, U keys, Q = L + 1 bytes of quality line per record)
        must = {"k_uniqq_len": N * (4 + 4 + 4 + 32 + 4), "k_uniqq_sizes": U * (4 + 4 + 4 + 4 + 32 + 16 + 8), "k_uniqq_base": U * (4 + 4 + 4 + 4 + 32 + 8 + 8 + 8),
                "k_uniqq_count_key": U * (4 + 4 + 12), "k_uniqq_write": N * (4 + 8 + 32 + 8 + 8 + L + 1) + U * (rec - L - 1) + out_bytes}
        for flag in ("-S", "-C"):
            d = os.path.join(tmp, "prof" + flag)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "uniqq", "--", os.path.join(BIN, "gzfastq_uniqQ"),
                            "-1", path, flag, "-o", "o"], cwd=work, env={**os.environ, "HPN_FULL_EXIT": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            stats = {}
            for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(fn)):
                    stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
            model = {}
            for k, b in must.items():
                v = next((x for name, x in stats.items() if k in name), None)
                if v and v["total_ms"] > 0:
                    model[k] = {"calls": v["calls"], "ms": v["total_ms"], "bytes": int(b * v["calls"]),
                                "GBps": round(b * v["calls"] / (v["total_ms"] * 1e-3) / 1e9, 1),
                                "share_of_hbm_peak": round(b * v["calls"] / (v["total_ms"] * 1e-3) / HBM_PEAK, 4)}
            result[flag]["kernel_ms"] = stats
            result[flag]["kernel_model"] = model
            result[flag]["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
