"""gzfastq_uniq_sort end to end on the README's 8e6 x 150 bp input with 22 % of its reads duplicates (scripts/uniq_e2e.py's file).

The input is bench_extra's synthetic text with the sequence of three reads in ten overwritten by the sequence of another
read; the second mate is the same text with every read's sequence taken from another read and then overwritten alike, so a
duplicated pair is duplicated in both mates.  On those plain files, in one session: the walls of `gzfastq_uniq_sort`
single-end and paired (three runs each) with the tool's HPN_TIMING split (reading and keying / grouping and ordering /
formatting, deflating and writing), the walls of `gzfastq_uniq` on the same file(s) as the floor (same ingest and grouping,
plain-text outputs), and, where --ref names a compiled reference gzfastq_uniq_sort, its wall on the same files and whether
the outputs are equal after gunzip.  `--profile` adds one rocprofv3 --kernel-trace --stats run of its own (no counters) per
mode and sets the new kernels' times against the bytes they have to move.

    python scripts/usort_e2e.py [--reads 8e6] [--ref PATH] [--profile] [--out profiles/usort/e2e.json]
"""
import argparse
import csv
import glob
import gzip
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
from uniq_e2e import BIN, HBM_PEAK, timed  # noqa: E402


def gunzipped_digests(d):
    """{file name: (bytes after gunzip, sha256 of them)}: the compressed bytes are each tool's own."""
    out = {}
    for fn in sorted(os.listdir(d)):
        h, size = hashlib.sha256(), 0
        with gzip.open(os.path.join(d, fn), "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
                size += len(blk)
        out[fn] = (size, h.hexdigest())
    return out


def split_seconds(stderr):
    m = re.search(r"\[hpn\] uniq_sort: reading and keying ([\d.]+) s, grouping and ordering ([\d.]+) s, formatting, deflating and writing ([\d.]+) s "
                  r"\(([\d.]+) s of deflate over the threads\); (\d+) hash clashes, largest group (\d+)", stderr)
    u = re.search(r"unique reads number = (\d+)\n", stderr)
    t = re.search(r"total reads = (\d+)\n", stderr)
    return {"read_key_s": float(m.group(1)), "group_order_s": float(m.group(2)), "format_deflate_write_s": float(m.group(3)),
            "deflate_thread_s": float(m.group(4)), "hash_clashes": int(m.group(5)), "largest_group": int(m.group(6)), "unique": int(u.group(1)),
            "records": int(t.group(1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--ref", default=None, help="compiled reference gzfastq_uniq_sort (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usort", "e2e.json"))
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
    mate = rows.copy()
    mate[:, 13:13 + L] = rows[(np.arange(n) * 7 + 1) % n, 13:13 + L]
    rs = np.random.RandomState(1)
    dst = rs.choice(n, int(a.dup * n), replace=False)
    src = rs.randint(0, n, dst.size)
    rows[dst, 13:13 + L] = rows[src, 13:13 + L]
    mate[dst, 13:13 + L] = mate[src, 13:13 + L]
    tmp = tempfile.mkdtemp(prefix="usort_e2e_")
    paths = [os.path.join(tmp, "reads_1.fq"), os.path.join(tmp, "reads_2.fq")]
    open(paths[0], "wb").write(rows.tobytes())
    open(paths[1], "wb").write(mate.tobytes())
    del raw, rows, mate
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "duplicated_fraction": a.dup, "reference_binary": bool(ref), "bytes": os.path.getsize(paths[0])}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    for mode, files in (("single", ["-1", paths[0]]), ("paired", ["-1", paths[0], "-2", paths[1]])):
        floor, _ = timed([os.path.join(BIN, "gzfastq_uniq")] + files + ["-o", "o"], work, reps=a.reps)
        walls, err = timed([os.path.join(BIN, "gzfastq_uniq_sort")] + files + ["-o", "o"], work, {"HPN_TIMING": "1"}, reps=a.reps)
        ours = gunzipped_digests(work)
        m = {"wall_s": walls, "gzfastq_uniq_wall_s": floor, **split_seconds(err), "outputs": {k: v[0] for k, v in ours.items()}}
        print(mode, m, flush=True)
        if ref:
            rw, _ = timed([ref] + files + ["-o", "o"], work)
            m["reference_wall_s"] = rw
            m["equals_reference"] = gunzipped_digests(work) == ours
            print(mode, "reference", rw, m["equals_reference"], flush=True)
        result[mode] = m
    if a.profile:
        for mode, files, mates in (("single", ["-1", paths[0]], 1), ("paired", ["-1", paths[0], "-2", paths[1]], 2)):
            N, U = result[mode]["records"], result[mode]["unique"]
            out_bytes = sum(result[mode]["outputs"].values())
            # the bytes each new kernel has to move (N records, U keys, `mates` sequences of L bytes per key)
            must = {"k_usort_seqlen": N * 32, "k_usort_djb64": U * (4 + mates * (32 + L) + 8), "k_usort_bucket": U * (20 + mates * 32 + 12),
                    "k_usort_count_key": U * (4 + 4 + 8), "k_usort_sizes": mates * U * (4 + 4 + 4 + mates * 32 + 8),
                    "k_usort_write": mates * U * (4 + 4 + 4 + 8 + mates * 32) + 2 * out_bytes}
            d = os.path.join(tmp, "prof_" + mode)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "usort", "--", os.path.join(BIN, "gzfastq_uniq_sort")]
                           + files + ["-o", "o"], cwd=work, env={**os.environ, "HPN_FULL_EXIT": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            stats = {}
            for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(fn)):
                    stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
            model = {}
            for k, b in must.items():
                v = next((x for name, x in stats.items() if k in name), None)
                if v and v["total_ms"] > 0:
                    model[k] = {"calls": v["calls"], "ms": v["total_ms"], "bytes": int(b), "GBps": round(b / (v["total_ms"] * 1e-3) / 1e9, 1),
                                "share_of_hbm_peak": round(b / (v["total_ms"] * 1e-3) / HBM_PEAK, 4)}
            result[mode]["kernel_ms"] = stats
            result[mode]["kernel_model"] = model
            result[mode]["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
