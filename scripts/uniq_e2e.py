"""gzfastq_uniq end to end on the README's 8e6 x 150 bp input with about 30 % duplicates: plain text and one gzip member,
single-end and as pairs.

The input is bench_extra's synthetic text with the sequence of three reads in ten overwritten by the sequence of another
read (the mate file: the same reads reversed, so a pair repeats exactly when its first mate does).  For every file: the
wall of fastq_count (the floor: same ingest, no dedup), the walls of `gzfastq_uniq` with the tool's HPN_TIMING split
(reading and keying / grouping and ordering / formatting and writing), and, where --ref names a compiled reference
gzfastq_uniq, its wall on the same files in the same session and whether the outputs are equal.  `--profile` adds one
rocprofv3 --kernel-trace --stats run of its own (no counters) on the plain single-end file and sets every kernel's time
against the bytes it has to move.

    python scripts/uniq_e2e.py [--reads 8e6] [--ref PATH] [--profile] [--out profiles/uniq/e2e.json]
"""
import argparse
import csv
import glob
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
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
HBM_PEAK = 8.0e12   # bytes / s


def digest_dir(d):
    out = {}
    for fn in sorted(os.listdir(d)):
        h = hashlib.sha256()
        with open(os.path.join(d, fn), "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        out[fn] = (os.path.getsize(os.path.join(d, fn)), h.hexdigest())
    return out


def timed(cmd, cwd, env=None, reps=1):
    walls, p = [], None
    for _ in range(reps):
        for fn in os.listdir(cwd):
            os.remove(os.path.join(cwd, fn))
        t0 = time.perf_counter()
        p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        walls.append(round(time.perf_counter() - t0, 3))
        assert p.returncode == 0, (cmd, p.stderr.decode("latin-1")[-2000:])
    return walls, p.stderr.decode("latin-1")


def split_seconds(stderr):
    m = re.search(r"\[hpn\] uniq: reading and keying ([\d.]+) s, grouping and ordering ([\d.]+) s, formatting and writing ([\d.]+) s; (\d+) hash clashes", stderr)
    u = re.search(r"unique reads number = (\d+)\((\d+) / (\d+) =", stderr)
    return {"read_key_s": float(m.group(1)), "group_order_s": float(m.group(2)), "format_write_s": float(m.group(3)), "hash_clashes": int(m.group(4)),
            "unique": int(u.group(1)), "records": int(u.group(3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--ref", default=None, help="compiled reference gzfastq_uniq (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniq", "e2e.json"))
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
    tmp = tempfile.mkdtemp(prefix="uniq_e2e_")
    files = {"plain": os.path.join(tmp, "reads_1.fq"), "gzip1": os.path.join(tmp, "one_1.fq.gz")}
    mates = {"plain": os.path.join(tmp, "reads_2.fq"), "gzip1": os.path.join(tmp, "one_2.fq.gz")}
    open(files["plain"], "wb").write(rows.tobytes())
    open(files["gzip1"], "wb").write(bench_extra._gz_single_member(rows.tobytes(), 256, 16))
    rows[:, 13:13 + L] = rows[:, 13:13 + L][:, ::-1].copy()
    open(mates["plain"], "wb").write(rows.tobytes())
    open(mates["gzip1"], "wb").write(bench_extra._gz_single_member(rows.tobytes(), 256, 16))
    del raw, rows
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "duplicated_fraction": a.dup, "reference_binary": bool(ref), "files": {}}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    for kind, path in files.items():
        r = {"bytes": os.path.getsize(path)}
        r["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path], work, reps=a.reps)
        for mode, extra in (("single", []), ("paired", ["-2", mates[kind]])):
            walls, err = timed([os.path.join(BIN, "gzfastq_uniq"), "-1", path] + extra + ["-o", "o"], work, {"HPN_TIMING": "1"}, reps=a.reps)
            m = {"wall_s": walls, **split_seconds(err), "outputs": {k: v[0] for k, v in digest_dir(work).items()}}
            print(kind, mode, m, flush=True)
            if ref and kind == "plain":   # (the reference reads gzip through zlib on one core: its plain-text wall is its best case)
                ours = digest_dir(work)
                rw, _ = timed([ref, "-1", path] + extra + ["-o", "o"], work)
                m["reference_wall_s"] = rw
                m["equals_reference"] = digest_dir(work) == ours
                print(kind, mode, "reference", rw, m["equals_reference"], flush=True)
            r[mode] = m
        result["files"][kind] = r
    if a.profile:
        d = os.path.join(tmp, "prof")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "uniq", "--", os.path.join(BIN, "gzfastq_uniq"), "-1", files["plain"],
                        "-o", "o"], cwd=work, env={**os.environ, "HPN_FULL_EXIT": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        stats = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
        result["kernel_ms_plain_single"] = stats
        # the bytes each kernel has to move.  U keys of N records; a sort pass reads 12 B twice and writes them once per key
        s = result["files"]["plain"]["single"]
        N, U = s["records"], s["unique"]
        out_rec = rec + 2
        words = (L + 7) // 8
        must = {"k_text_lines": N * (rec + 4), "k_uniq_keys": N * (20 + 2 * L + 32), "k_uniq_pair": N * (32 + 20), "k_uniq_flags": N * (12 + 2 * 32 + 2 * L + 4),
                "k_uniq_reduce": N * (16 + 4 + 12), "k_radix_hist": (8 * N + 8 * (1 + words) * U) * 8, "k_radix_scatter": (8 * N + 8 * (1 + words) * U) * 24,
                "k_uniq_seq_word": words * U * (4 + 4 + 32 + 8 + 8), "k_uniq_write": 2 * U * (2 * out_rec + 32 + 20), "k_uniq_sizes": 2 * U * (32 + 12)}   # (two outputs are formatted)
        model = {}
        for k, b in must.items():
            v = next((x for name, x in stats.items() if k in name), None)
            if v and v["total_ms"] > 0:
                model[k] = {"calls": v["calls"], "ms": v["total_ms"], "bytes": int(b), "GBps": round(b / (v["total_ms"] * 1e-3) / 1e9, 1),
                            "share_of_hbm_peak": round(b / (v["total_ms"] * 1e-3) / HBM_PEAK, 4)}
        result["kernel_model_plain_single"] = model
        result["kernel_ms_total"] = round(sum(v["total_ms"] for v in stats.values()), 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
