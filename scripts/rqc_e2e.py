"""rfastqc_tally end to end on the README's 8e6 x 150 bp input with 22 % of its reads duplicates: plain text and one gzip member,
single-end and as pairs.

The input is uniq_e2e's: bench_extra's synthetic text with the sequence of 22 reads in a hundred overwritten by the sequence of
another read (the mate file: the same reads reversed, so a pair repeats exactly when its first mate does).  For every file: the
wall of fastq_count (the floor: same ingest, nothing kept), the walls of gzfastq_uniq on the same file (the same store and
grouping, plus two 2 GB outputs) and the walls of `rfastqc_tally` with the tool's HPN_TIMING split (reading and framing /
tallying and grouping / writing).  Where --ref names a driver built as tests/golden/make_golden_rqc.py builds it (the reference's
Rgzfastq_uniq.c and hashtbl.c with tests/golden/rshim/), its wall on the plain files in the same session and whether every list
element is equal.  `--profile` adds one rocprofv3 --kernel-trace --stats run of its own (no counters) on the plain single-end
file and sets k_rqc_key and k_rqc_flags against the key bytes they have to read.

    python scripts/rqc_e2e.py [--reads 8e6] [--ref PATH] [--profile] [--out profiles/rqc/e2e.json]
"""
import argparse
import json
import os
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")

from twobit_e2e import kernel_stats  # noqa: E402
from uniq_e2e import HBM_PEAK, digest_dir, timed  # noqa: E402

NAMES = ["dup.i32"] + ["R%d.%s" % (m, s) for m in (1, 2) for s in ("gc.f64", "quality.i32", "nucleotide.i32", "length.i32")]


def split(stderr):
    m = re.search(r"\[hpn\] rfastqc_tally: reading and framing ([\d.]+) s, tallying and grouping ([\d.]+) s, writing ([\d.]+) s; (\d+) reads, (\d+) keys, (\d+) clashes", stderr)
    return {"read_frame_s": float(m.group(1)), "tally_group_s": float(m.group(2)), "write_s": float(m.group(3)), "records": int(m.group(4)),
            "unique": int(m.group(5)), "hash_clashes": int(m.group(6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--dup", type=float, default=0.22)
    ap.add_argument("--ref", default=None, help="compiled reference driver (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rqc", "e2e.json"))
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
    tmp = tempfile.mkdtemp(prefix="rqc_e2e_")
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
    tool = os.path.join(BIN, "rfastqc_tally")
    for kind, path in files.items():
        r = {"bytes": os.path.getsize(path)}
        r["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path], work, reps=a.reps)
        for mode, extra in (("single", []), ("paired", ["-2", mates[kind]])):
            uw, _ = timed([os.path.join(BIN, "gzfastq_uniq"), "-1", path] + extra + ["-o", "o"], work, reps=a.reps)
            walls, err = timed([tool, "-1", path] + extra + ["-o", "o"], work, {"HPN_TIMING": "1"}, reps=a.reps)
            ours = digest_dir(work)
            m = {"wall_s": walls, "gzfastq_uniq_wall_s": uw, **split(err), "outputs": {k: v[0] for k, v in ours.items()}}
            print(kind, mode, m, flush=True)
            if ref and kind == "plain":   # (the reference reads gzip through zlib on one core: its plain-text wall is its best case)
                rw, _ = timed([ref, path] + extra[1:], work)
                theirs = digest_dir(work)
                m["reference_wall_s"] = rw
                m["equals_reference"] = all(theirs.get("e%d.bin" % k) == ours.get("o." + s) for k, s in enumerate(NAMES[:len(ours)]))
                print(kind, mode, "reference", rw, m["equals_reference"], flush=True)
            r[mode] = m
        result["files"][kind] = r
    if a.profile:
        stats = kernel_stats([tool, "-1", files["plain"], "-o", "o"], work, os.path.join(tmp, "prof"), "rqc")
        result["kernel_ms_plain_single"] = stats
        # the bytes the two new kernels have to move: a 150-base read's key is its first 50 bytes.  key: one 16-byte descriptor and
        # the key per record, 13 bytes written; flags: 12 bytes per position, a flag written, and where the hashes are equal (the
        # duplicates) two descriptors and two keys
        s = result["files"]["plain"]["single"]
        N, U = s["records"], s["unique"]
        must = {"k_rqc_key": N * (16 + 50 + 13), "k_rqc_flags": N * (12 + 1 + 4) + (N - U) * 2 * (16 + 50)}
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
