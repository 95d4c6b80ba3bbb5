"""fastq2twobit and twoBit2seq end to end on the README's 8e6 x 150 bp input: plain text and one gzip member in, the packed file
back out as text.

The input is bench_extra's synthetic text (sort_e2e's without the duplicated sequences: nothing here looks at them).  For every
file: the wall of fastq_count (the floor: same ingest, nothing kept) and the walls of `fastq2twobit` with the tool's HPN_TIMING
split (reading and framing / packing / writing); then `twoBit2seq` on the packed file with its split (reading / unpacking with
both copies / writing), and whether its lines are the reads' sequences, last read first.  Where --ref names a directory with a
compiled reference fastq2twobit and twoBit2seq, their walls on the plain file in the same session and whether the outputs are
equal.  `--profile` adds one rocprofv3 --kernel-trace --stats run of its own (no counters) per tool.

    python scripts/twobit_e2e.py [--reads 8e6] [--ref DIR] [--profile] [--out profiles/twobit/e2e.json]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")

from uniq_e2e import digest_dir, timed  # noqa: E402


def pack_split(stderr):
    m = re.search(r"\[hpn\] twobit pack: reading and framing ([\d.]+) s, packing ([\d.]+) s, writing ([\d.]+) s; (\d+) bytes", stderr)
    return {"read_frame_s": float(m.group(1)), "pack_s": float(m.group(2)), "write_s": float(m.group(3)), "out_bytes": int(m.group(4))}


def unpack_split(stderr):
    m = re.search(r"\[hpn\] twobit unpack: reading ([\d.]+) s, unpacking \(with both copies\) ([\d.]+) s, writing ([\d.]+) s; (\d+) records", stderr)
    return {"read_s": float(m.group(1)), "unpack_copy_s": float(m.group(2)), "write_s": float(m.group(3)), "records": int(m.group(4))}


def kernel_stats(cmd, cwd, d, name):
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", name, "--"] + cmd, cwd=cwd,
                   env={**os.environ, "HPN_FULL_EXIT": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    stats = {}
    for fn in glob.glob(os.path.join(d, "**", name + "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--ref", default=None, help="directory with a compiled reference fastq2twobit and twoBit2seq (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twobit", "e2e.json"))
    a = ap.parse_args()
    n, L = int(a.reads), 150
    import torch  # noqa: F401
    import highperformancengs_amd as hp
    import bench_extra

    ctx = hp.Context(0)
    raw = bench_extra._fastq_text(ctx, n, L, 40)
    ctx.close()
    rec = raw.size // n
    rows = raw.reshape(n, rec)
    want = hashlib.sha256()      # what twoBit2seq must print: the sequences, last read first, every letter that is not A, C, G as T
    seqs = rows[::-1, 13:13 + L + 1].copy()
    assert (seqs[:, L] == 10).all()
    seqs[:, :L][~((seqs[:, :L] == 65) | (seqs[:, :L] == 67) | (seqs[:, :L] == 71))] = 84
    want.update(seqs.tobytes())
    tmp = tempfile.mkdtemp(prefix="twobit_e2e_")
    files = {"plain": os.path.join(tmp, "reads.fq"), "gzip1": os.path.join(tmp, "one.fq.gz")}
    open(files["plain"], "wb").write(rows.tobytes())
    open(files["gzip1"], "wb").write(bench_extra._gz_single_member(rows.tobytes(), 256, 16))
    del raw, rows, seqs
    ref = {t: os.path.join(os.path.abspath(a.ref), t) for t in ("fastq2twobit", "twoBit2seq")} if a.ref else None
    if ref and not all(os.access(p, os.X_OK) for p in ref.values()):
        ref = None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "reference_binaries": bool(ref), "files": {}}
    work, keep = os.path.join(tmp, "work"), os.path.join(tmp, "packed.2bit")
    os.makedirs(work)
    for kind, path in files.items():
        r = {"bytes": os.path.getsize(path)}
        r["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path], work, reps=a.reps)
        walls, err = timed([os.path.join(BIN, "fastq2twobit"), "-i", path, "-o", "o"], work, {"HPN_TIMING": "1"}, reps=a.reps)
        r["fastq2twobit"] = {"wall_s": walls, **pack_split(err), "outputs": {k: v[0] for k, v in digest_dir(work).items()}}
        print(kind, "fastq2twobit", r["fastq2twobit"], flush=True)
        if kind == "plain":
            ours = digest_dir(work)
            shutil.copy(os.path.join(work, "o_sort_by_seq.fq"), keep)
            if ref:
                rw, _ = timed([ref["fastq2twobit"], "-i", path, "-o", "o"], work)
                r["fastq2twobit"].update(reference_wall_s=rw, equals_reference=digest_dir(work) == ours)
        result["files"][kind] = r
    walls, err = timed([os.path.join(BIN, "twoBit2seq"), "-i", keep, "-o", "o"], work, {"HPN_TIMING": "1"}, reps=a.reps)
    ours = digest_dir(work)
    u = {"bytes": os.path.getsize(keep), "wall_s": walls, **unpack_split(err), "outputs": {k: v[0] for k, v in ours.items()},
         "lines_are_the_reads_reversed": ours["o.decompress"][1] == want.hexdigest()}
    if ref:
        rw, _ = timed([ref["twoBit2seq"], "-i", keep, "-o", "o"], work)
        u.update(reference_wall_s=rw, equals_reference=digest_dir(work) == ours)
    print("twoBit2seq", u, flush=True)
    result["twoBit2seq"] = u
    if a.profile:
        d = os.path.join(tmp, "prof")
        result["kernel_ms_fastq2twobit_plain"] = kernel_stats([os.path.join(BIN, "fastq2twobit"), "-i", files["plain"], "-o", "o"], work, d, "pack")
        result["kernel_ms_twoBit2seq"] = kernel_stats([os.path.join(BIN, "twoBit2seq"), "-i", keep, "-o", "o"], work, d, "unpack")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
