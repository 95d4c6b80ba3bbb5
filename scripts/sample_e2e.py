"""gzfastq_sample end to end on the README's 8e6 x 150 bp input: plain text, one gzip member, 32 gzip members.

For every file: the wall of fastq_count (reading and framing alone), of `gzfastq_sample -s F` with F chosen so that one
record in ten is kept (the synthetic names @r0000000017 hash into a narrow band, so F is the 10th percentile of their
hash values, not 0.1), of `-s 0.99999999` (everything kept: bound by compressing the output) and of `-n reads/10`; the
time spent compressing (the tool's HPN_TIMING line: thread-seconds of deflate, and the reading thread's wait for it); and, where --ref names a compiled reference sampler, its wall on the
same file in the same session with the decompressed outputs compared.  `--profile` adds one rocprofv3 --kernel-trace
--stats run of its own (no counters) for the per-kernel times and sets them against the bytes each kernel moves per record.

    python scripts/sample_e2e.py [--reads 8e6] [--ref PATH] [--profile | --profile-only] [--out profiles/sample/e2e.json]
"""
import argparse
import csv
import glob
import gzip
import hashlib
import json
import os
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
    """{output file: (decompressed size, sha256)} of a run directory."""
    out = {}
    for fn in sorted(os.listdir(d)):
        h, n = hashlib.sha256(), 0
        if os.path.getsize(os.path.join(d, fn)):
            with gzip.open(os.path.join(d, fn), "rb") as f:
                for blk in iter(lambda: f.read(1 << 24), b""):
                    h.update(blk)
                    n += len(blk)
        out[fn] = (n, h.hexdigest())
    return out


def timed(cmd, cwd, env=None, reps=1):
    walls, p = [], None
    for _ in range(reps):
        for fn in os.listdir(cwd):
            os.remove(os.path.join(cwd, fn))
        t0 = time.perf_counter()
        p = subprocess.run(cmd, cwd=cwd, env={**os.environ, **(env or {})}, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        walls.append(round(time.perf_counter() - t0, 3))
        assert p.returncode == 0, (cmd, p.stderr.decode()[-2000:])
    return walls, p.stderr.decode()


def compress_seconds(stderr):
    """The tool's HPN_TIMING line: deflate time summed over the threads, and how long the reading thread was held up by it."""
    for line in stderr.split("\n"):
        if line.startswith("[hpn] output: deflate"):
            w = line.split()
            return {"deflate_thread_s": float(w[3]), "threads": int(w[6]), "reader_waited_s": float(w[12])}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--ref", default=None, help="compiled reference gzfastq_sample (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-only", action="store_true", help="only the rocprofv3 runs, added to an existing --out file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample", "e2e.json"))
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
    # the fraction that keeps one record in ten: X31 of the 12-byte names, vectorised
    names = raw.reshape(n, rec)[:: max(1, n // 200000), :12].astype(np.uint32)
    h = np.zeros(len(names), np.uint32)
    for k in range(12):
        h = h * np.uint32(31) + names[:, k]
    frac = float(np.quantile((h & 0xFFFFFF) / float(1 << 24), 0.1))
    s_tenth, s_all, n_tenth = "%.8f" % frac, "0.99999999", str(n // 10)
    tmp = tempfile.mkdtemp(prefix="sample_e2e_")
    raw = raw.tobytes()
    files = {"plain": os.path.join(tmp, "reads.fq"), "gzip1": os.path.join(tmp, "one.fq.gz"), "gzip32": os.path.join(tmp, "members.fq.gz")}
    open(files["plain"], "wb").write(raw)
    if a.profile_only:
        files = {"plain": files["plain"]}
    else:
        open(files["gzip1"], "wb").write(bench_extra._gz_single_member(raw, 256, 16))
        open(files["gzip32"], "wb").write(bench_extra._gz_members(raw, 32, 16))
    del raw
    ref = os.path.abspath(a.ref) if a.ref and os.access(a.ref, os.X_OK) else None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "fraction_for_a_tenth": s_tenth, "reference_binary": bool(ref), "files": {}}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    if a.profile_only and os.path.exists(a.out):
        result = json.load(open(a.out))
    for kind, path in ({} if a.profile_only else files).items():
        r = {"bytes": os.path.getsize(path)}
        r["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path], work, reps=a.reps)
        for mode, args in (("s_tenth", ["-s", s_tenth]), ("s_all", ["-s", s_all]), ("n_tenth", ["-n", n_tenth])):
            walls, err = timed([os.path.join(BIN, "gzfastq_sample"), "-1", path] + args, work, {"HPN_TIMING": "1"}, reps=a.reps)
            m = {"args": args, "wall_s": walls, "compress": compress_seconds(err), "outputs": {k: v[0] for k, v in digest_dir(work).items()}}
            print(kind, mode, m, flush=True)
            if ref and mode != "s_all":   # (everything kept is 2.5 GB through one core's deflate: not worth the session's time)
                ours = digest_dir(work)
                rw, _ = timed([ref, "-1", path] + args, work)
                m["reference_wall_s"] = rw
                m["equals_reference"] = digest_dir(work) == ours
                print(kind, mode, "reference", rw, m["equals_reference"], flush=True)
            r[mode] = m
        result["files"][kind] = r
    if a.profile or a.profile_only:
        prof = os.path.join(tmp, "prof")
        kernels = {}
        for mode, args in (("s_tenth", ["-s", s_tenth]), ("s_all", ["-s", s_all]), ("n_tenth", ["-n", n_tenth])):
            d = os.path.join(prof, mode)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sample", "--", os.path.join(BIN, "gzfastq_sample"), "-1", files["plain"]] + args,
                           cwd=work, env={**os.environ, "HPN_FULL_EXIT": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            stats = {}
            for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(fn)):
                    stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
            kernels[mode] = stats
        result["kernel_ms_plain"] = kernels
        # bytes per record each kernel has to move (index 16 B + the line end in front 4 B, the 12-byte name as one 16-byte load, off[] 8 B,
        # 8 B per kept ordinal; a kept record read once and written once with its 8 + 8 + 20 B of bookkeeping)
        kept = {"s_tenth": 0.1, "s_all": 1.0, "n_tenth": 0.1}
        model = {}
        for mode, st in kernels.items():
            sel = next((v for k, v in st.items() if "k_sample_select" in k), None)
            wr = next((v for k, v in st.items() if "k_sample_write" in k), None)
            ln = next((v for k, v in st.items() if "k_text_lines" in k), None)
            passes = 2 if mode == "n_tenth" else 1     # (-n frames the file twice; only the second pass selects)
            b_sel = n * (20 + (16 if mode != "n_tenth" else 0) + 8 + 8 * kept[mode])
            b_wr = n * kept[mode] * (2 * rec + 10 + 36)
            model[mode] = {k: {"bytes": int(b), "ms": v["total_ms"], "GBps": round(b / (v["total_ms"] * 1e-3) / 1e9, 1),
                               "share_of_hbm_peak": round(b / (v["total_ms"] * 1e-3) / HBM_PEAK, 4)}
                           for k, b, v in (("k_sample_select", b_sel, sel), ("k_sample_write", b_wr, wr), ("k_text_lines", passes * n * (rec + 4), ln)) if v}
        result["kernel_model_plain"] = model
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
