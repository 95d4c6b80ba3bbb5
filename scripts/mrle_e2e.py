"""gzfastq_mrle end to end on the README's 8e6 x 150 bp input with binned qualities: plain text and one gzip member in, the packed
quality lines and the decoded text out.

The input is bench_extra's synthetic text with its quality lines rewritten over the codec's six symbols  # / 7 < B F  the way a
sequencer with binned qualities writes them: a head of F of random length, then blocks of 8 equal symbols.  For every file: the
wall of fastq_count (the floor: same ingest, nothing kept), the wall of fastq2twobit (the yardstick: same session, a quarter of
the sequence bytes out) and the walls of `gzfastq_mrle -o o` with the tool's HPN_TIMING split (reading and framing / coding /
writing) and whether the decoded text is the quality lines; on the plain file also the run with the default prefix (both streams
on one descriptor).  Where --ref names a directory with a compiled reference gzfastq_mrle, its wall on the plain file in the same
session and whether the outputs are equal.  `--profile` adds one rocprofv3 --kernel-trace --stats run of its own (no counters).

    python scripts/mrle_e2e.py [--reads 8e6] [--ref DIR] [--profile] [--out profiles/mrle/e2e.json]
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")

from twobit_e2e import kernel_stats  # noqa: E402
from uniq_e2e import digest_dir, timed  # noqa: E402

SYM = np.frombuffer(b"#/7<BF", np.uint8)


def split(stderr):
    m = re.search(r"\[hpn\] mrle: reading and framing ([\d.]+) s, coding ([\d.]+) s, writing ([\d.]+) s; packed (\d+), text (\d+), shared (\d+) bytes", stderr)
    return {"read_frame_s": float(m.group(1)), "code_s": float(m.group(2)), "write_s": float(m.group(3)), "packed_bytes": int(m.group(4)),
            "text_bytes": int(m.group(5)), "shared_bytes": int(m.group(6))}


def binned(rows, L, seed):
    """Rewrites the quality columns of the (n, rec) records in place; returns the SHA-256 of the text the decoder must print."""
    n, rec = rows.shape
    q0 = rec - 1 - L
    rs = np.random.RandomState(seed)
    want = hashlib.sha256()
    for a in range(0, n, 1 << 20):      # a million records at a time
        b = min(n, a + (1 << 20))
        tail = np.repeat(SYM[rs.randint(0, 6, (b - a, (L + 7) // 8))], 8, axis=1)[:, :L]
        head = rs.randint(0, L + 1, (b - a, 1))
        q = np.where(np.arange(L)[None, :] < head, np.uint8(ord("F")), tail)
        rows[a:b, q0:q0 + L] = q
        want.update(rows[a:b, q0:].tobytes())      # the line and its newline
    return want.hexdigest()


def timed_stdout(cmd, cwd, reps):
    """timed() with standard output digested instead of kept: (walls, stderr, (bytes, sha256) of the last run's stdout)."""
    walls = []
    for _ in range(reps):
        for fn in os.listdir(cwd):
            os.remove(os.path.join(cwd, fn))
        h, size = hashlib.sha256(), 0
        t0 = time.perf_counter()
        p = subprocess.Popen(cmd, cwd=cwd, env={**os.environ, "HPN_TIMING": "1"}, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = []
        t = threading.Thread(target=lambda: err.append(p.stderr.read()))
        t.start()
        for blk in iter(lambda: p.stdout.read(1 << 24), b""):
            h.update(blk)
            size += len(blk)
        t.join()
        assert p.wait() == 0, (cmd, err[0].decode("latin-1")[-2000:])
        walls.append(round(time.perf_counter() - t0, 3))
    return walls, err[0].decode("latin-1"), (size, h.hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--ref", default=None, help="directory with a compiled reference gzfastq_mrle (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrle", "e2e.json"))
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
    want = binned(rows, L, 41)
    tmp = tempfile.mkdtemp(prefix="mrle_e2e_")
    files = {"plain": os.path.join(tmp, "reads.fq"), "gzip1": os.path.join(tmp, "one.fq.gz")}
    open(files["plain"], "wb").write(rows.tobytes())
    open(files["gzip1"], "wb").write(bench_extra._gz_single_member(rows.tobytes(), 256, 16))
    del raw, rows
    ref = os.path.join(os.path.abspath(a.ref), "gzfastq_mrle") if a.ref else None
    if ref and not os.access(ref, os.X_OK):
        ref = None
    result = {"reads": n, "read_length": L, "record_bytes": rec, "reference_binary": bool(ref), "files": {}}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    tool = os.path.join(BIN, "gzfastq_mrle")
    for kind, path in files.items():
        r = {"bytes": os.path.getsize(path)}
        r["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path], work, reps=a.reps)
        r["fastq2twobit_wall_s"], _ = timed([os.path.join(BIN, "fastq2twobit"), "-i", path, "-o", "o"], work, reps=a.reps)
        walls, err, text = timed_stdout([tool, "-i", path, "-o", "o"], work, a.reps)
        ours = digest_dir(work)
        r["gzfastq_mrle"] = {"wall_s": walls, **split(err), "packed_sha256": ours["o_sort_by_seq.fq"][1], "text_is_the_quality_lines": text[1] == want}
        print(kind, "gzfastq_mrle", r["gzfastq_mrle"], flush=True)
        if kind == "plain":
            walls, err, shared = timed_stdout([tool, "-i", path], work, a.reps)
            r["gzfastq_mrle_shared"] = {"wall_s": walls, "bytes": shared[0], "sha256": shared[1]}
            if ref:
                rw, _, rtext = timed_stdout([ref, "-i", path, "-o", "o"], work, 1)
                same = digest_dir(work) == ours and rtext == text
                rs, _, rshared = timed_stdout([ref, "-i", path], work, 1)
                r["reference"] = {"wall_s": rw, "equals": same, "shared_wall_s": rs, "shared_equals": rshared == shared}
        result["files"][kind] = r
    if a.profile:
        result["kernel_ms_plain"] = kernel_stats([tool, "-i", files["plain"], "-o", "o"], work, os.path.join(tmp, "prof"), "mrle")
        result["kernel_ms_fastq2twobit_plain"] = kernel_stats([os.path.join(BIN, "fastq2twobit"), "-i", files["plain"], "-o", "o"], work, os.path.join(tmp, "prof"), "pack")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
