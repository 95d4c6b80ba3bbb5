"""map_kseq and kbtree_kseq end to end on the 8e6 x 150 bp input of scripts/sort_e2e.py (22 % of the records repeat an earlier
sequence) and on the same reads as FASTA wrapped at 60: plain text and one gzip member each.

For every file: three walls per tool with the tool's HPN_TIMING split (reading and framing / ordering and formatting / writing),
the route it reports, the refinement's `rounds` and `refined`, and whether both tools wrote the same bytes.  The yardstick is
`gzfastq_sort -s` of this build on the FASTQ files, three walls in the same session: the kseq tools run the same ordering rounds
and write about 78 % of its output.  (FASTA as the reference reads it passes over every second header line -- tests/kseq_ref.py --
so the FASTA files give half the records.)  --ref DIR: where DIR holds the reference's sources, map_kseq.cpp is compiled into
oracle/_ref/map_kseq_ref first; whenever that binary exists its wall on the plain files is taken in the same session and its
output compared.  Without it the result says "not measured".

    python scripts/kseq_e2e.py [--reads 8e6] [--ref DIR] [--out profiles/kseq/e2e.json]
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "map_kseq_ref")
SPLIT = re.compile(r"\[hpn\] kseq: route (\w+), shape (\w+), (\d+) records; reading and framing ([\d.]+) s, ordering and formatting ([\d.]+) s, "
                   r"writing ([\d.]+) s; (\d+) rounds, (\d+) records refined")


def timed_stdout(cmd, env=None, reps=1):
    """walls, the last run's stderr, (size, SHA-256) of its stdout -- stdout goes to a file, as a user's redirection would"""
    walls, err, digest = [], "", None
    for _ in range(reps):
        with tempfile.NamedTemporaryFile(dir=os.path.dirname(cmd[-1])) as out:
            t0 = time.perf_counter()
            p = subprocess.run(cmd, env={**os.environ, **(env or {})}, stdout=out, stderr=subprocess.PIPE)
            walls.append(round(time.perf_counter() - t0, 3))
            assert p.returncode == 0, (cmd, p.stderr.decode("latin-1")[-2000:])
            err = p.stderr.decode("latin-1")
            h = hashlib.sha256()
            out.seek(0)
            for blk in iter(lambda: out.read(1 << 24), b""):
                h.update(blk)
            digest = (out.tell(), h.hexdigest())
    return walls, err, digest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--dup", type=float, default=0.3)
    ap.add_argument("--ref", default=None, help="the reference's source tree (compiled into oracle/_ref/ where it exists)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kseq", "e2e.json"))
    a = ap.parse_args()
    if a.ref and os.path.exists(os.path.join(a.ref, "map_kseq.cpp")):
        os.makedirs(os.path.dirname(REF_EXE), exist_ok=True)
        subprocess.check_call(["g++", "-O3", "-w", "-I", a.ref, os.path.join(a.ref, "map_kseq.cpp"), "-o", REF_EXE, "-lz"])
    ref = REF_EXE if os.access(REF_EXE, os.X_OK) else None
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
    rows[dst, 13:13 + L] = rows[rs.randint(0, n, dst.size), 13:13 + L]      # (sort_e2e.py's file)
    fa = np.empty((n, 13 + L + 3), np.uint8)      # ">name\n", the sequence in lines of 60, 60 and 30
    fa[:, :13] = rows[:, :13]
    fa[:, 0] = ord(">")
    fa[:, 13:73], fa[:, 73] = rows[:, 13:73], 10
    fa[:, 74:134], fa[:, 134] = rows[:, 73:133], 10
    fa[:, 135:165], fa[:, 165] = rows[:, 133:163], 10
    tmp = tempfile.mkdtemp(prefix="kseq_e2e_")
    files = {"fastq_plain": os.path.join(tmp, "reads.fq"), "fastq_gzip1": os.path.join(tmp, "reads.fq.gz"), "fasta_plain": os.path.join(tmp, "reads.fa"),
             "fasta_gzip1": os.path.join(tmp, "reads.fa.gz")}
    open(files["fastq_plain"], "wb").write(rows.tobytes())
    open(files["fastq_gzip1"], "wb").write(bench_extra._gz_single_member(rows.tobytes(), 256, 16))
    open(files["fasta_plain"], "wb").write(fa.tobytes())
    open(files["fasta_gzip1"], "wb").write(bench_extra._gz_single_member(fa.tobytes(), 256, 16))
    del raw, rows, fa
    result = {"reads": n, "read_length": L, "duplicated_fraction": a.dup, "reference_wall_s": "not measured", "files": {}}
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    for kind, path in files.items():
        r = {"bytes": os.path.getsize(path)}
        for tool in ("map_kseq", "kbtree_kseq"):
            walls, err, digest = timed_stdout([os.path.join(BIN, tool), path], {"HPN_TIMING": "1"}, reps=a.reps)
            m = SPLIT.search(err)
            r[tool] = {"wall_s": walls, "route": m.group(1), "shape": m.group(2), "records": int(m.group(3)), "read_frame_s": float(m.group(4)),
                       "order_format_s": float(m.group(5)), "write_s": float(m.group(6)), "rounds": int(m.group(7)), "refined": int(m.group(8)),
                       "distinct": int(err.splitlines()[0]), "stdout_bytes": digest[0], "stdout_sha256": digest[1]}
            print(kind, tool, r[tool], flush=True)
        r["tools_agree"] = r["map_kseq"]["stdout_sha256"] == r["kbtree_kseq"]["stdout_sha256"]
        if kind.startswith("fastq"):
            from uniq_e2e import timed
            walls, err = timed([os.path.join(BIN, "gzfastq_sort"), "-i", path, "-o", "o", "-s"], work, {"HPN_TIMING": "1"}, reps=a.reps)
            r["gzfastq_sort_by_seq"] = {"wall_s": walls, "output_bytes": sum(os.path.getsize(os.path.join(work, f)) for f in os.listdir(work))}
            print(kind, "gzfastq_sort -s", r["gzfastq_sort_by_seq"], flush=True)
        if ref and kind.endswith("plain"):
            walls, err, digest = timed_stdout([ref, path])
            r["reference"] = {"wall_s": walls, "equal": digest[1] == r["map_kseq"]["stdout_sha256"] and err == "%d\n" % r["map_kseq"]["distinct"]}
            result["reference_wall_s"] = "measured"
            print(kind, "reference", r["reference"], flush=True)
        result["files"][kind] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
