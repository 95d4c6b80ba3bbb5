"""pick_pair end to end on the README's 8e6 x 150 bp input, written twice with reads lost.

The input is bench_extra's synthetic text (names without a space, ascending: the whole names are compared).  Three scenarios, all
plain text:
  both_lost     one read in 50 removed from EACH copy, independently (never one of the last four: the reference crashes when one
                file runs out in front of the other).  A B-only read directly in front of an A-only one makes the reference's walk
                mispair, so no proposal of the device verifies here and the tool walks on the host (docs/kernels/fastq_pair.md).
  one_lost      one read in 50 removed from the second copy only: the join.
  nothing_lost  both copies whole: the identity.
For each: the walls of `pick_pair`, the route it names and its HPN_TIMING split (reading and pairing / deflating and writing),
the record counts, and the walls of fastq_count on the first file (the floor of reading ONE of the two).  Where --ref names a
directory with a compiled reference pick_pair, its wall in the same session and whether the inflated outputs are equal; that
number can only be taken where the reference tree is checked out.  `--profile` adds one rocprofv3 --kernel-trace --stats run of
its own (no counters) per scenario.  No speed threshold is asserted.

    python scripts/pair_e2e.py [--reads 8e6] [--ref DIR] [--profile] [--out profiles/pair/e2e.json]
"""
import argparse
import gzip
import hashlib
import json
import os
import re
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")

from twobit_e2e import kernel_stats  # noqa: E402
from uniq_e2e import timed  # noqa: E402


def split(stderr):
    m = re.search(r"\[hpn\] pick_pair: route (\w+); reading and pairing ([\d.]+) s, deflating and writing ([\d.]+) s; (\d+) pairs, (\d+) \+ (\d+) singles", stderr)
    return {"route": m.group(1), "read_pair_s": float(m.group(2)), "deflate_write_s": float(m.group(3)), "pairs": int(m.group(4)),
            "singles": [int(m.group(5)), int(m.group(6))]}


def inflated_digests(d):
    """{name: (inflated size, sha256)} of the .gz files of a directory."""
    out = {}
    for fn in sorted(os.listdir(d)):
        if not fn.endswith(".gz"):
            continue
        h, n = hashlib.sha256(), 0
        with gzip.open(os.path.join(d, fn), "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
                n += len(blk)
        out[fn] = (n, h.hexdigest())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=8e6)
    ap.add_argument("--ref", default=None, help="directory with a compiled reference pick_pair (absent: no comparison)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair", "e2e.json"))
    a = ap.parse_args()
    n, L = int(a.reads), 150
    import torch  # noqa: F401
    import highperformancengs_amd as hp
    import bench_extra

    ctx = hp.Context(0)
    raw = bench_extra._fastq_text(ctx, n, L, 40)
    ctx.close()
    rows = raw.reshape(n, raw.size // n)
    rs = np.random.RandomState(50)
    keep = [rs.randint(0, 50, n) != 0 for _ in range(2)]
    for k in keep:
        k[-4:] = True      # (a mispair next to the end would leave one file exhausted in front of the other)
    tmp = tempfile.mkdtemp(prefix="pair_e2e_")
    path = lambda name: os.path.join(tmp, name)
    open(path("whole.fq"), "wb").write(rows.tobytes())
    open(path("lost_1.fq"), "wb").write(rows[keep[0]].tobytes())
    open(path("lost_2.fq"), "wb").write(rows[keep[1]].tobytes())
    del raw, rows
    scenarios = {"both_lost": ("lost_1.fq", "lost_2.fq"), "one_lost": ("whole.fq", "lost_2.fq"), "nothing_lost": ("whole.fq", "whole.fq")}
    ref = os.path.join(os.path.abspath(a.ref), "pick_pair") if a.ref else None
    if ref and not os.access(ref, os.X_OK):
        ref = None
    result = {"reads": n, "read_length": L, "lost_one_in": 50, "reference_binary": bool(ref), "scenarios": {}}
    work = path("work")
    os.makedirs(work)
    result["fastq_count_wall_s"], _ = timed([os.path.join(BIN, "fastq_count"), path("whole.fq")], work, reps=a.reps)
    for name, (f1, f2) in scenarios.items():
        cmd = ["-1", path(f1), "-2", path(f2), "-o", "o"]
        walls, err = timed([os.path.join(BIN, "pick_pair")] + cmd, work, {"HPN_TIMING": "1"}, reps=a.reps)
        r = {"bytes": [os.path.getsize(path(f1)), os.path.getsize(path(f2))], "wall_s": walls, **split(err)}
        ours = inflated_digests(work)
        r["outputs"] = {k: v[0] for k, v in ours.items()}
        if ref:
            rw, _ = timed([ref] + cmd, work)
            r.update(reference_wall_s=rw, equals_reference=inflated_digests(work) == ours)
        if a.profile:
            r["kernel_ms"] = kernel_stats([os.path.join(BIN, "pick_pair")] + cmd, work, path("prof"), name)
        print(name, r, flush=True)
        result["scenarios"][name] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result, sort_keys=True))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
