#!/usr/bin/env python3
"""K1 (k_tally_scan) on the resident 1e9 x 150 bp batch with the byte range starting s bytes into the quality buffer:
does the launch time (and, under scripts/pmc.py, FETCH_SIZE) depend on where the range starts relative to a 128-byte line?
The buffer is a fresh allocation (line-aligned), so s = 0 and s = 128 start ON a line, s = 16 / 64 inside one, and s = 112 puts
a kernel that sets vector 0 aside (the parent of the line-aligned origin) exactly on the lines: its first whole vector is byte 128.

    python3 scripts/k1_origin.py                          every shift, the whole list twice (the spread = pass 1 against pass 2)
    python3 scripts/k1_origin.py --shift 112 --launches 3   one shift (for a PMC pass: every k_tally_scan launch is that shift's)

Offsets are d_off + s over n - 1 records, so the range stays inside the buffer; total and SeqLen[150] are checked in closed form."""
import argparse, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import highperformancengs_amd as hp

ap = argparse.ArgumentParser()
ap.add_argument("--shift", type=int, action="append", help="byte shift(s); default 0 16 64 112 128")
ap.add_argument("--launches", type=int, default=6, help="launches per shift and pass; the first is not timed")
ap.add_argument("--passes", type=int, default=None, help="times the list of shifts is gone through (default 2, or 1 with --shift)")
ap.add_argument("--reads", type=float, default=1e9)
a = ap.parse_args()
shifts = a.shift or [0, 16, 64, 112, 128]
passes = a.passes or (1 if a.shift else 2)
n, L = int(a.reads), 150
assert all(0 <= s <= L for s in shifts) and a.launches >= 1

ctx = hp.Context(0)
dq = torch.empty(n * L, dtype=torch.uint8, device="cuda")
do = torch.empty(n + 1, dtype=torch.int64, device="cuda")
ctx.synth_fastq_dev(12345, 0, n, L, dq, None, do)
ctx.sync()
torch.cuda.synchronize()
print(f"{os.path.relpath(hp.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}: n={n - 1:.3e} x {L} bp, qual at 0x{dq.data_ptr():x} (mod 4096 = {dq.data_ptr() % 4096})", flush=True)
alg = (n - 1) * L + n * 8
cur = 0
for p in range(passes):
    for s in shifts:
        do += s - cur            # in place: the offsets stay where they are, only the byte range moves
        cur = s
        torch.cuda.synchronize()
        ts = []
        for r in range(a.launches):
            ctx.fastq_tally_dev(dq, do, n - 1)      # records 0 .. n-2 of the shifted offsets: bytes [s, s + (n-1) L)
            got = ctx.fastq_tally_fetch()
            if r or a.launches == 1:
                ts.append(ctx.last_kernel_ms(0))
            assert got.total == (n - 1) * L and int(got.seqlen[L]) == n - 1 and int(got.seqlen.sum()) == n - 1, (s, got.total)
        med = statistics.median(ts)
        print(f"pass {p} shift {s:4d}  start mod 128 = {(dq.data_ptr() + s) % 128:3d}  {med:7.3f} ms  (min {min(ts):7.3f} max {max(ts):7.3f})  "
              f"{alg / med / 1e6:7.1f} GB/s", flush=True)
