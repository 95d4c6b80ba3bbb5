"""CPU: scripts/bam_synth.cpp's --targets mode and tests/c4.py (the checker of the hg38-shaped file test) are held to the
compiled reference on a small instance: the reference's own bam2depth / bam_sliding_count read the BAM + .bai the generator
writes, and the oracle's answers computed from the generator's SoA sidecar must be those bytes.  The reference's reports are
stored under tests/golden/c4_synth/ (tests/golden/make_golden.py) with the MD5 of the inflated BAM they were made from: the
generator must write that very BAM again."""
import gzip
import hashlib
import os

import c4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "c4_synth")


def _golden(case, name):
    path = os.path.join(GOLD, case, name)
    if os.path.exists(path + ".gz"):
        with gzip.open(path + ".gz", "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


def _same_bam(case, bam):
    """The generator wrote the BAM the stored reports were made from (compared inflated: BGZF bytes depend on zlib)."""
    with open(bam, "rb") as f:
        got = hashlib.md5(gzip.decompress(f.read())).hexdigest()
    assert got == _golden(case, "bam_inflated.md5").decode().strip(), f"{bam}: not the BAM of tests/golden/c4_synth/{case}"


def test_generator_sidecar_and_checker_against_the_reference(tmp_path):
    tg = [("chr1", 300000, 40000), ("chrTiny", 16569, 3300), ("chrEmpty", 5000, 0), ("chrX", 120000, 9000)]
    # (a target without reads: bam2depth still prints its windows, bam_sliding_count leaves its row out)
    bam, prefix = c4.synth(str(tmp_path), "t.bam", [t for t in tg], 3)
    _same_bam("targets", bam)
    soa = c4.Soa(prefix, len(tg))
    assert soa.n == sum(r for _, _, r in tg)
    W = 2000
    # reference: bam2depth -w 2000 -o d t.bam
    bed = _golden("targets", "t.bam.1.bedGraph")
    dep = _golden("targets", "d.1.depth")
    ob, od = b"", b""
    for t, (name, tlen, _) in enumerate(tg):
        runs, bins = c4.oracle_depth_target(soa, tg, t, W)
        b, d = c4.oracle_target_text(name, tlen, W, runs, bins)
        ob, od = ob + b, od + d
    assert ob == bed and od == dep
    # reference: bam_sliding_count -w 2000 -o s t.bam
    assert c4.oracle_window_report(soa, tg, W) == _golden("targets", "s.txt")


def test_float32_gc_sum_beyond_2_pow_24_is_order_dependent_and_the_oracle_replays_it(tmp_path):
    """bam_sliding_count.c:121 adds an unsigned short to a float per record: past 2^24 every += rounds, so the window's value
    depends on the order of the records.  The oracle replays the additions in record order (orc_window_gc_f32) and must print the
    reference's digits; a sum taken as an integer and converted prints others -- which is why the tool refuses such a window
    (tests/test_c4_files_gpu.py::test_gc_window_beyond_the_float32_domain_is_refused)."""
    import numpy as np
    import orc
    tg = [("chrBig", 2_000_000, 260_000), ("chrS", 50_000, 1000)]
    bam, prefix = c4.synth(str(tmp_path), "g.bam", tg, 3)
    soa = c4.Soa(prefix, len(tg))
    _same_bam("gc_f32", bam)
    W = 3_000_000
    ref = _golden("gc_f32", "s.txt")   # reference: bam_sliding_count -w 3000000 -o s g.bam
    assert c4.oracle_window_report(soa, tg, W) == ref
    rc, off, bins, gc, ln, touched, _ = orc.window_counts(c4.whole_view(soa, tg), W)
    assert rc == 0 and int(gc[0]) >= 1 << 24                       # the window is past the exact range ...
    naive = np.float32(int(gc[0])) / np.float32(ln[0]) * np.float32(100)
    assert ("%f" % naive).encode() not in ref.split(b"\n")[1]      # ... and the converted integer sum would print other digits
