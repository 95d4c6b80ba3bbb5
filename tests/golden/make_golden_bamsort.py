#!/usr/bin/env python3
"""Records what the reference's `samtools sort` does: tests/golden/bamsort/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of tests/golden/make_golden_bai.py, into a TEMPORARY
directory and linked to a driver of our own that calls its bam_sort(argc, argv) -- the function behind `samtools sort`.  Every
case runs in a directory of its own under a limit of 20 s with its input copied there as in.bam.  Status, stderr, the directory's
listing afterwards and the output (size + SHA-256; whole, base64, up to 2 KiB) are stored as data.  No reference text is stored
and nothing compiled stays.  The inputs come from tests/bamsort_inputs.py (fixed seeds) and are NOT stored: the manifest holds
their SHA-256, the tests make them again and check it.

"expect" is `same` for every case the reference finishes; `refuse` only where it crashed or ran past the limit, with the reason
in "why".  Before anything is written the sequential restatement tests/bamsort_ref.py is held to every finished run."""
import base64
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bamsort_inputs  # noqa: E402  (tests/bamsort_inputs.py)
import bamsort_ref  # noqa: E402
import make_golden_bai  # noqa: E402  (the recipe: sources, flags)

OUT = os.path.join(HERE, "bamsort")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 20
DRIVER = "int bam_sort(int argc, char *argv[]);\nint main(int argc, char *argv[])\n{\n    return bam_sort(argc, argv);\n}\n"


def build_reference(ref, tmp):
    make_golden_bai.build_reference(ref, tmp)          # libbam.a under tmp/samtools-0.1.19
    sam = os.path.join(tmp, "samtools-0.1.19")
    drv = os.path.join(tmp, "sort_driver.c")
    with open(drv, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "sort")          # (argv[0] is `sort`, as samtools hands it to bam_sort)
    subprocess.check_call(["gcc", "-O2", "-w", drv, "-o", exe, "-L", sam, "-lbam", "-lpthread", "-lm", "-lz"])
    return exe


def mem_for(recs, n_threads, want):
    """the smallest -m for which the reference makes `want(record counts of its files)` true, by the model of its accounting"""
    sizes, key = [len(r) for r in recs], [bamsort_ref.keys(*bamsort_ref.fields(r))[0] for r in recs]
    for m in range(2000, bamsort_ref.fresh_mem(sizes) + 2, 7):
        files = bamsort_ref.plan_chunks(sizes, m * max(1, n_threads), max(1, n_threads), lambda idx: sorted(idx, key=lambda i: key[i]))
        if want([len(f) for f in files]):
            return m
    raise AssertionError("no -m value")


def cases(inputs):
    c = [{"id": n, "input": n, "opts": []} for n in bamsort_inputs.names()]
    sizes = bamsort_ref.parse(inputs["strands"]).recs
    total = bamsort_ref.fresh_mem([len(r) for r in sizes])
    m3 = mem_for(sizes, 1, lambda p: len(p) == 3)
    m9 = mem_for(sizes, 1, lambda p: len(p) == 9)
    big = mem_for(sizes, 2, lambda p: len(p) == 4 and p[0] >= 64 and p[1] >= 64)          # chunks of 128 records and more: two files each
    small = mem_for(sizes, 2, lambda p: len(p) > 4 and all(n < 128 for n in p))          # chunks below 128 records: one file each
    on = [("l0", ["-l", "0"]), ("l1", ["-l", "1"]), ("l9", ["-l", "9"]), ("l12", ["-l", "12"]), ("t2", ["-@", "2"]),
          ("m_none", ["-m", str(total + 1)]), ("m_exact", ["-m", str(total)]), ("m_3", ["-m", str(m3)]), ("m_9", ["-m", str(m9)]),
          ("m_1K", ["-m", "1K"]), ("t2_m_big", ["-@", "2", "-m", str(big)]), ("t2_m_small", ["-@", "2", "-m", str(small)]),
          ("l1_m_3", ["-l", "1", "-m", str(m3)]), ("l0_m_3", ["-l", "0", "-m", str(m3)]), ("f", ["-f"]), ("o", ["-o"]), ("n", ["-n"])]
    c += [{"id": "strands_" + k, "input": "strands", "opts": o} for k, o in on]
    for name in ("pos_out_2p30m1", "pos_out_m2", "pos_out_2p31m1", "tid_below", "unplaced_pos", "oversize"):
        s = bamsort_ref.parse(inputs[name]).recs
        m = mem_for(s, 1, lambda p: len(p) == 4)
        c.append({"id": name + "_m_4", "input": name, "opts": ["-m", str(m)]})
    c.append({"id": "pos_out_m2_t2_m", "input": "pos_out_m2", "opts": ["-@", "2", "-m", "3000"]})
    for name in ("oversize", "residues", "hd_long", "packed_1000"):
        c.append({"id": name + "_l0", "input": name, "opts": ["-l", "0"]})
    c.append({"id": "all_equal_n", "input": "all_equal", "opts": ["-n"]})
    c.append({"id": "missing_input", "input": None, "opts": [], "args": ["nope.bam", "out"]})
    c.append({"id": "one_argument", "input": "one_record", "opts": [], "args": ["in.bam"]})
    c.append({"id": "no_arguments", "input": None, "opts": [], "args": []})
    for e in c:
        e.setdefault("args", e["opts"] + ["in.bam", "out"])
        e["out"] = None if len(e["args"]) < 2 or e["input"] is None else "stdout" if "-o" in e["opts"] else "out" if "-f" in e["opts"] else "out.bam"
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = bamsort_inputs.materialize(made)
        inputs = bamsort_inputs.own_inputs()
        for c in cases(inputs):
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            data = inputs[c["input"]] if c["input"] else None
            if data is not None:
                with open(os.path.join(work, "in.bam"), "wb") as fh:
                    fh.write(data)
            why = None
            try:
                p = subprocess.run([exe] + c["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT)
                rc, err, out = p.returncode, p.stderr.decode("latin-1"), p.stdout
                if rc < 0:
                    why = "the reference ends with signal %d" % -rc
            except subprocess.TimeoutExpired:
                rc, err, out = None, "", b""
                why = "the reference runs past %d s" % TIME_LIMIT
            listing = sorted(fn for fn in os.listdir(work) if fn != "in.bam")
            got = None
            if why is None:
                assert rc in (0, 1), (c["id"], rc)
                if c["out"] == "stdout":
                    got = out
                    assert listing == [], (c["id"], listing)
                else:
                    assert out == b"" and listing in ([], [c["out"]]), (c["id"], listing)
                    if listing:
                        got = open(os.path.join(work, c["out"]), "rb").read()
                if data is not None and c["out"]:       # the restatement against the recording
                    want, want_err = bamsort_ref.sort(data, **bamsort_ref.options(c["opts"]))
                    assert want_err == err, (c["id"], want_err, err)
                    assert want == got, (c["id"], len(want), None if got is None else len(got))
                    assert c["id"] != c["input"] or bamsort_ref.route(data) in ("device", "host")
            else:
                err, rc, listing = "", None, []
            e = {"id": c["id"], "input": c["input"], "opts": c["opts"], "args": c["args"], "out": c["out"], "rc": rc, "stderr": err, "listing": listing,
                 "expect": "refuse" if why else "same", "why": why, "route": bamsort_ref.route(data) if data is not None and "-n" not in c["opts"] else "host",
                 "bam": None}
            if got is not None:
                e["bam"] = {"size": len(got), "sha256": hashlib.sha256(got).hexdigest(),
                            "b64": base64.b64encode(got).decode() if len(got) <= INLINE_LIMIT else None}
            manifest.append(e)
            print("%-24s rc %5s  %-6s %-6s %8s bytes  %s" % (c["id"], rc, e["expect"], e["route"], "-" if got is None else len(got),
                                                           (why or err.strip().replace("\n", " | "))[:100]))
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
