#!/usr/bin/env python3
"""Records what the reference's `samtools merge` does: tests/golden/bammerge/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of tests/golden/make_golden_bai.py, into a TEMPORARY
directory and linked to a driver of our own that calls its bam_merge(argc, argv) -- the function behind `samtools merge`.  Every
case runs in a directory of its own under a limit of 20 s with its inputs written there as in1.bam, in2.bam, ...  Status, stderr,
the directory's listing afterwards and the output (size + SHA-256; whole, base64, up to 2 KiB) are stored as data.  No reference
text is stored and nothing compiled stays.  The inputs come from tests/bammerge_inputs.py (fixed seeds) and are NOT stored: the
manifest holds their SHA-256, the tests make them again and check it.

"expect" is `same` for every case the reference finishes; `refuse` only where it crashed or ran past the limit, with the reason
in "why".  Before anything is written the sequential restatement tests/bammerge_ref.py is held to every finished run."""
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
import bammerge_inputs  # noqa: E402  (tests/bammerge_inputs.py)
import bammerge_ref  # noqa: E402
import make_golden_bai  # noqa: E402  (the recipe: sources, flags)

OUT = os.path.join(HERE, "bammerge")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 20
OLD = b"what was here before\n"          # the content of an output that exists before the run
DRIVER = "int bam_merge(int argc, char *argv[]);\nint main(int argc, char *argv[])\n{\n    return bam_merge(argc, argv);\n}\n"


def build_reference(ref, tmp):
    make_golden_bai.build_reference(ref, tmp)          # libbam.a under tmp/samtools-0.1.19
    sam = os.path.join(tmp, "samtools-0.1.19")
    drv = os.path.join(tmp, "merge_driver.c")
    with open(drv, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "merge")          # (argv[0] is `merge`, as samtools hands it to bam_merge)
    subprocess.check_call(["gcc", "-O2", "-w", drv, "-o", exe, "-L", sam, "-lbam", "-lpthread", "-lm", "-lz"])
    return exe


def cases(sets):
    """id, set (None: no input is written), opts, args (None: options, the output, every file of the set), out ('out.bam',
    'stdout' or None), old (the output exists before the run), h (the -h file of bammerge_inputs.header_files() written as h.sam)"""
    c = [{"id": n, "set": n, "opts": []} for n in sorted(sets)]
    on = [("l0", ["-l", "0"]), ("l1", ["-l", "1"]), ("l9", ["-l", "9"]), ("l12", ["-l", "12"]), ("l_neg", ["-l", "-3"]), ("u", ["-u"]), ("1", ["-1"]),
          ("u_1_l9", ["-u", "-1", "-l", "9"]), ("1_l9", ["-1", "-l", "9"]), ("t2", ["-@", "2"]), ("u_t2", ["-u", "-@", "2"]), ("f", ["-f"]), ("r", ["-r"]),
          ("n", ["-n"]), ("nr_u", ["-nr", "-u"])]
    c += [{"id": "three_sorted_" + k, "set": "three_sorted", "opts": o} for k, o in on]
    c.append({"id": "three_sorted_f_over", "set": "three_sorted", "opts": ["-f"], "old": True})
    c.append({"id": "three_sorted_exists", "set": "three_sorted", "opts": [], "old": True})
    c.append({"id": "three_sorted_stdout", "set": "three_sorted", "opts": [], "out": "stdout"})
    c.append({"id": "three_sorted_stdout_u", "set": "three_sorted", "opts": ["-u"], "out": "stdout"})
    for name in ("unsorted_all", "oversize", "residues", "hd_long", "packed", "seventeen", "exact_fill", "incompressible"):
        c.append({"id": name + "_u", "set": name, "opts": ["-u"]})
    c += [{"id": "names_n", "set": "names", "opts": ["-n"]}, {"id": "unsorted_all_n", "set": "unsorted_all", "opts": ["-n"]},
          {"id": "rg_tagged_r", "set": "rg_tagged", "opts": ["-r"]}, {"id": "unsorted_all_r", "set": "unsorted_all", "opts": ["-r"]},
          {"id": "heap_empty_mid_n", "set": "heap_empty_mid", "opts": ["-n"]}, {"id": "heap_empty_mid_r", "set": "heap_empty_mid", "opts": ["-r"]}]
    for h in sorted(bammerge_inputs.header_files()):
        c.append({"id": "two_sorted_" + h, "set": "two_sorted", "opts": ["-h", "h.sam"], "h": h})
    c.append({"id": "two_sorted_h_missing", "set": "two_sorted", "opts": ["-h", "h.sam"]})
    c.append({"id": "more_targets_h_count", "set": "more_targets_later", "opts": ["-h", "h.sam"], "h": "h_match"})
    c.append({"id": "rg_in_subdirectory", "set": "two_sorted", "opts": ["-r"], "args": ["-r", "out.bam", "./in1.bam", "in2.bam"]})
    c.append({"id": "missing_input", "set": "two_sorted", "opts": [], "args": ["out.bam", "in1.bam", "nope.bam"]})
    c.append({"id": "missing_first", "set": "no_eof", "opts": [], "args": ["out.bam", "nope.bam", "in2.bam"]})
    c.append({"id": "two_arguments", "set": "two_sorted", "opts": [], "args": ["out.bam", "in1.bam"], "out": None})
    c.append({"id": "no_arguments", "set": None, "opts": [], "args": [], "out": None})
    for e in c:
        e.setdefault("out", "out.bam")
        e.setdefault("old", False)
        e.setdefault("h", None)
        n = len(sets[e["set"]]) if e["set"] else 0
        e.setdefault("args", e["opts"] + ["-" if e["out"] == "stdout" else "out.bam"] + ["in%d.bam" % (k + 1) for k in range(n)])
    return c


def restate(c, sets, headers):
    """the restatement's (output, stderr, status) of a case with at least three file arguments"""
    files_at = len(c["opts"]) + 1
    given = c["args"][files_at:]
    on_disk = {"in%d.bam" % (k + 1): f for k, f in enumerate(sets[c["set"]])}
    kw = bammerge_ref.options(c["opts"])
    if "h_name" in kw:
        kw["h_text"] = headers[c["h"]].encode() if c["h"] else None
    if c["old"] and "-f" not in c["opts"]:
        return OLD, bammerge_ref.MSG_EXISTS % "out.bam", 1
    return bammerge_ref.merge([on_disk.get(os.path.basename(g)) for g in given], given, **kw)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    manifest = []
    sets, headers = bammerge_inputs.own_sets(), bammerge_inputs.header_files()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        for c in cases(sets):
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            given = bammerge_inputs.materialize(work, c["set"], sets[c["set"]]) if c["set"] else []
            if c["h"]:
                with open(os.path.join(work, "h.sam"), "w") as fh:
                    fh.write(headers[c["h"]])
                given.append("h.sam")
            if c["old"]:
                with open(os.path.join(work, "out.bam"), "wb") as fh:
                    fh.write(OLD)
            why = None
            try:
                p = subprocess.run([exe] + c["args"], cwd=work, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT)
                rc, err, out = p.returncode, p.stderr.decode("latin-1"), p.stdout
                if rc < 0:
                    why = "the reference ends with signal %d" % -rc
            except subprocess.TimeoutExpired:
                rc, err, out = None, "", b""
                why = "the reference runs past %d s" % TIME_LIMIT
            listing = sorted(fn for fn in os.listdir(work) if fn not in given)
            got = None
            if why is None:
                assert rc in (0, 1), (c["id"], rc)
                if c["out"] == "stdout":
                    got = out
                    assert listing == [], (c["id"], listing)
                else:
                    assert out == b"" and listing in ([], ["out.bam"]), (c["id"], listing)
                    if listing:
                        got = open(os.path.join(work, "out.bam"), "rb").read()
                if len(c["args"]) - len(c["opts"]) >= 3:       # the restatement against the recording
                    want, want_err, want_rc = restate(c, sets, headers)
                    assert want_err == err, (c["id"], want_err, err)
                    assert want_rc == rc, (c["id"], want_rc, rc)
                    assert want == got, (c["id"], None if want is None else len(want), None if got is None else len(got))
                else:
                    assert (rc, err, got) == (1, bammerge_ref.USAGE, None), c["id"]
            else:
                err, rc, listing = "", None, []
            route = "host"
            if why is None and rc == 0 and c["set"]:
                route = bammerge_ref.route(sets[c["set"]], c["opts"])
            e = {"id": c["id"], "set": c["set"], "opts": c["opts"], "args": c["args"], "out": c["out"], "old": c["old"], "h": c["h"], "rc": rc, "stderr": err,
                 "listing": listing, "expect": "refuse" if why else "same", "why": why, "route": route, "bam": None}
            if got is not None:
                e["bam"] = {"size": len(got), "sha256": hashlib.sha256(got).hexdigest(),
                            "b64": base64.b64encode(got).decode() if len(got) <= INLINE_LIMIT else None}
            manifest.append(e)
            print("%-28s rc %5s  %-6s %-6s %8s bytes  %s" % (c["id"], rc, e["expect"], e["route"], "-" if got is None else len(got),
                                                           (why or err.strip().replace("\n", " | "))[:100]))
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "headers": %s,\n "cases": [\n' % (json.dumps(bammerge_inputs.digests(), sort_keys=True),
                                                                   json.dumps({k: hashlib.sha256(v.encode()).hexdigest() for k, v in headers.items()}, sort_keys=True)))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
