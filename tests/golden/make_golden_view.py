#!/usr/bin/env python3
"""Records what the reference's `samtools view` does: tests/golden/view/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  libbam is compiled from the
samtools-0.1.19 tarball the reference vendors, with the sources and flags of tests/golden/make_golden_bai.py, into a TEMPORARY
directory, sam_view.c of the same tarball beside it, and both are linked to a driver of our own that calls main_samview with
argv[0] = "view" -- the function behind `samtools view`.  Every case runs in a directory of its own under a limit of 20 s with its
input written there as in.bam.  Status, stderr, stdout, the -o file, the directory's listing afterwards are stored as data (size
+ SHA-256; whole, base64, up to 512 bytes).  No reference text is stored and nothing compiled stays.  The inputs come from
tests/view_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256.

"expect" is `same` for every case the reference finishes inside its own memory; `refuse` for what the tool leaves out (regions,
SAM input, -L, -B: not run at all) and where the reference reads memory that is not its own (UNDEFINED below).  Before anything
is written the sequential restatement tests/view_ref.py is held to every finished run, and `-b -@ 4` is held to `-b` on every
input: the threads change no byte."""
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
import make_golden_bai  # noqa: E402  (the recipe: sources, flags)
import view_inputs  # noqa: E402  (tests/view_inputs.py)
import view_ref  # noqa: E402

OUT = os.path.join(HERE, "view")
INLINE_LIMIT = 512
TIME_LIMIT = 20
DRIVER = ('int main_samview(int argc, char *argv[]);\nint main(int argc, char *argv[])\n{\n    argv[0] = "view";\n    return main_samview(argc, argv);\n}\n')
UNDEFINED = {"tid_beyond_header": "target_name is read past its end (refID 3 of 3 targets)",
             "mtid_beyond_header": "target_name is read past its end (mate refID 7 of 3 targets)"}
DAMAGED = ("truncated_mid_block", "truncated_mid_record", "no_eof")
RG_LIST = b"a2\nb1 zz\n"
SEEDS = (7, 11)


def build_reference(ref, tmp):
    make_golden_bai.build_reference(ref, tmp)          # libbam.a under tmp/samtools-0.1.19
    sam = os.path.join(tmp, "samtools-0.1.19")
    subprocess.check_call(["gcc", "-c", "-g", "-O2", "-w"] + make_golden_bai.SAM_DFLAGS + ["-I.", "sam_view.c", "-o", "sam_view.o"], cwd=sam)
    drv = os.path.join(tmp, "view_driver.c")
    with open(drv, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "view")
    subprocess.check_call(["gcc", "-O2", "-w", drv, os.path.join(sam, "sam_view.o"), "-o", exe, "-L", sam, "-lbam", "-lpthread", "-lm", "-lz"])
    return exe


def cases(inputs):
    """id, input (None: no input is written), args, stdin (the input comes through a pipe), files (others the arguments name)"""
    c = []
    add = lambda cid, inp, args, **kw: c.append(dict({"id": cid, "input": inp, "args": args}, **kw))
    for n in sorted(inputs):
        if n in UNDEFINED:
            continue
        add(n + "_text", n, ["in.bam"])
        add(n + "_b", n, ["-b", "-o", "out.bam", "in.bam"])
        add(n + "_c", n, ["-c", "in.bam"])
    for n in sorted(UNDEFINED):
        add(n + "_text", n, ["in.bam"])
        add(n + "_b", n, ["-b", "-o", "out.bam", "in.bam"])        # (BAM output and the count do not look the names up)
        add(n + "_c", n, ["-c", "in.bam"])
    # numbers, lengths, aux: the flag styles and the filters that read the record's inside
    for n in ("numbers", "lengths", "aux_all", "aux_float"):
        add(n + "_x", n, ["-x", "in.bam"])
        add(n + "_X", n, ["-X", "in.bam"])
    add("numbers_m", "numbers", ["-m", "100", "in.bam"])
    add("numbers_q", "numbers", ["-q", "100", "-c", "in.bam"])
    add("lengths_Q", "lengths", ["-Q", "2", "in.bam"])
    add("lengths_Q_b", "lengths", ["-Q", "3", "-b", "-o", "out.bam", "in.bam"])
    add("aux_float_b_Q", "aux_float", ["-Q", "2", "-u", "-o", "out.bam", "in.bam"])
    add("name_nul_inside_s", "name_nul_inside", ["-s", "0.5", "-c", "in.bam"])
    # read groups
    for cid, args in (("rg_r", ["-r", "a1"]), ("rg_r_unknown", ["-r", "nope"]), ("rg_l", ["-l", "libA"]), ("rg_l_b", ["-l", "libB", "-b", "-o", "out.bam"]),
                      ("rg_r_l", ["-r", "b1", "-l", "libA"]), ("rg_R", ["-R", "list.txt"]), ("rg_R_h", ["-R", "list.txt", "-h"]),
                      ("rg_R_b", ["-R", "list.txt", "-b", "-o", "out.bam"]), ("rg_l_c", ["-l", "libA", "-c"])):
        add(cid, "rg", args + ["in.bam"], files={"list.txt": RG_LIST} if "-R" in args else {})
    for cid, args in (("rg_R_l", ["-R", "list.txt", "-l", "libB"]), ("rg_clean_l", ["-l", "libA"]), ("rg_clean_l_b", ["-l", "libB", "-b", "-o", "out.bam"]),
                      ("rg_clean_r_l", ["-r", "b1", "-l", "libA"]), ("rg_clean_R_l", ["-R", "list.txt", "-l", "libA", "-h"]), ("rg_clean_l_c", ["-l", "libA", "-c"]),
                      ("rg_clean_l_none", ["-l", "nolib", "-c"]), ("rg_clean_R", ["-R", "list.txt", "-F", "0x400"])):
        add(cid, "rg" if cid == "rg_R_l" else "rg_clean", args + ["in.bam"], files={"list.txt": RG_LIST} if "-R" in args else {})
    # subsampling
    for k, s in enumerate(["0.5", "0.000001", "1.0", "0.9999999", "7.25", "7", "x", "11.5", "0.3333333"]):
        add("subsample_s%d" % k, "subsample", ["-s", s, "in.bam"])
        add("subsample_s%d_c" % k, "subsample", ["-s", s, "-c", "in.bam"])
    add("mixed_s_b", "mixed", ["-s", "7.25", "-b", "-o", "out.bam", "in.bam"])
    # keep patterns against the scan's tile
    add("runs_F", "runs", ["-F", "0x400", "in.bam"])
    add("runs_f", "runs", ["-f", "0x400", "-b", "-o", "out.bam", "in.bam"])
    add("runs_none", "runs", ["-f", "0x800", "in.bam"])
    add("runs_none_b", "runs", ["-f", "0x800", "-b", "-o", "out.bam", "in.bam"])
    add("runs_F_c", "runs", ["-F", "0x400", "-c", "in.bam"])
    add("last_only_F", "last_only", ["-F", "0x400", "in.bam"])
    add("last_only_F_b", "last_only", ["-F", "0x400", "-b", "-o", "out.bam", "in.bam"])
    # the writer's cuts
    for n in ("cuts_exact", "cuts_less", "cuts_more"):
        for lv in ("-b", "-u", "-1"):
            add("%s_F%s" % (n, lv), n, ["-F", "0x400", lv, "-o", "out.bam", "in.bam"])
        add(n + "_Q", n, ["-F", "0x400", "-Q", "2", "-b", "-o", "out.bam", "in.bam"])
    # mixed: every option, combinations, pipes
    add("mixed_fFqm", "mixed", ["-f", "0x1", "-F", "0x404", "-q", "20", "-m", "50", "in.bam"])
    add("mixed_fFqm_c", "mixed", ["-f", "0x1", "-F", "0x404", "-q", "20", "-m", "50", "-c", "in.bam"])
    add("mixed_fFqm_b", "mixed", ["-f", "0x1", "-F", "0x404", "-q", "20", "-m", "50", "-b", "-o", "out.bam", "in.bam"])
    add("mixed_h", "mixed", ["-h", "in.bam"])
    add("mixed_H", "mixed", ["-H", "in.bam"])
    add("mixed_bH", "mixed", ["-b", "-H", "-o", "out.bam", "in.bam"])
    add("mixed_cH", "mixed", ["-c", "-H", "in.bam"])
    add("mixed_xh", "mixed", ["-x", "-h", "-F", "0x400", "in.bam"])
    add("mixed_X_o", "mixed", ["-X", "-o", "out.sam", "in.bam"])
    add("mixed_u", "mixed", ["-u", "-o", "out.bam", "in.bam"])
    add("mixed_1", "mixed", ["-1", "-o", "out.bam", "in.bam"])
    add("mixed_Q", "mixed", ["-Q", "2", "-q", "10", "in.bam"])
    add("mixed_c_o", "mixed", ["-c", "-o", "out.txt", "in.bam"])
    add("mixed_threads", "mixed", ["-b", "-@", "4", "-o", "out.bam", "in.bam"])
    add("mixed_octal", "mixed", ["-f", "0100", "-F", "1024", "-c", "in.bam"])
    add("mixed_stdin", "mixed", ["-F", "0x400", "-"], stdin=True)
    add("mixed_stdin_c", "mixed", ["-c", "-"], stdin=True)
    add("mixed_b_stdout", "mixed", ["-b", "-F", "0x400", "in.bam"])
    add("mixed_pipe", "mixed", ["-u", "-q", "30", "-"], stdin=True)
    add("hdr_no_sq_h", "hdr_no_sq", ["-h", "in.bam"])
    add("hdr_mismatch_h", "hdr_mismatch", ["-h", "in.bam"])
    add("hdr_mismatch_H", "hdr_mismatch", ["-H", "in.bam"])
    for n in DAMAGED:
        add(n + "_h", n, ["-h", "-F", "0x400", "in.bam"])
    # the tool itself
    add("no_arguments", None, [])
    add("long_help", None, ["-?"])
    add("unknown_option", None, ["-z"])
    add("unknown_option_file", "lengths", ["-z", "-c", "in.bam"])
    add("missing_argument", None, ["-q"])
    add("only_options", None, ["-b", "-h"])
    add("missing_input", None, ["nope.bam"])
    add("missing_input_c", None, ["-c", "nope.bam"])
    # refused: not run
    add("region", "mixed", ["in.bam", "c0:1-100"], skip="regions are outside the tool's scope")
    for opt, arg in (("-S", None), ("-t", "list.txt"), ("-T", "ref.fa"), ("-L", "x.bed"), ("-B", None)):
        add("option_" + opt[1], "mixed", [opt] + ([arg] if arg else []) + ["in.bam"], skip="%s is outside the tool's scope" % opt)
    for e in c:
        e.setdefault("stdin", False)
        e.setdefault("files", {})
        e.setdefault("skip", None)
    return c


def blob(b):
    if b is None:
        return None
    return {"size": len(b), "sha256": hashlib.sha256(b).hexdigest(), "b64": base64.b64encode(b).decode() if len(b) <= INLINE_LIMIT else None}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    manifest = []
    inputs = view_inputs.inputs()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)

        def run(cid, data, args, stdin, files):
            work = os.path.join(tmp, "run_" + cid)
            os.makedirs(work)
            given = []
            if data is not None and not stdin:
                given.append(view_inputs.materialize(work, cid, data))
            for fn, b in files.items():
                with open(os.path.join(work, fn), "wb") as fh:
                    fh.write(b)
                given.append(fn)
            feed = {"input": data} if stdin else {"stdin": subprocess.DEVNULL}
            try:
                p = subprocess.run([exe] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIME_LIMIT, **feed)
            except subprocess.TimeoutExpired:
                return None, "", b"", [], None, "the reference runs past %d s" % TIME_LIMIT
            listing = sorted(fn for fn in os.listdir(work) if fn not in given)
            made = open(os.path.join(work, listing[0]), "rb").read() if len(listing) == 1 else None
            return p.returncode, p.stderr.decode("latin-1"), p.stdout, listing, made, ("the reference ends with signal %d" % -p.returncode if p.returncode < 0 else None)

        # -@: the threads change no byte of a BAM output
        for n in sorted(inputs):
            if n in UNDEFINED or n in DAMAGED or n.startswith("truncated"):
                continue
            a = run("thr0_" + n, inputs[n], ["-b", "-o", "out.bam", "in.bam"], False, {})
            b = run("thr4_" + n, inputs[n], ["-b", "-@", "4", "-o", "out.bam", "in.bam"], False, {})
            assert a[0] == b[0] == 0 and a[4] == b[4] and a[1] == b[1], ("-@ changes the output", n)
        for c in cases(inputs):
            data = inputs[c["input"]] if c["input"] else None
            text_out = not any(a in c["args"] for a in ("-b", "-u", "-1", "-c")) and "-bH" not in c["args"]
            why = c["skip"] or (UNDEFINED.get(c["input"]) if text_out else None)
            rc, err, out, listing, made = None, "", b"", [], None
            if not c["skip"]:
                rc, err, out, listing, made, crashed = run(c["id"], data, c["args"], c["stdin"], c["files"])
                why = why or crashed
            route = "host"
            if why is None:
                assert rc in (0, 1) and len(listing) <= 1, (c["id"], rc, listing)
                w_out, w_file, w_err, w_rc = view_ref.view(data, c["args"], c["files"], c["stdin"])      # the restatement against the recording
                assert w_rc == rc, (c["id"], w_rc, rc, err)
                assert w_err == err, (c["id"], w_err, err)
                assert w_out == out, (c["id"], len(w_out), len(out), w_out[:300], out[:300])
                assert w_file == made, (c["id"], None if w_file is None else len(w_file), None if made is None else len(made))
                if c["input"]:
                    route = view_ref.route(data, c["args"], c["stdin"], c["files"])
            else:
                rc, err, out, listing, made = None, "", b"", [], None
            e = {"id": c["id"], "input": c["input"], "args": c["args"], "stdin": c["stdin"], "files": {k: v.decode() for k, v in c["files"].items()}, "rc": rc,
                 "stderr": err, "listing": listing, "expect": "refuse" if why else "same", "why": why, "route": route, "stdout": blob(out if why is None else None),
                 "file": blob(made)}
            manifest.append(e)
            print("%-26s rc %5s  %-6s %-9s %8d out %8s file  %s" % (c["id"], rc, e["expect"], e["route"], len(out), "-" if made is None else len(made),
                                                                   (why or err.strip().replace("\n", " | "))[:90]))
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    rand = {str(s): view_ref.libc_rand(s) for s in SEEDS}
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "rand": %s,\n "threads_change_nothing": true,\n "cases": [\n' % (json.dumps(view_inputs.digests(), sort_keys=True), json.dumps(rand)))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
