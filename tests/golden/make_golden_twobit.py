#!/usr/bin/env python3
"""Records what the reference's 2-bit pair does: tests/golden/twobit/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  Both tools are compiled into
a TEMPORARY directory -- fastq2twobit.c with list.c and hiredis/sds.c, twoBit2seq.c with hiredis/sds.c -- and run on the cases
below, each in a directory of its own under a limit of 5 s (and of 64 MiB per file written: twoBit2seq on a header whose packedLen
is 0 prints newlines without end).  Output bytes, stderr (the run times masked) and exit status or signal are stored as data.  No
reference text is stored and nothing compiled stays.  Outputs of up to 2 KiB are kept in the manifest (bytes as the code points
0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of tests/golden/fastq/ come from
tests/twobit_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the tests make them again and
check it.  A twoBit2seq case with "from" reads the OUTPUT of that fastq2twobit case (a round trip).  Re-running reproduces the
file byte for byte.

What a case expects of the tool here ("expect"):
  same     the reference finished with status 0: its bytes, stderr and status are the tool's.
  refuse   the reference crashed (signal), never ended (the limits above: "endless"), or its result is undefined by construction
           ("constructed": a sequence byte >= 0x80 indexes its table with a negative number -- nothing of its run is kept):
           status 2.
  usage    no argument, -h, or an unknown option: usage on stderr, status 1 (the usage text is the tool's own).
"""
import hashlib
import json
import os
import re
import resource
import shutil
import signal
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import twobit_inputs  # noqa: E402  (tests/twobit_inputs.py)

OUT = os.path.join(HERE, "twobit")
INLINE_LIMIT = 2 << 10
TIME_LIMIT, FILE_LIMIT = 5, 64 << 20
TIMES = re.compile(rb"at \d+\.\d{3} s")
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_uniq.py's list
OWN = "twobit/inputs/"


def build_reference(ref, tmp):
    inc = ["-I", ref, "-I", os.path.join(ref, "hiredis")]
    sds = os.path.join(ref, "hiredis", "sds.c")
    pack, unpack = os.path.join(tmp, "fastq2twobit_ref"), os.path.join(tmp, "twoBit2seq_ref")
    subprocess.check_call(["gcc", "-O2", "-w"] + inc + [os.path.join(ref, "fastq2twobit.c"), os.path.join(ref, "list.c"), sds, "-o", pack, "-lz"])
    subprocess.check_call(["gcc", "-O2", "-w"] + inc + [os.path.join(ref, "twoBit2seq.c"), sds, "-o", unpack, "-lz"])
    return {"pack": pack, "unpack": unpack}


def cases():
    c = []

    def add(tool, cid, inp, args=None, stdin=None, constructed=False, source=None):
        """args: the command line behind the program's name; "{in}" stands for the input's path.  stdin: None or "file" (the input
        is the process's standard input).  source: the pack case whose output is this unpack case's input."""
        c.append({"tool": tool, "id": cid, "in": inp, "from": source, "args": ["-i", "{in}", "-o", "o"] if args is None else args, "stdin": stdin,
                  "constructed": constructed})

    # ---- fastq2twobit
    for f in FASTQ:
        add("pack", "p_" + f.replace(".", "_"), "fastq/" + f)
    for n in twobit_inputs.PACK_LENGTHS:
        add("pack", "p_len%d" % n, OWN + "len%d.fq" % n)
    for name in ("all_lengths", "mixed", "mixed_last150", "letters", "crlf", "nonl", "example", "plain12"):
        add("pack", "p_" + name, OWN + name + ".fq")
    for name in ("hi_last", "hi_first", "hi_mid"):
        add("pack", "p_" + name, OWN + name + ".fq", constructed=True)
    add("pack", "p_opt_n", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-n"])
    add("pack", "p_opt_s_n", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-s", "-n"])
    add("pack", "p_opt_n_s", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-n", "-s"])
    add("pack", "p_o_twice", OWN + "plain12.fq", ["-o", "a", "-i", "{in}", "-o", "b"])
    add("pack", "p_no_o", OWN + "example.fq", ["-i", "{in}"])
    add("pack", "p_o_dash", OWN + "example.fq", ["-i", "{in}", "-o", "-x", "-n"])
    add("pack", "p_opt_r", OWN + "plain12.fq", ["-i", "{in}", "-o", "o", "-r", "5"])
    add("pack", "p_stdin_file", OWN + "mixed_last150.fq", ["-o", "o"], "file")
    add("pack", "p_stdin_gz", "fastq/t.fq.gz", ["-i", "-", "-o", "o"], "file")
    add("pack", "p_missing_file", None, ["-i", "no_such_file.fq", "-o", "o"])
    add("pack", "p_no_arguments", None, [])
    add("pack", "p_help", None, ["-h"])
    # ---- twoBit2seq
    for s in twobit_inputs.UNPACK_SEQLENS:
        add("unpack", "u_seqlen%d" % s, OWN + "u%d.2bit" % s)
    names = sorted(n[:-5] for n in twobit_inputs.own_inputs() if n.endswith(".2bit") and not (n[0] == "u" and n[1:-5].isdigit()))
    for name in names:
        add("unpack", "u_" + name, OWN + name + ".2bit")
    add("unpack", "u_opt_c", OWN + "n17.2bit", ["-i", "{in}", "-o", "o", "-c", "9"])
    add("unpack", "u_o_dash", OWN + "n2.2bit", ["-i", "{in}", "-o", "-"])
    add("unpack", "u_no_o", OWN + "n2.2bit", ["-i", "{in}"])
    add("unpack", "u_o_twice", OWN + "n2.2bit", ["-o", "a", "-i", "{in}", "-o", "b"])
    add("unpack", "u_stdin_file", OWN + "partial.2bit", ["-o", "o"], "file")
    add("unpack", "u_opt_z", OWN + "n2.2bit", ["-i", "{in}", "-o", "o", "-z"])
    add("unpack", "u_missing_file", None, ["-i", "no_such_file.2bit", "-o", "o"])
    add("unpack", "u_no_arguments", None, [])
    add("unpack", "u_help", None, ["-h"])
    for p in [x for x in c if x["tool"] == "pack" and x["in"] and not x["constructed"] and x["args"] == ["-i", "{in}", "-o", "o"]]:
        add("unpack", "rt_" + p["id"][2:], None, source=p["id"])
    return c


def blob(text):
    o = {"size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None}
    if text and len(text) <= INLINE_LIMIT:
        o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
    return o


def limits():
    resource.setrlimit(resource.RLIMIT_FSIZE, (FILE_LIMIT, FILE_LIMIT))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest, packed = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = twobit_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len(OWN):]) if rel.startswith(OWN) else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            if c["from"]:
                if packed.get(c["from"]) is None:
                    continue      # (the pack case has no answer: nothing to unpack)
                path = os.path.join(tmp, c["id"] + ".2bit")
                open(path, "wb").write(packed[c["from"]])
            else:
                path = where(c["in"]) if c["in"] else None
            raw = open(path, "rb").read() if path else b""
            cmd = [exe[c["tool"]]] + [path if a == "{in}" else a for a in c["args"]]
            out_path, timed_out = os.path.join(tmp, "stdout_" + c["id"]), False
            with open(out_path, "wb") as so:
                try:
                    p = subprocess.run(cmd, cwd=work, stdin=open(path, "rb") if c["stdin"] == "file" else subprocess.DEVNULL, stdout=so, stderr=subprocess.PIPE,
                                       env={**os.environ, "MALLOC_CHECK_": "0"}, timeout=TIME_LIMIT, preexec_fn=limits)
                    rc, stderr = p.returncode, p.stderr
                except subprocess.TimeoutExpired:
                    rc, stderr, timed_out = None, b"", True
            endless = timed_out or rc == -signal.SIGXFSZ
            if endless:      # only where the header says packedLen == 0 and the file has its two bytes
                assert c["tool"] == "unpack" and len(raw) >= 2 and raw[1] == 0, c["id"]
                rc = None
            stdout = open(out_path, "rb").read() if not endless else b""
            os.remove(out_path)
            files = {} if endless else {fn: open(os.path.join(work, fn), "rb").read() for fn in sorted(os.listdir(work))}
            files.pop("no_such_file.fq", None), files.pop("no_such_file.2bit", None)     # (the reference creates a missing input: O_CREAT)
            err = TIMES.sub(b"at T s", stderr)
            if endless:
                expect = "refuse"
            elif rc == 1 and b"Usage" in stderr:
                assert not stdout and not files, c["id"]
                expect = "usage"
            elif c["constructed"]:
                expect, rc = "refuse", None
            elif rc == 0:
                expect = "same"
            else:
                assert rc in (-signal.SIGSEGV, -signal.SIGABRT, -signal.SIGBUS), (c["id"], rc)
                expect = "refuse"
            entry = {"tool": c["tool"], "id": c["id"], "in": c["in"], "from": c["from"], "args": c["args"], "stdin": c["stdin"], "rc": rc,
                     "constructed": c["constructed"], "endless": endless, "expect": expect, "in_sha256": hashlib.sha256(raw).hexdigest() if path else None,
                     "stderr": err.decode("latin-1") if expect == "same" else "", "stdout": None, "outputs": []}
            if expect == "same":
                assert len(files) <= 1 and (not files or stdout == b""), c["id"]
                entry["stdout"] = blob(stdout)
                entry["outputs"] = [dict(blob(text), name=fn) for fn, text in files.items()]
                if c["tool"] == "pack":
                    packed[c["id"]] = stdout if not files else next(iter(files.values()))
            manifest.append(entry)
            print("%-26s rc %5s  %-7s %s" % (c["id"], rc, expect, " ".join("%s:%d" % (k, len(v)) for k, v in files.items())))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
