#!/usr/bin/env python3
"""Records what the reference gzfastq_sort does: tests/golden/sort/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  The reference tool is
compiled into a TEMPORARY directory, run on the cases below, and its outputs, stderr (the run times masked) and exit status
or signal are stored as data.  No reference text is stored.  Outputs of up to 2 KiB are kept in the manifest (bytes as the
code points 0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of tests/golden/fastq/ come from
tests/sort_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the tests make them again and
check it.  Re-running reproduces the file byte for byte.

What a case expects of the tool here ("expect"):
  same     the reference finished: output bytes (file or stdout), stderr and status are the tool's.  For every such case whose
           input the restatement frames, the recorder ASSERTS that the reference's output is the stable order
           (length, bytes, input ordinal) of tests/sort_ref.py.
  usage    the usage text on stderr, status 1 (only status and the word "Usage" are held: the text names the program).
  refuse   the reference has no answer (it was killed by a signal, or gzgets split a line of 1023+ characters and the records
           behind it are made of the wrong lines): the tool leaves with status 2 and one line.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sort_inputs  # noqa: E402  (tests/sort_inputs.py)
import sort_ref     # noqa: E402

OUT = os.path.join(HERE, "sort")
INLINE_LIMIT = 2 << 10
TIMES = re.compile(rb"at \d+\.\d{3} s")
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "gzfastq_sort_ref")
    subprocess.check_call(["gcc", "-O2", "-w", "-I", ref, os.path.join(ref, "gzfastq_sort.c"), "-o", exe, "-lz"])
    return exe


def cases():
    c = []

    def add(cid, inp, args, stdin=None):
        """args: the command line behind the program's name; "{in}" stands for the input's path.  stdin: None, "file" (the
        input is the process's standard input, a regular file) or "pipe"."""
        c.append({"id": cid, "in": inp, "args": args, "stdin": stdin})

    for f in FASTQ:
        for mode in ("-s", "-n"):
            add(f.replace(".", "_") + mode, "fastq/" + f, ["-i", "{in}", "-o", "o", mode])
    for name in ("ties40", "dup_names", "edges", "illumina", "hibytes", "small", "crlf", "nonl", "lone_line", "shortq", "nul_bytes", "one",
                 "cut_plus", "cut_seq", "cut_name"):
        for mode in ("-s", "-n"):
            add(name + mode, "sort/inputs/%s.fq" % name, ["-i", "{in}", "-o", "o", mode])
    I = "sort/inputs/"
    add("no_mode", I + "small.fq", ["-i", "{in}", "-o", "o"])
    add("n_then_s", I + "small.fq", ["-i", "{in}", "-o", "o", "-n", "-s"])
    add("s_then_n", I + "small.fq", ["-i", "{in}", "-o", "o", "-s", "-n"])
    add("gz-s", I + "ties40.fq.gz", ["-i", "{in}", "-o", "o", "-s"])
    add("gz-n", I + "ties40.fq.gz", ["-i", "{in}", "-o", "o", "-n"])
    add("gz_small", I + "small.fq.gz", ["-i", "{in}", "-o", "o", "-n"])
    add("no_dash_o", I + "small.fq", ["-i", "{in}", "-n"])
    add("dash_o_dash", I + "small.fq", ["-i", "{in}", "-o", "-x", "-s"])
    add("r_exact", I + "small.fq", ["-i", "{in}", "-o", "o", "-n", "-r", "12"])
    add("r_larger", I + "small.fq", ["-i", "{in}", "-o", "o", "-s", "-r", "1000"])
    add("r_digits_then_text", I + "small.fq", ["-i", "{in}", "-o", "o", "-s", "-r", "20x"])
    add("r_zero", I + "small.fq", ["-i", "{in}", "-o", "o", "-s", "-r", "0"])
    add("r_text", I + "small.fq", ["-i", "{in}", "-o", "o", "-s", "-r", "many"])
    add("r_smaller", I + "ties40.fq", ["-i", "{in}", "-o", "o", "-s", "-r", "10"])
    add("r_negative", I + "small.fq", ["-i", "{in}", "-o", "o", "-s", "-r", "-3"])
    add("stdin_file", I + "ties40.fq", ["-o", "o", "-n"], "file")
    add("stdin_file_dash", I + "small.fq", ["-i", "-", "-o", "o", "-s"], "file")
    add("stdin_file_gz", I + "small.fq.gz", ["-o", "o", "-s"], "file")
    add("stdin_file_r", I + "small.fq", ["-o", "o", "-s", "-r", "12"], "file")
    add("pipe", I + "small.fq", ["-o", "o", "-s"], "pipe")
    add("pipe_r", I + "ties40.fq", ["-o", "o", "-n", "-r", "3000"], "pipe")
    add("pipe_gz_r", I + "ties40.fq.gz", ["-o", "o", "-s", "-r", "5000"], "pipe")
    add("pipe_r_stdout", I + "small.fq", ["-r", "12", "-n"], "pipe")
    add("pipe_r_smaller", I + "ties40.fq", ["-o", "o", "-s", "-r", "7"], "pipe")
    add("missing_file", None, ["-i", "no_such_file.fq", "-o", "o", "-s"])
    add("usage_none", None, [])
    add("usage_h", None, ["-h"])
    add("usage_unknown", None, ["-i", "x", "-Z"])
    return c


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = []
    import gzip
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = sort_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len("sort/inputs/"):]) if rel.startswith("sort/inputs/") else os.path.join(HERE, rel)
        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            path = where(c["in"]) if c["in"] else None
            cmd = [exe] + [path if a == "{in}" else a for a in c["args"]]
            raw = open(path, "rb").read() if path else b""
            kw = {}
            if c["stdin"] == "file":
                kw["stdin"] = open(path, "rb")
            elif c["stdin"] == "pipe":
                kw["input"] = raw
            else:
                kw["stdin"] = subprocess.DEVNULL
            p = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={**os.environ, "MALLOC_CHECK_": "0"}, **kw)
            err = TIMES.sub(b"at T s", p.stderr)
            files = {fn: open(os.path.join(work, fn), "rb").read() for fn in sorted(os.listdir(work))}
            files.pop("no_such_file.fq", None)     # (the reference creates a missing input: O_CREAT)
            assert p.returncode in (0, 1, -6, -11), (c["id"], p.returncode)
            by_name = False
            for a in c["args"]:
                by_name = True if a == "-n" else False if a == "-s" else by_name
            rarg = c["args"][c["args"].index("-r") + 1] if "-r" in c["args"] else None
            framed = None
            if p.returncode == 0:
                try:
                    text = gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw
                    framed = sort_ref.simulate(text, by_name, sort_ref.parse_r(rarg) if rarg else None, c["stdin"] != "pipe", bookkeeping=False)
                except (sort_ref.NoAnswer, OSError, EOFError, Exception) as e:   # a damaged gzip stream, a line gzgets splits
                    framed = None
                    why = "%s: %s" % (type(e).__name__, e)
            if p.returncode == 1 and b"Usage" in p.stderr:
                expect = "usage"
            elif p.returncode == 1:
                expect = "same"      # ("reads count must be a positive integer!")
            elif p.returncode == 0 and framed is not None:
                expect = "same"
                got = p.stdout if not files else files[next(iter(files))]
                assert len(files) <= 1 and (not files or p.stdout == b"")
                # THE finding this recorder exists for: the reference's qsort is stable on these sizes
                assert got == framed[0], (c["id"], "the reference's output is not the stable order")
                assert err.decode("latin-1") == framed[1], (c["id"], err, framed[1])
            else:
                expect = "refuse"
            entry = {"id": c["id"], "in": c["in"], "args": c["args"], "stdin": c["stdin"], "rc": p.returncode, "expect": expect,
                     "by_name": by_name, "stderr": err.decode("latin-1") if expect == "same" else "", "stdout": None, "outputs": []}
            if expect == "refuse" and p.returncode == 0:
                entry["why"] = why
            if expect == "same":
                blobs = [("stdout", p.stdout)] + list(files.items())
                for name, text in blobs:
                    o = {"name": name, "size": len(text), "sha256": hashlib.sha256(text).hexdigest(),
                         "text": text.decode("latin-1") if len(text) <= INLINE_LIMIT else None}
                    if name == "stdout":
                        entry["stdout"] = o
                    else:
                        entry["outputs"].append(o)
            manifest.append(entry)
            print("%-22s rc %4d  %-7s %s" % (c["id"], p.returncode, expect, " ".join("%s:%d" % (k, len(v)) for k, v in files.items())))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "cases": [\n' % json.dumps(digests, sort_keys=True))   # one case per line
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
