#!/usr/bin/env python3
"""Records what the reference's map_kseq does: tests/golden/kseq/manifest.json.

Run where the reference tree is checked out (argument or $HPN_REFERENCE, default /root/reference).  map_kseq.cpp is compiled into
a TEMPORARY directory and run on the cases below, each in a directory of its own under a limit of 5 s.  Output bytes, stderr and
exit status are stored as data.  No reference text is stored and nothing compiled stays.  Outputs of up to 2 KiB are kept in the
manifest (bytes as the code points 0 .. 255), larger ones as length + SHA-256 only.  The inputs that are not files of
tests/golden/fastq/ come from tests/kseq_inputs.py (fixed seeds) and are NOT stored: the manifest holds their SHA-256, and the
tests make them again and check it.  Re-running reproduces the file byte for byte.

kbtree_kseq.c is tried too -- and does not compile against the klib copy that lies beside it (it uses kb_itr_first / kbitr_t,
which that kbtree.h does not have; the manifest's "kbtree_builds" records what happened).  Its cases therefore carry what its
source fixes: with sequences of ONE length its B-tree is a set in strcmp order and its output is map_kseq's recorded run of the
same input, byte for byte ("same"); with more than one length what the tree holds is an artefact of an unparenthesised ?: in
its comparison, and the tool here refuses ("refuse").  Where it does compile, its runs on the one-length cases are held against
map_kseq's right here.

What a case expects of the tool ("expect"), with the reason in "why", and the route the input must take ("route": "device" or
"host", decided from the input alone by tests/kseq_ref.py):
  same     the reference finished with status 0: its stdout, stderr and status are the tool's.
  refuse   "damaged stream": the gzip stream fails its CRC-32 / ISIZE check, which the reference never looks at; "NUL byte": the
           reference's "%s" cuts the line there; "mixed lengths": kbtree_kseq, above.  Status 2, nothing on stdout.
  usage    no argument: the reference dereferences NULL; the tool prints its own usage, status 1.
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kseq_inputs  # noqa: E402  (tests/kseq_inputs.py)
import kseq_ref  # noqa: E402

OUT = os.path.join(HERE, "kseq")
INLINE_LIMIT = 2 << 10
TIME_LIMIT = 5
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_uniq.py's list
OWN = "kseq/inputs/"
BTREE = ["fq_one_length.fq", "fq_run_300.fq", "fq_all_equal.fq", "fq_all_distinct.fq", "fa_one_length.fa", "fq_n256.fq", "fa_n17.fa", "fq_keys.fq",
         "fa_w60.fa", "fq_wrapped.fq", "fa_crlf.fa"]


def build(ref, tmp, src, cc, exe):
    p = subprocess.run([cc, "-O2", "-w", "-I", ref, os.path.join(ref, src), "-o", os.path.join(tmp, exe), "-lz"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    return os.path.join(tmp, exe) if p.returncode == 0 else None


def cases():
    c = []

    def add(cid, inp, tool="map_kseq", stdin=None):
        c.append({"id": cid, "in": inp, "tool": tool, "stdin": stdin})

    for f in FASTQ:
        add("g_" + f.replace(".", "_"), "fastq/" + f)
    for name in sorted(list(kseq_inputs.own_inputs()) + list(kseq_inputs.gz_inputs())):
        add("f_" + name.replace(".", "_"), OWN + name)
    for name in BTREE:
        add("b_" + name.replace(".", "_"), OWN + name, "kbtree_kseq")
    add("stdin_dash_fq", OWN + "fq_keys.fq", stdin="-")
    add("stdin_empty_name_fa", OWN + "fa_w60.fa", stdin="")
    add("stdin_gz", OWN + "fq_keys.fq.gz", stdin="-")
    add("stdin_btree", OWN + "fq_one_length.fq", "kbtree_kseq", stdin="-")
    add("missing_file", None)
    add("no_arguments", None)
    add("no_arguments_btree", None, "kbtree_kseq")
    return c


def blob(text):
    o = {"size": len(text), "sha256": hashlib.sha256(text).hexdigest(), "text": None}
    if len(text) <= INLINE_LIMIT:
        o["text"] = text.decode("latin-1")   # (bytes as code points 0 .. 255)
    return o


def inflate(raw, is_gz):
    """the stream the reference's gzread delivers, or None for a damaged one"""
    if not is_gz:
        return raw
    try:
        return gzip.decompress(raw)
    except (zlib.error, gzip.BadGzipFile, EOFError):
        return None


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HPN_REFERENCE", "/root/reference")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest, runs = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = {"map_kseq": build(ref, tmp, "map_kseq.cpp", "g++", "map_kseq_ref"), "kbtree_kseq": build(ref, tmp, "kbtree_kseq.c", "gcc", "kbtree_kseq_ref")}
        assert exe["map_kseq"]
        made = os.path.join(tmp, "inputs")
        os.makedirs(made)
        digests = kseq_inputs.materialize(made)
        where = lambda rel: os.path.join(made, rel[len(OWN):]) if rel.startswith(OWN) else os.path.join(HERE, rel)

        def run(tool, path, stdin, work):
            argv = [exe[tool]] + ([] if path is None and stdin is None else [stdin if stdin is not None else path])
            p = subprocess.run(argv, cwd=work, stdin=open(path, "rb") if stdin is not None else subprocess.DEVNULL, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=TIME_LIMIT)
            return p.returncode, p.stdout, p.stderr

        for c in cases():
            work = os.path.join(tmp, "run_" + c["id"])
            os.makedirs(work)
            entry = {"id": c["id"], "in": c["in"], "tool": c["tool"], "stdin": c["stdin"], "rc": None, "expect": None, "why": None, "route": None,
                     "in_sha256": None, "stdout": None, "stderr": ""}
            if c["in"] is None and c["id"].startswith("no_arguments"):
                entry["expect"], entry["rc"], entry["why"] = "usage", 1, "the reference dereferences NULL"
                manifest.append(entry)
                continue
            path = where(c["in"]) if c["in"] else os.path.join(work, "no_such_file.fa")
            raw = open(path, "rb").read() if c["in"] else b""
            text = inflate(raw, bool(c["in"]) and c["in"].endswith(".gz"))
            entry["in_sha256"] = hashlib.sha256(raw).hexdigest() if c["in"] else None
            if text is None:
                entry["expect"], entry["rc"], entry["why"] = "refuse", 2, "damaged stream"
            elif b"\0" in text:
                entry["expect"], entry["rc"], entry["why"] = "refuse", 2, "NUL byte"
            elif c["tool"] == "kbtree_kseq" and len(kseq_ref.lengths(text)) > 1:
                entry["expect"], entry["rc"], entry["why"] = "refuse", 2, "mixed lengths"
            else:
                entry["route"] = kseq_ref.route(text)
                if c["tool"] == "map_kseq":
                    rc, out, err = run("map_kseq", path, c["stdin"], work)
                    runs[(c["in"], c["stdin"])] = (out, err)
                else:
                    rc, (out, err) = 0, runs[(c["in"], None)]      # one length: map_kseq's run of the same input
                    entry["why"] = "one length: map_kseq's recorded run"
                    if exe["kbtree_kseq"]:
                        assert run("kbtree_kseq", path, c["stdin"], work) == (0, out, err), c["id"]
                assert rc == 0, (c["id"], rc)
                entry["expect"], entry["rc"] = "same", 0
                entry["stdout"], entry["stderr"] = blob(out), err.decode("latin-1")
                assert (out, err) == kseq_ref.map_kseq(text), c["id"]      # (the restatement, held to the run right here)
            manifest.append(entry)
            print("%-30s %-11s rc %s  %-7s %-7s %-16s stdout:%s" % (c["id"], c["tool"], entry["rc"], entry["expect"], entry["route"], entry["why"],
                                                                   entry["stdout"]["size"] if entry["stdout"] else None))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        f.write('{"inputs": %s,\n "kbtree_builds": %s,\n "cases": [\n' % (json.dumps(digests, sort_keys=True), json.dumps(bool(exe["kbtree_kseq"]))))
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in manifest))
        f.write("\n ]}\n")
    print("%d cases, %d bytes in %s" % (len(manifest), os.path.getsize(os.path.join(OUT, "manifest.json")), OUT))


if __name__ == "__main__":
    main()
