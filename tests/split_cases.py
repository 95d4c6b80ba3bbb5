"""What tests/test_split_golden.py and tests/test_split_gpu.py share: the manifest of bamSplitChr's recorded reference runs, the
comparison of one output file with its entry, the Python restatement run on a case, the tool run on a case."""
import base64
import json
import os
import re
import shutil
import subprocess
import zlib

import split_inputs
import split_ref
from conftest import BIN, golden_path

MANIFEST = json.load(open(golden_path("split", "manifest.json")))
CASES = {c["id"]: c for c in MANIFEST["cases"]}
SAME_ZLIB = MANIFEST["zlib"] == zlib.ZLIB_RUNTIME_VERSION
TIMES = re.compile(r"at \d+\.\d{3} s")
TOOL = os.path.join(BIN, "bamSplitChr")
HPN_LINES = []      # the "[hpn] ..." lines of the last run_tool


def stop_on_fault(rc, text):
    """A GPU fault, an abort, a segmentation fault or a time limit ends the whole run: nothing more is started on that device."""
    import pytest
    if rc in (134, 139, 124, 137, -6, -11, -9) or "illegal memory access" in text or "HSA_STATUS_ERROR" in text:
        pytest.exit("the device or a tool faulted (status %s): %s" % (rc, text[-2000:]), returncode=3)


def materialize_checked(directory):
    digests = split_inputs.materialize(directory)
    assert digests == MANIFEST["inputs"], "tests/split_inputs.py no longer makes the inputs the manifest was recorded on"
    return directory


def level_of(args):
    """the reference's option loop: -u x and -1 x set the level, the last one wins"""
    level, k = -1, 0
    while k < len(args) and args[k].startswith("-") and len(args[k]) == 2 and args[k][1] in "owrsu1":
        level = {"-u": 0, "-1": 1}.get(args[k], level)
        k += 2
    return level


def place(case, made, work):
    for k, name in enumerate(case["inputs"]):
        src, dst = split_inputs.path_of(name, made), os.path.join(work, "in.bam" if k == 0 else "in%d.bam" % (k + 1))
        shutil.copyfile(src, dst)
        if case["bai"]:
            shutil.copyfile(src + ".bai", dst + ".bai")
    return set(os.listdir(work))


def check_file(want, data, level, why):
    """one output file against its manifest entry (see the module's docstring for what is always compared)"""
    got = split_ref.describe(data)
    assert got["isize"] == want["isize"], why      # (describe() has checked every block's CRC-32 field against its inflated bytes,
    assert got["inflated_sha256"] == want["inflated_sha256"], why      # which are the reference's: so is every CRC-32)
    assert data[-28:] == split_ref.EOF_BLOCK, why
    if level == 0 or SAME_ZLIB:
        assert got["size"] == want["size"] and got["sha256"] == want["sha256"], why
        if want["b64"] is not None:
            assert data == base64.b64decode(want["b64"]), why
        return True
    return False


def run_model(case, made):
    """split_ref on the case's inputs -> ({name: bytes}, masked stderr)"""
    args, level = case["args"], level_of(case["args"])
    k = 0
    o = None
    while k < len(args) and args[k].startswith("-") and len(args[k]) == 2 and args[k][1] in "owrsu1":
        if args[k] == "-o":
            o = args[k + 1]
        k += 2
    files, err = {}, ""
    for i, (path, name) in enumerate(zip(args[k:], case["inputs"])):
        prefix = o if (i == 0 and o is not None) else path
        bam = split_ref.read(split_inputs.path_of(name, made))
        for target, data, _ in split_ref.split(bam, level):
            files["%s_%s.bam" % (prefix, target)] = data
        err += split_ref.stderr_of(bam, path)
    return files, err


def model_case(cid, name, args, made):
    """a case like the manifest's whose expectation comes from the restatement (inputs with too many outputs to record)"""
    case = {"id": cid, "inputs": [name], "args": args, "bai": True, "rc": 0, "expect": "same", "why": None}
    files, err = run_model(case, made)
    return dict(case, stderr=err, outputs=[dict(split_ref.describe(d), name=fn, b64=None) for fn, d in files.items()])


def run_tool(case, made, work, env_extra, tool=TOOL):
    before = place(case, made, str(work))
    env = {k: v for k, v in os.environ.items() if not k.startswith("HPN_")}
    env.update(env_extra)
    p = subprocess.run([tool] + case["args"], cwd=str(work), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    files = {fn: open(os.path.join(str(work), fn), "rb").read() for fn in sorted(os.listdir(str(work))) if fn not in before}
    stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
    lines = p.stderr.decode("latin-1").splitlines(True)
    HPN_LINES[:] = [ln for ln in lines if ln.startswith("[hpn]")]          # (HPN_TIMING's diagnostics: not the reference's)
    err = TIMES.sub("at T s", "".join(ln for ln in lines if not ln.startswith("[hpn]"))).replace("bamSplitChr:", "PROG:")
    return p.returncode, p.stdout, err, files


def check_tool(case, made, work, env_extra, tool=TOOL):
    """the tool on one recorded case, whatever route env_extra selects"""
    rc, out, err, files = run_tool(case, made, work, env_extra, tool)
    cid = case["id"]
    if case["expect"] == "usage":
        assert rc == 1 and "Usage" in err and not out and not files, cid
        return
    if case["expect"] == "refuse":
        assert rc == 2 and not out and not files, (cid, rc, err, sorted(files))
        why = case["why"].split()
        if why[1] == "record":
            m = re.search(r"record (\d+) \(refID (-?\d+), pos (-?\d+)\)", err)
            assert m and [m.group(1), m.group(2), m.group(3)] == why[2:5], (cid, err)
        else:
            assert "outside the tool's domain" in err, (cid, err)
        return
    assert rc == case["rc"] and not out, (cid, rc, err)
    assert err == case["stderr"], cid
    assert sorted(files) == sorted(o["name"] for o in case["outputs"]), cid
    level = level_of(case["args"])
    model = None
    for o in case["outputs"]:
        if not check_file(o, files[o["name"]], level, (cid, o["name"])):
            model = model or run_model(case, made)[0]
            assert files[o["name"]] == model[o["name"]], (cid, o["name"])     # this machine's zlib on both sides
            print("zlib differs from the manifest's: %s compared with split_ref's bytes instead" % o["name"])
