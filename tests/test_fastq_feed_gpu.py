"""GPU: gzfastq_sample, gzfastq_uniq and gzfastq_sort when an input route is LEFT after it has accepted text -- half a
megabyte of regular reads first, then, in the last quarter of the file,

  - a record whose name line holds a NUL byte: irregular text to the device framer on every route, so what the session holds
    is dropped and the host's exact framer reads the file again from its first byte;
  - a BGZF block that fails its check: the device's decoder reports it (an error code, as in test_cli_gpu.py), the route is
    given up, the host's reader meets the same block and the tool refuses the file.

Expected bytes come from the Python restatements that the *_golden.py tests pin to the reference's recorded outputs.
sample_ref does not model NUL bytes; it is given the late record as readNextNode keeps it -- the name line as strlen sees
it ("@late x") without its last byte, which stands where the newline would (gzfastq_sample.c:319; uniq_ref._cstr(line)[:-1]
is the same statement): "@late ".  Leaving the 'x' in place is NOT what the reference writes: it prints "@late _5688"."""
import gzip
import os
import re
import subprocess

import pytest

import sample_ref
import sort_inputs
import sort_ref
import uniq_inputs
import uniq_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "highperformancengs_amd", "bin")
TIMES = re.compile(r"at \d+\.\d{3} s")
LATE = b"@late x\0junk\nACGT\n+\nIIII\n"
SAMPLE_ARGS = ["-s", "5.2", "-n", "6000"]

# (name, the file the route reads, the switches that force the route and cut the text into many pieces)
ROUTES = [("plain text, small chunks", "plain", {"HPN_TEXT_CHUNK": "4099"}),
          ("bgzip on the device, sliced", "bgzip", {"HPN_TEXT_SLICE": "5000", "HPN_BAM_CHUNK": "70000"}),
          ("one gzip member on the device", "gzip", {"HPN_GZ_GPU_FORCE": "1", "HPN_GZ_STRETCH": "8192", "HPN_GZ_BATCH": "7", "HPN_TEXT_SLICE": "4099"}),
          ("host framer", "plain", {"HPN_TEXT": "0"})]


def bgzip(text, block=3000):
    import io
    from highperformancengs_amd.bamio import _Bgzf
    fh = io.BytesIO()
    z = _Bgzf(fh)
    for i in range(0, len(text), block):
        z.write(text[i:i + block])
    z.close()
    return fh.getvalue()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The files (every packing under the one name late.fq / late.fq.gz, in a directory of its own) and what each tool
    has to make of them, computed once."""
    regular = sort_inputs.illumina(1500) + uniq_inputs.dups5000()
    lines = regular.split(b"\n")
    k = (len(lines) // 4) * 7 // 8
    text = b"\n".join(lines[:4 * k]) + b"\n" + LATE + b"\n".join(lines[4 * k:])
    assert 400_000 < len(text) < 600_000 and text.index(LATE) > 3 * len(text) // 4 and text.endswith(b"\n")
    damaged = bytearray(bgzip(regular))
    damaged[len(damaged) // 2] ^= 0x55
    base = tmp_path_factory.mktemp("feed")
    paths = {}
    for kind, name, data in (("plain", "late.fq", text), ("bgzip", "late.fq.gz", bgzip(text)), ("gzip", "late.fq.gz", gzip.compress(text, 6)),
                             ("damaged", "bad.fq.gz", bytes(damaged))):
        os.makedirs(base / kind)
        paths[kind] = str(base / kind / name)
        open(paths[kind], "wb").write(data)
    as_kept = text.replace(b"x\0junk", b"")      # (module docstring)
    want = {"uniq": uniq_ref.simulate(text)[:2], "sort -s": sort_ref.simulate(text, False, bookkeeping=False)[:2],
            "sort -n": sort_ref.simulate(text, True, bookkeeping=False)[:2]}
    for name in ("late.fq", "late.fq.gz"):
        want["sample", name] = sample_ref.simulate(SAMPLE_ARGS, name, as_kept)
    assert b"@late _" in want["sample", "late.fq"][0]["late.fq.6000.gz"]      # the late record is among the picks
    return paths, want


def run(tool, args, cwd, env):
    os.makedirs(cwd)
    p = subprocess.run([os.path.join(BIN, tool)] + args, cwd=cwd, env={**os.environ, **env}, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p, {fn: open(os.path.join(cwd, fn), "rb").read() for fn in os.listdir(cwd)}


def command(tool, path):
    if tool == "sample":
        return "gzfastq_sample", ["-1", path] + SAMPLE_ARGS
    if tool == "uniq":
        return "gzfastq_uniq", ["-1", path, "-o", "o"]
    return "gzfastq_sort", ["-i", path, "-o", "o", tool[-2:]]


@pytest.mark.parametrize("tool", ["sample", "uniq", "sort -s", "sort -n"])
def test_late_irregular_record_on_every_route(tool, inputs, tmp_path):
    paths, want = inputs
    for k, (what, kind, env) in enumerate(ROUTES):
        exe, args = command(tool, paths[kind])
        p, got = run(exe, args, tmp_path / ("r%d" % k), env)
        err = TIMES.sub("at T s", p.stderr.decode("latin-1"))
        print(tool, "|", what, "| status", p.returncode, "|", {fn: len(v) for fn, v in got.items()})
        assert p.returncode == 0, (what, err)
        assert p.stdout == b"", what
        if tool == "sample":
            files, want_err = want["sample", os.path.basename(paths[kind])]
            got = {fn: gzip.decompress(v) if v else None for fn, v in got.items()}
        elif tool == "uniq":
            files, want_err = {"o" + suffix: v for suffix, v in want["uniq"][0].items()}, want["uniq"][1]
        else:
            files, want_err = {"o_sort_by_name.fq" if tool == "sort -n" else "o_sort_by_seq.fq": want[tool][0]}, want[tool][1]
        assert got == files, what
        assert err == want_err, what


@pytest.mark.parametrize("tool", ["sample", "uniq", "sort -s"])
def test_late_damaged_block_is_refused(tool, inputs, tmp_path):
    paths, _ = inputs
    # (small launches and slices: the device route has handed text on before it meets the damaged block, so the sink starts over)
    for k, env in enumerate(({}, {"HPN_BAM_GPU": "0"}, {"HPN_BAM_CHUNK": "70000", "HPN_TEXT_SLICE": "5000"})):
        exe, args = command(tool, paths["damaged"])
        p, _ = run(exe, args, tmp_path / ("r%d" % k), env)
        print(tool, "|", env, "| status", p.returncode, "|", p.stderr)
        assert p.returncode == 2, (env, p.stderr.decode("latin-1"))
        assert p.stderr.startswith(exe.encode() + b": ") and p.stderr.count(b"\n") == 1 and p.stderr.endswith(b"\n"), (env, p.stderr)
        assert b"bad.fq.gz" in p.stderr, (env, p.stderr)
