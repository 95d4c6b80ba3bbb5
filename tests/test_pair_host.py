"""CPU: what bin/pick_pair does without a device -- the usage screen, a missing input and the refusal to run without a GPU -- against
the recorded reference runs (tests/golden/pair/)."""
import os
import subprocess

import pytest

from test_pair_golden import BY_ID, input_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "highperformancengs_amd", "bin", "pick_pair")


def run(args, cwd):
    p = subprocess.run([TOOL] + args, cwd=cwd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p, sorted(os.listdir(cwd))


def case_args(case):
    return [input_path(case[a[0]]) if a in ("a.fq", "b.fq") and case[a[0]] else a for a in case["args"]]


@pytest.mark.parametrize("cid", ["no_arguments", "help", "unknown_option"])
def test_usage(cid, tmp_path):
    case = BY_ID[cid]
    p, files = run(case["args"], tmp_path)
    assert p.returncode == case["rc"] == 1 and files == [] and p.stdout == b""
    assert b"Usage:" in p.stderr and b"[-1 READ1] [-2 READ2] [-o OUTFILE] [-h]" in p.stderr


@pytest.mark.parametrize("cid", ["missing_1", "missing_2"])
def test_a_missing_input(cid, tmp_path):
    case = BY_ID[cid]
    p, files = run(case_args(case), tmp_path)
    assert p.returncode == case["rc"] == 1 and files == [] and p.stdout == b""
    assert p.stderr.decode() == case["stderr"] == "open file no_such_file.fq failed\n"


def test_without_both_inputs_there_is_nothing_to_open(tmp_path):
    p, files = run(["-1", input_path(BY_ID["same3"]["a"])], tmp_path)      # (the reference hands gzopen a NULL name)
    assert p.returncode == 2 and files == [] and b"-2 READ2" in p.stderr


def test_no_device_is_an_error_not_a_fallback(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    case = BY_ID["same3"]
    p, files = run(case_args(case), tmp_path)
    assert p.returncode == 2 and files == [] and b"hpn_ctx_create" in p.stderr
