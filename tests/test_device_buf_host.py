"""CPU: the owning device buffers under the store families -- Scratch (csrc/hpn_ctx.hpp), InfoBlock, StoreSession, grow_keep
(csrc/hpn_store.hpp) and the Sorter (csrc/hpn_sorter.hpp) -- inside a stand-alone program with its own main
(tests/device_buf_host_main.cpp) that defines counting, malloc-backed stand-ins for the HIP calls the headers make and links no
HIP runtime.  Built with g++ -fsanitize=address,undefined and run as a process of its own: nothing built here is loaded into
python.  Every case ends with no live allocation and no pointer freed twice; the program says which cases it ran."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

CASES = ["move_construct", "move_assign_live", "self_move", "release_twice", "reserve_growth", "grow_keep_carries", "grow_keep_malloc_fails",
         "grow_keep_copy_fails", "info_block", "store_session", "family_state"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_buf") / "device_buf_host_main")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_buf_host_main.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtimes inside the program)
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
                           src, "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_the_program_ends_clean(run):
    assert run.returncode == 0 and run.stderr == b"", run.stderr.decode()[-2000:]      # (a sanitizer's report would stand here)
    assert run.stdout.decode().split("\n")[:-1] == ["ok " + c for c in CASES]


@pytest.mark.parametrize("case", CASES)
def test_case(run, case):
    assert ("ok " + case).encode() in run.stdout.split(b"\n"), run.stderr.decode()[-2000:]
