"""The hpn_bam_sort_* bindings INTEGRATION.md shows are real: tests/abi/seam3_sort.c is the loop as a C99 program, compiled with
-std=c99 -pedantic -Wall -Wextra -Werror against include/hpngs.h and linked with libhpngs only.  CPU: it compiles and links.
GPU: the order it prints and every block's length and CRC-32 are the restatement's (tests/bamsort_ref.py), whatever the slice."""
import subprocess
import zlib

import numpy as np
import pytest

import bamsort_inputs
import bamsort_ref
from split_cases import stop_on_fault
from test_abi_c import _cc


def test_the_stub_compiles_and_links(tmp_path):
    exe = _cc("seam3_sort.c", tmp_path / "seam3_sort")
    assert "libhpngs.so" in subprocess.run(["ldd", exe], stdout=subprocess.PIPE).stdout.decode()


@pytest.mark.gpu
def test_the_stub_sorts_as_the_restatement(tmp_path):
    exe = _cc("seam3_sort.c", tmp_path / "seam3_sort")
    inputs = bamsort_inputs.own_inputs()
    for name, slices in (("strands", ("", "100")), ("oversize", ("", "3")), ("hd_long", ("",)), ("packed_1000", ("7",)), ("no_records", ("",))):
        path = tmp_path / (name + ".bam")
        path.write_bytes(inputs[name])
        recs = bamsort_ref.parse(inputs[name]).recs
        order = list(np.argsort(bamsort_ref.model_keys(recs), kind="stable")) if recs else []
        want = ["records %d payload %d" % (len(recs), sum(len(r) for r in recs)), " ".join(["order"] + [str(i) for i in order])]
        want += ["block %d %08x" % (len(p), zlib.crc32(p) & 0xffffffff) for p in bamsort_ref.cut(b"", [recs[i] for i in order])]
        for per in slices:
            p = subprocess.run([exe, str(path)] + ([per] if per else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
            assert p.returncode == 0, p.stderr.decode()
            assert p.stdout.decode().splitlines() == want, (name, per)
