"""The hpn_bam_fixmate_* bindings INTEGRATION.md shows are real: tests/abi/seam3_fixmate.c is the session as a C99 program, compiled
with -std=c99 -pedantic -Wall -Wextra -Werror against include/hpngs.h and linked with libhpngs only.  CPU: it compiles and links.
GPU: the order it prints, the counts and every block's length and CRC-32 are the restatement's (tests/fixmate_ref.py), whatever
the slice, with and without -r; the first record outside the domain is named."""
import subprocess
import zlib

import pytest

import fixmate_inputs
import fixmate_ref
from bamsort_ref import cut
from split_cases import stop_on_fault
from test_abi_c import _cc


def test_the_stub_compiles_and_links(tmp_path):
    exe = _cc("seam3_fixmate.c", tmp_path / "seam3_fixmate")
    assert "libhpngs.so" in subprocess.run(["ldd", exe], stdout=subprocess.PIPE).stdout.decode()


def expected(data, remove):
    p = fixmate_ref.parse(data)
    bad = fixmate_ref.device_reason(p.recs, len(p.targets))
    if bad:
        c = fixmate_ref.core(p.recs[bad[0]])
        return ["outside record %d refID %d pos %d reason %d" % (bad[0], c["tid"], c["pos"], bad[1])]
    out, n = fixmate_ref.machine(p.recs, [ln for _, ln in p.targets], remove)
    want = ["records %d out %d pairs %d singletons %d tags %d added %d payload %d" % (len(p.recs), len(out), n["pairs"], n["singletons"], n["tags"], n["added"],
                                                                                        sum(len(r) for _, r in out)),
            " ".join(["order"] + [str(i) for i, _ in out])]
    return want + ["block %d %08x" % (len(b), zlib.crc32(b) & 0xffffffff) for b in cut(b"", [r for _, r in out])]


@pytest.mark.gpu
def test_the_stub_fixes_as_the_restatement(tmp_path):
    exe = _cc("seam3_fixmate.c", tmp_path / "seam3_fixmate")
    inputs = fixmate_inputs.own_inputs()
    for name, slices in (("mixed", ("0", "7")), ("skipped_between", ("0", "1")), ("ct_straddles_cut", ("50",)), ("flags_and_ends", ("0",)),
                         ("no_records", ("0",)), ("only_skipped", ("0",)), ("op_back", ("0",)), ("tid_beyond_header", ("0",))):
        work = tmp_path / name
        work.mkdir()
        given = fixmate_inputs.materialize(str(work), name, inputs[name])
        for remove in ("0", "1"):
            want = expected(inputs[name], remove == "1")
            for per in slices:
                p = subprocess.run([exe, per, remove, given], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
                stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
                assert p.returncode == 0, p.stderr.decode()
                assert p.stdout.decode().splitlines() == want, (name, per, remove)
