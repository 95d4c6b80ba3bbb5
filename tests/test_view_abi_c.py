"""The hpn_bam_view_* bindings INTEGRATION.md shows are real: tests/abi/seam3_view.c is the session as a C99 program, compiled with
-std=c99 -pedantic -Wall -Wextra -Werror against include/hpngs.h and linked with libhpngs only.  CPU: it compiles and links.  GPU:
the count and the text it prints are the restatement's (tests/view_ref.py), whatever the slice; the first record outside the
domain is named."""
import subprocess

import pytest

import view_inputs
import view_ref
from split_cases import stop_on_fault
from test_abi_c import _cc


def test_the_stub_compiles_and_links(tmp_path):
    exe = _cc("seam3_view.c", tmp_path / "seam3_view")
    assert "libhpngs.so" in subprocess.run(["ldd", exe], stdout=subprocess.PIPE).stdout.decode()


def expected(data, emit, flag_off):
    p = view_ref.parse(data)
    args = ["-F", str(flag_off)] + (["-c"] if emit == 2 else []) + ["in.bam"]
    bad = view_ref.device_reason(p.recs, len(p.targets), view_ref.options(args))
    if bad:
        c = view_ref.core(p.recs[bad[0]])
        return b"outside record %d refID %d pos %d reason %d\n" % (bad[0], c["tid"], c["pos"], bad[1])
    out, _, _, rc = view_ref.view(data, args)
    assert rc == 0
    kept = int(out) if emit == 2 else out.count(b"\n")
    return b"records %d kept %d text %d\n" % (len(p.recs), kept, 0 if emit == 2 else len(out)) + (b"" if emit == 2 else out)


@pytest.mark.gpu
def test_the_stub_views_as_the_restatement(tmp_path):
    exe = _cc("seam3_view.c", tmp_path / "seam3_view")
    inputs = view_inputs.inputs()
    for name, flag_off, slices in (("lengths", 0, ("0", "1")), ("aux_all", 0, ("0",)), ("runs", 0x400, ("2049",)), ("no_records", 0, ("0",)),
                                   ("aux_float", 0, ("0",)), ("tid_beyond_header", 0, ("0",))):
        work = tmp_path / name
        work.mkdir()
        given = view_inputs.materialize(str(work), name, inputs[name])
        for emit in (1, 2):
            want = expected(inputs[name], emit, flag_off)
            for per in slices:
                p = subprocess.run([exe, str(emit), str(flag_off), per, given], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
                stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
                assert p.returncode == 0, p.stderr.decode()
                assert p.stdout == want, (name, per, emit)
