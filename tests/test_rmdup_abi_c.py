"""The hpn_bam_rmdup_* bindings INTEGRATION.md shows are real: tests/abi/seam3_rmdup.c is the loop as a C99 program, compiled with
-std=c99 -pedantic -Wall -Wextra -Werror against include/hpngs.h and linked with libhpngs only.  CPU: it compiles and links.
GPU: the order it prints, the counts per library and target and every block's length and CRC-32 are the restatement's
(tests/rmdup_ref.py), whatever the slice."""
import subprocess
import zlib

import pytest

import bamsort_ref
import rmdup_inputs
import rmdup_ref
from split_cases import stop_on_fault
from test_abi_c import _cc


def test_the_stub_compiles_and_links(tmp_path):
    exe = _cc("seam3_rmdup.c", tmp_path / "seam3_rmdup")
    assert "libhpngs.so" in subprocess.run(["ldd", exe], stdout=subprocess.PIPE).stdout.decode()


@pytest.mark.gpu
def test_the_stub_decides_as_the_restatement(tmp_path):
    exe = _cc("seam3_rmdup.c", tmp_path / "seam3_rmdup")
    inputs = rmdup_inputs.own_inputs()
    for name, slices in (("mixed", ("0", "100")), ("oversize", ("0", "3")), ("hd_long", ("0",)), ("packed_1000", ("7",)), ("no_records", ("0",)), ("tails", ("1",))):
        path = tmp_path / (name + ".bam")
        path.write_bytes(inputs[name])
        p = bamsort_ref.parse(inputs[name])
        recs = [rmdup_ref.Rec(b) for b in p.recs]
        tbl = rmdup_ref.id_table(p.text)
        libs = [b"\t"] + sorted(set(tbl.values()))
        order, counts, unmatched, bad = rmdup_ref.plan(recs, tbl)
        assert bad is None
        want = ["records %d out %d payload %d" % (len(recs), len(order), sum(len(p.recs[i]) for i in order)), " ".join(["order"] + [str(i) for i in order])]
        want += ["lib %d %d %d %d" % ((k, counts[l][1], counts[l][0], counts[l][2]) if l in counts else (k, 0, 0, -1)) for k, l in enumerate(libs)]
        tids = {r.tid for r in recs}
        want += ["target %d %d" % (t, unmatched.get(t, 0)) for t in range(len(p.targets)) if t in tids] + (["target %d 0" % len(p.targets)] if -1 in tids else [])
        want += ["block %d %08x" % (len(b), zlib.crc32(b) & 0xffffffff) for b in bamsort_ref.cut(b"", [p.recs[i] for i in order])]
        table = [a for i in sorted(tbl) for a in (i.decode(), str(libs.index(tbl[i])))]
        for per in slices:
            q = subprocess.run([exe, str(path), per, str(len(libs))] + table, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            stop_on_fault(q.returncode, q.stderr.decode("latin-1"))
            assert q.returncode == 0, q.stderr.decode()
            assert q.stdout.decode().splitlines() == want, (name, per)
