"""The hpn_bam_merge_* bindings INTEGRATION.md shows are real: tests/abi/seam3_merge.c is the session as a C99 program, compiled
with -std=c99 -pedantic -Wall -Wextra -Werror against include/hpngs.h and linked with libhpngs only.  CPU: it compiles and links.
GPU: the order it prints, the lifted count and every block's length and CRC-32 are the restatement's (tests/bammerge_ref.py),
whatever the slice; the record with the HEAP_EMPTY key is named."""
import subprocess
import zlib

import pytest

import bammerge_inputs
import bammerge_ref
from bamsort_ref import cut
from split_cases import stop_on_fault
from test_abi_c import _cc


def test_the_stub_compiles_and_links(tmp_path):
    exe = _cc("seam3_merge.c", tmp_path / "seam3_merge")
    assert "libhpngs.so" in subprocess.run(["ldd", exe], stdout=subprocess.PIPE).stdout.decode()


def expected(files):
    recs = [bammerge_ref.parse(f).recs for f in files]
    keys = [[bammerge_ref.key(r) for r in f] for f in recs]
    base = [sum(len(f) for f in recs[:k]) for k in range(len(recs))]
    if any(bammerge_ref.EMPTY in k for k in keys):
        f, i = next((f, k.index(bammerge_ref.EMPTY)) for f, k in enumerate(keys) if bammerge_ref.EMPTY in k)
        tid, pos, _ = bammerge_ref.fields(recs[f][i])
        return ["outside record %d refID %d pos %d reason 1" % (base[f] + i, tid, pos)]
    order, lifted = bammerge_ref.effective_order(keys)
    assert order == bammerge_ref.heap_order(keys)
    n = sum(len(f) for f in recs)
    want = ["records %d files %d payload %d lifted %d" % (n, len(files), sum(len(r) for f in recs for r in f), lifted),
            " ".join(["order"] + [str(base[f] + i) for f, i in order])]
    return want + ["block %d %08x" % (len(p), zlib.crc32(p) & 0xffffffff) for p in cut(b"", [recs[f][i] for f, i in order])]


@pytest.mark.gpu
def test_the_stub_merges_as_the_restatement(tmp_path):
    exe = _cc("seam3_merge.c", tmp_path / "seam3_merge")
    sets = bammerge_inputs.own_sets()
    for name, slices in (("three_sorted", ("0", "50")), ("unsorted_all", ("0", "7")), ("oversize", ("3",)), ("empty_middle", ("0",)), ("all_empty", ("0",)),
                         ("seventeen", ("100",)), ("heap_empty_2p31m2", ("0",))):      # (a pos of -2 has the same key, but the record index takes no pos below -1)
        work = tmp_path / name
        work.mkdir()
        given = bammerge_inputs.materialize(str(work), name, sets[name])
        want = expected(sets[name])
        for per in slices:
            p = subprocess.run([exe, per] + given, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            stop_on_fault(p.returncode, p.stderr.decode("latin-1"))
            assert p.returncode == 0, p.stderr.decode()
            assert p.stdout.decode().splitlines() == want, (name, per)
