"""CPU: bamSplitChr's recorded reference runs (tests/golden/split/manifest.json, made by tests/golden/make_golden_split.py from
the compiled reference) against the Python restatement tests/split_ref.py -- partition + cut rule + framing -- and against the
tool's host route (HPN_BAM_GPU=0: the host reader, BgzfCutter and BgzfWriter; no device is opened).

Every `same` case: file names, status, masked stderr, the ISIZE sequence, every block's CRC-32 and the inflated bytes, always;
level-0 files and the empty last block whole, always; files of levels >= 1 whole against the manifest when this machine's zlib
is the one the manifest was recorded with (else against what split_ref makes with this machine's zlib, and the skipped
comparison is said).  Every `refuse` case is classified from the input alone; the tool leaves with status 2, names the record
the restatement names, and leaves no output."""
import zlib

import pytest

import split_cases as SC
import split_inputs
import split_ref
from split_cases import CASES, MANIFEST


@pytest.fixture(scope="session")
def made(tmp_path_factory):
    return SC.materialize_checked(str(tmp_path_factory.mktemp("split_inputs")))


SAME_WITH_FILES = [c["id"] for c in MANIFEST["cases"] if c["expect"] == "same" and c["rc"] == 0]


@pytest.mark.parametrize("cid", SAME_WITH_FILES)
def test_the_restatement_reproduces_the_reference(made, cid):
    case = CASES[cid]
    files, err = SC.run_model(case, made)
    assert sorted(files) == sorted(o["name"] for o in case["outputs"])
    assert err == case["stderr"]
    level = SC.level_of(case["args"])
    whole = [SC.check_file(o, files[o["name"]], level, (cid, o["name"])) for o in case["outputs"]]
    if not all(whole):
        print("zlib %s here, %s in the manifest: whole-file comparison of %d files skipped" % (zlib.ZLIB_RUNTIME_VERSION, MANIFEST["zlib"], whole.count(False)))


@pytest.mark.parametrize("cid", [c["id"] for c in MANIFEST["cases"] if c["expect"] == "refuse"])
def test_refusals_are_classified_from_the_input_alone(made, cid):
    case = CASES[cid]
    path = split_inputs.path_of(case["inputs"][0], made)
    prefix = case["args"][case["args"].index("-o") + 1]
    k = split_ref.classify(split_ref.read(path), open(path + ".bai", "rb").read(), prefix)
    assert k is not None and case["why"] == "in.bam: " + " ".join(str(x) for x in k)


def test_the_manifest_covers_the_issue():
    kinds = {c["expect"] for c in MANIFEST["cases"]}
    assert kinds == {"same", "refuse", "usage"}
    assert CASES["u_eats_o"]["rc"] == 1 and CASES["no_bai"]["rc"] == 1 and CASES["missing_input"]["rc"] == 1
    assert len(CASES["two_inputs"]["outputs"]) == 7
    assert all(n <= split_ref.FULL for c in MANIFEST["cases"] for o in c["outputs"] for n in o["isize"])
    edges = [o for o in CASES["u_edges"]["outputs"] if o["name"] == "o_c0.bam"][0]["isize"]
    assert split_ref.FULL - 1 in edges and split_ref.FULL in edges and 200 in edges and 70000 - split_ref.FULL + 38 in edges


@pytest.mark.parametrize("cid", [c["id"] for c in MANIFEST["cases"]])
def test_the_host_route_of_the_tool(made, tmp_path, cid):
    """HPN_BAM_GPU=0: every recorded case through the tool's host reader, BgzfCutter and BgzfWriter"""
    SC.check_tool(CASES[cid], made, tmp_path, {"HPN_BAM_GPU": "0"})


@pytest.mark.parametrize("opt", [[], ["-u", "x"]])
def test_the_host_route_on_300_targets(made, tmp_path, opt):
    SC.check_tool(SC.model_case("t300", "t300", opt + ["-o", "o", "in.bam"], made), made, tmp_path, {"HPN_BAM_GPU": "0"})


def test_the_tool_prints_its_zlib_under_timing(made, tmp_path):
    rc, out, err, files = SC.run_tool(CASES["d_one_each"], made, tmp_path, {"HPN_BAM_GPU": "0", "HPN_TIMING": "1"})
    assert rc == 0 and "[hpn] zlib %s\n" % zlib.ZLIB_RUNTIME_VERSION in SC.HPN_LINES and err == CASES["d_one_each"]["stderr"]
