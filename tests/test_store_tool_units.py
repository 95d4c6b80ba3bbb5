"""CPU: canonical_feed of csrc/host/store_tool.hpp -- the host's framing of text the device refused, shared by gzfastq_sort,
fastq2twobit, gzfastq_uniqQ and gzfastq_uniq_sort -- on its own, compiled into a throw-away program: both field rules, both
lone-line settings, a flush threshold of 16 bytes so that every record crosses it.  The accepted text is checked against the
framing of the Python restatement (uniq_ref.records: gzgets into 1024 bytes, what strlen sees, the last byte dropped); a
refusal against the tools' words."""
import os
import subprocess

import pytest

import uniq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "../highperformancengs_amd/csrc/host/store_tool.hpp"
using namespace hpn;
// argv: rule (0 what strlen sees, 1 the line), keep_lone_line; the stream on stdin.  stdout: "refused: WHY", or the chunks'
// sizes ("!" behind the one flagged last) on one line and then the text.
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    std::string mem, text, sizes;
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, stdin)) > 0;) mem.append(buf, k);
    auto add = [&](const void *p, uint64_t n, bool last) {
        text.append((const char *)p, n);
        sizes += std::to_string(n) + (last ? "! " : " ");
        return true;
    };
    const char *why = canonical_feed(mem, atoi(argv[1]) ? FieldRule::kLine : FieldRule::kStrlen, atoi(argv[2]) != 0, add, 16);
    if (why) {
        printf("refused: %s", why);
        return 0;
    }
    printf("%s\n", sizes.c_str());
    fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
'''

BODY = b"@a x\nACGT\n+\nIIII\n" b"@b\nGG\n+\nII\n" b"@c\n\n+\n\n"
ENDS, LONG, LEADING_NUL, ANY_NUL = "the file ends inside a record", "line of 1023 or more characters", "line that starts with a NUL byte", "NUL byte in a line"
# (input, lone open line behind it, refusal under the strlen rule, refusal under the line rule)
CASES = {
    "regular": (BODY, b"", None, None),
    "last line open": (BODY[:-1] + b"II", b"", None, None),
    "lone open line": (BODY, b"@d", None, None),
    "line of 1022": (b"@n\n" + b"A" * 1022 + b"\n+\n" + b"I" * 1022 + b"\n", b"", None, None),
    "line of 1023": (b"@n\n" + b"A" * 1023 + b"\n+\n" + b"I" * 1023 + b"\n", b"", LONG, LONG),
    "leading NUL": (b"@a\n\0CGT\n+\nIIII\n", b"", LEADING_NUL, ANY_NUL),
    "NUL inside": (b"@a\nAC\0T\n+\nII\0I\n", b"", None, ANY_NUL),
    "ends after 1 line": (BODY + b"@d\n", b"", ENDS, ENDS),
    "ends after 2 lines": (BODY + b"@d\nAC\n", b"", ENDS, ENDS),
    "ends after 3 lines": (BODY + b"@d\nAC\n+\n", b"", ENDS, ENDS),
    "plus line with content": (b"@a\nACGT\n+a anything \t here\nIIII\n", b"", None, None),
    "empty": (b"", b"", None, None),
}


def canonical(data):
    return b"".join(b"%s\n%s\n+\n%s\n" % rec for rec in uniq_ref.records(data))


def build(tmp_path, flags=("-O1",)):
    src, exe = tmp_path / "c.cpp", tmp_path / "c"
    src.write_text(SRC.replace("../highperformancengs_amd", os.path.join(ROOT, "highperformancengs_amd")))
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-lpthread", "-lz"])
    return str(exe)


def check_case(exe, name):
    data, lone, why_strlen, why_line = CASES[name]
    for rule, why in ((0, why_strlen), (1, why_line)):
        for keep in (0, 1):
            p = subprocess.run([exe, str(rule), str(keep)], input=data + lone, stdout=subprocess.PIPE, check=True)
            if why:
                assert p.stdout == b"refused: " + why.encode(), (name, rule, keep)
                continue
            sizes, _, text = p.stdout.partition(b"\n")
            assert text == canonical(data) + (lone if keep else b""), (name, rule, keep)
            sizes = sizes.split()
            assert sizes[-1].endswith(b"!") and not any(s.endswith(b"!") for s in sizes[:-1]), (name, sizes)      # one last chunk, behind the others
            assert all(int(s) >= 16 for s in sizes[:-1]) and sum(int(s.rstrip(b"!")) for s in sizes) == len(text)
            if data.count(b"\n") >= 8:
                assert len(sizes) > 1, (name, sizes)      # the threshold was crossed
    if why_strlen:      # the restatement has no answer there either
        with pytest.raises(uniq_ref.NoAnswer):
            canonical(data)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("store_tool"))


@pytest.mark.parametrize("name", list(CASES))
def test_canonical_feed(exe, name):
    check_case(exe, name)
