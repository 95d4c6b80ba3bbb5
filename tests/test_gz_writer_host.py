"""CPU: host/gz_writer.hpp -- text in pieces of any size -> a gzip file of consecutive members that decompresses to the
text, in order; restart() forgets what was written; no text at all is one empty member; abandon() leaves a 0-byte file."""
import gzip
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "host/gz_writer.hpp"
#include <string>
using namespace hpn;
int main()
{
    std::string all;
    {
        GzWriter w("out.gz");
        for (int i = 0; i < 120; ++i) {
            std::string s;
            for (int j = 0; j < (i % 7) * 90000 + 17; ++j) {
                s += "ACGT"[(i * 31 + j * 7) % 4];
                if (j % 100 == 99) s += '\n';
            }
            all += s;
            if (!w.write(s.data(), s.size())) return 1;
            if (i == 40) {
                if (!w.restart()) return 2;
                all.clear();
            }
        }
        if (!w.finish()) return 3;
    }
    FILE *f = fopen("want.txt", "wb");
    fwrite(all.data(), 1, all.size(), f);
    fclose(f);
    {
        GzWriter e("empty.gz");
        if (!e.finish()) return 4;
    }
    {
        GzWriter a("abandoned.gz");
        a.abandon();
    }
    GzWriter bad("no_such_dir/x.gz");
    return bad.ok() ? 5 : 0;
}
"""


def test_gz_writer_round_trip(tmp_path):
    (tmp_path / "driver.cpp").write_text(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "highperformancengs_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "driver.cpp", "-o", "driver", "-lz", "-lpthread"], cwd=tmp_path)
    subprocess.check_call(["./driver"], cwd=tmp_path)
    raw = (tmp_path / "out.gz").read_bytes()
    want = (tmp_path / "want.txt").read_bytes()
    assert len(want) > 20 << 20
    assert gzip.decompress(raw) == want
    assert raw.count(b"\x1f\x8b\x08\x00") >= len(want) // (512 << 10)      # consecutive members of at most 512 KiB of text
    assert gzip.decompress((tmp_path / "empty.gz").read_bytes()) == b"" and os.path.getsize(tmp_path / "empty.gz") > 0
    assert os.path.getsize(tmp_path / "abandoned.gz") == 0
