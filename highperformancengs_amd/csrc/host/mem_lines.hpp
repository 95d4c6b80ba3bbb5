// mem_lines.hpp -- a whole inflated stream in memory and zlib's gzgets / gzeof over it: what gzfastq_uniqQ and gzfastq_uniq_sort
// frame on the host when the device's framer has refused the text (or the input is standard input, which cannot be read twice).
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "fastq_reader.hpp"

namespace hpn {

// the whole inflated stream; false: the reader met a CRC-32 / ISIZE / data error
inline bool slurp_stream(const char *path, std::string &mem)
{
    InStream in = open_input_stream(path);
    std::vector<char> buf((size_t)1 << 20);
    for (;;) {
        const int k = in.read(buf.data(), (unsigned)buf.size());
        if (k <= 0) break;
        mem.append(buf.data(), (size_t)k);
    }
    const bool damaged = in.damaged();
    in.close();
    return !damaged;
}

// gzgets(file, buf, 1024) and gzeof over the stream in memory
struct MemLines {
    const std::string &d;
    size_t pos = 0;
    bool past = false;
    explicit MemLines(const std::string &s) : d(s) {}
    bool gets(const char **p, size_t *n)
    {
        if (pos >= d.size()) {
            past = true;
            return false;
        }
        const size_t room = d.size() - pos < (size_t)kLineBuf - 1 ? d.size() - pos : (size_t)kLineBuf - 1;
        const void *nl = memchr(d.data() + pos, '\n', room);
        size_t k = nl ? (size_t)((const char *)nl - (d.data() + pos)) + 1 : room;
        if (!nl && pos + k == d.size() && k < (size_t)kLineBuf - 1) past = true;
        *p = d.data() + pos, *n = k;
        pos += k;
        return true;
    }
};

}  // namespace hpn
