// bgzf_writer.hpp -- payload blocks -> a BGZF file, deflated by several threads (modelled on gz_writer.hpp).
//
// samtools' writer (bgzf.c: deflate_block behind bgzf_flush) turns every block of at most 0xff00 bytes into one gzip member:
// the 18-byte header with the BC extra field, deflate(level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) in ONE Z_FINISH call,
// CRC-32, ISIZE -- on one core.  Here the blocks arrive cut (where they are cut is the caller's: the device's list, or
// BgzfCutter below on the host route) and, from the device route, with their CRC-32; each is deflated by one of usable_cpus()
// threads with the same parameters -- so the bytes are the reference's wherever the zlib is the same -- and one writer thread
// appends them in order.  At level 0 the device has framed the blocks already: add_framed() only appends.  One file is open
// at a time (begin / finish); the threads live as long as the writer, so thousands of small targets start no thread each.
// finish() appends the 28-byte empty block bgzf_close writes (made at the default level, whatever the file's level).
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "cpus.hpp"

namespace hpn {

constexpr uint32_t kBgzfPayloadMax = 0xff00;     // BGZF_BLOCK_SIZE (bgzf.c:41)

// One block of at most 0xff00 bytes as the BGZF member samtools writes.  level: -1 (default), 0 .. 9.
inline bool bgzf_member(const uint8_t *p, uint32_t n, uint32_t crc, int level, std::vector<uint8_t> &out)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (n > kBgzfPayloadMax || deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    out.resize(65536);
    z.next_in = const_cast<Bytef *>(p ? p : (const uint8_t *)"");
    z.avail_in = n;
    z.next_out = out.data() + 18;
    z.avail_out = 65536 - 18 - 8;
    const int r = deflate(&z, Z_FINISH);
    const size_t comp = z.total_out;
    deflateEnd(&z);
    if (r != Z_STREAM_END) return false;
    const uint32_t bsize = (uint32_t)comp + 25;     // total size - 1
    const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    memcpy(out.data(), head, 18);
    for (int k = 0; k < 4; ++k) out[18 + comp + k] = (uint8_t)(crc >> (8 * k)), out[22 + comp + k] = (uint8_t)(n >> (8 * k));
    out.resize(comp + 26);
    return true;
}

inline uint32_t bgzf_crc(const uint8_t *p, uint32_t n) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, n); }

// bgzf_write of `n` bytes that are no record (the BAM header: bam_header_write + bgzf_flush): a block every 0xff00 bytes.
inline bool bgzf_plain_blocks(const uint8_t *p, size_t n, int level, std::vector<uint8_t> &out)
{
    std::vector<uint8_t> one;
    for (size_t at = 0; at < n; at += kBgzfPayloadMax) {
        const uint32_t k = (uint32_t)(n - at < kBgzfPayloadMax ? n - at : kBgzfPayloadMax);
        if (!bgzf_member(p + at, k, bgzf_crc(p + at, k), level, one)) return false;
        out.insert(out.end(), one.begin(), one.end());
    }
    return true;
}

// bam_write1's cuts on the host (bam.c:238 bgzf_flush_try, then bgzf_write): the block is closed first if the record does not
// fit, and at once when it reaches 0xff00.  emit(bytes, len) gets every closed block.
template <typename Emit>
class BgzfCutter {
public:
    explicit BgzfCutter(Emit emit) : emit_(emit) { blk_.reserve(kBgzfPayloadMax); }
    void record(const uint8_t *p, size_t s)
    {
        if (blk_.size() + s > kBgzfPayloadMax) close();
        while (s) {
            const size_t k = kBgzfPayloadMax - blk_.size() < s ? kBgzfPayloadMax - blk_.size() : s;
            blk_.insert(blk_.end(), p, p + k);
            p += k, s -= k;
            if (blk_.size() == kBgzfPayloadMax) close();
        }
    }
    void close()
    {
        if (blk_.empty()) return;
        emit_(blk_.data(), (uint32_t)blk_.size());
        blk_.clear();
    }
    size_t fill() const { return blk_.size(); }

private:
    Emit emit_;
    std::vector<uint8_t> blk_;
};

class BgzfWriter {
public:
    explicit BgzfWriter(int level) : level_(level)
    {
        const long cpus = usable_cpus();
        threads_ = (int)(cpus < 1 ? 1 : cpus > 64 ? 64 : cpus);
    }
    ~BgzfWriter()
    {
        stop();
        if (fd_ >= 0) close(fd_);
    }
    bool ok() const { return !failed_; }
    double deflate_seconds() const { return deflate_s_; }
    double waited_seconds() const { return waited_s_; }

    // Creates (or empties) `path` and writes `head` (the header's blocks, made once per input) into it.
    bool begin(const char *path, const std::vector<uint8_t> &head)
    {
        if (fd_ >= 0) return false;
        fd_ = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd_ < 0) return false;
        failed_ = false;
        put(head.data(), head.size());
        return !failed_;
    }
    // One block, in order.  have_crc: `crc` is the payload's CRC-32 (the device's); else a thread computes it.
    bool add(const uint8_t *p, uint32_t n, uint32_t crc, bool have_crc)
    {
        if (fd_ < 0 || failed_) return false;
        auto job = std::make_shared<Job>();
        job->in.assign(p, p + n);
        job->crc = crc, job->have_crc = have_crc;
        push(job, true);
        return !failed_;
    }
    // Bytes that are blocks already (the device's stored image at level 0), in order.
    bool add_framed(const uint8_t *p, size_t n)
    {
        if (fd_ < 0 || failed_) return false;
        auto job = std::make_shared<Job>();
        job->out.assign(p, p + n);
        job->done = true;
        push(job, false);
        return !failed_;
    }
    // Everything is in the file, the empty last block behind it, the file closed.
    bool finish()
    {
        if (fd_ < 0) return false;
        drain();
        static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!failed_) put(eof, sizeof eof);
        if (close(fd_) != 0) failed_ = true;
        fd_ = -1;
        return !failed_;
    }
    void abandon()       // the file is closed as it is (the caller removes it)
    {
        if (fd_ < 0) return;
        drain();
        close(fd_);
        fd_ = -1;
    }

private:
    struct Job {
        std::vector<uint8_t> in, out;
        uint32_t crc = 0;
        bool have_crc = false, done = false, bad = false;
    };
    void push(const std::shared_ptr<Job> &job, bool work)
    {
        start();
        std::unique_lock<std::mutex> lk(m_);
        if (order_.size() >= (size_t)threads_ * 8) {
            const double t0 = wall_s();
            room_.wait(lk, [this] { return order_.size() < (size_t)threads_ * 8; });
            waited_s_ += wall_s() - t0;
        }
        if (work) todo_.push_back(job);
        order_.push_back(job);
        if (work) work_.notify_one();
        else done_.notify_all();
    }
    void start()
    {
        if (!pool_.empty()) return;
        for (int t = 0; t < threads_; ++t) pool_.emplace_back([this] { deflate_loop(); });
        writer_ = std::thread([this] { write_loop(); });
    }
    void drain()
    {
        const double t0 = wall_s();
        std::unique_lock<std::mutex> lk(m_);
        room_.wait(lk, [this] { return order_.empty(); });
        waited_s_ += wall_s() - t0;
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        work_.notify_all();
        done_.notify_all();
        for (std::thread &t : pool_) t.join();
        pool_.clear();
        if (writer_.joinable()) writer_.join();
        stop_ = false;
    }
    void deflate_loop()
    {
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lk(m_);
                work_.wait(lk, [this] { return !todo_.empty() || stop_; });
                if (todo_.empty()) return;
                job = todo_.front();
                todo_.pop_front();
            }
            const double t0 = wall_s();
            const uint32_t n = (uint32_t)job->in.size();
            const uint32_t crc = job->have_crc ? job->crc : bgzf_crc(job->in.data(), n);
            const bool ok = bgzf_member(job->in.data(), n, crc, level_, job->out);
            std::vector<uint8_t>().swap(job->in);
            const double dt = wall_s() - t0;
            {
                std::lock_guard<std::mutex> lk(m_);
                job->done = true, job->bad = !ok;
                deflate_s_ += dt;
            }
            done_.notify_all();
        }
    }
    void write_loop()
    {
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lk(m_);
                done_.wait(lk, [this] { return (!order_.empty() && order_.front()->done) || stop_; });
                if (order_.empty() || !order_.front()->done) return;
                job = order_.front();
            }
            if (job->bad) failed_ = true;
            if (!failed_) put(job->out.data(), job->out.size());
            {
                std::lock_guard<std::mutex> lk(m_);
                order_.pop_front();
            }
            room_.notify_all();
        }
    }
    void put(const uint8_t *p, size_t n)
    {
        for (size_t done = 0; done < n;) {
            const ssize_t k = ::write(fd_, p + done, n - done);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) {
                failed_ = true;
                return;
            }
            done += (size_t)k;
        }
    }
    int fd_ = -1;
    int level_;
    int threads_ = 1;
    bool stop_ = false;
    std::atomic<bool> failed_{false};
    double deflate_s_ = 0, waited_s_ = 0;
    std::deque<std::shared_ptr<Job>> todo_, order_;
    std::mutex m_;
    std::condition_variable work_, done_, room_;
    std::vector<std::thread> pool_;
    std::thread writer_;
};

}  // namespace hpn
