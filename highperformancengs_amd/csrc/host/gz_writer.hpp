// gz_writer.hpp -- text -> a gzip file, compressed by several threads.
//
// gzfastq_sample writes its output through gzprintf on one core (gzfastq_sample.c:30-37).  Here the text of a
// chunk arrives in one piece from the device; it is cut into slices of 512 KiB, each slice is deflated into a gzip
// member of its own by one of usable_cpus() threads (never the machine's core count: cpus.hpp), and a writer
// thread puts the members into the file in order -- all of it beside the caller, who only copies the text in and
// waits when more than a few slices per thread are queued.  A concatenation of gzip members is a gzip file
// (RFC 1952, 2.2): gzip -dc, zlib's gzread and the tools of this directory read it as one stream.  The
// compressed bytes differ from the reference's (they depend on the zlib build anyway); the decompressed bytes
// are the text handed in.  A file that got no text at all is one empty member -- a valid gzip file that
// decompresses to nothing.
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

class GzWriter {
public:
    static constexpr size_t kSlice = (size_t)512 << 10;

    // Creates (or empties) `path`.  Nothing is written before the first text or finish().
    explicit GzWriter(const char *path) : fd_(open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666))
    {
        const long cpus = usable_cpus();
        threads_ = (int)(cpus < 1 ? 1 : cpus > 64 ? 64 : cpus);
    }
    ~GzWriter()
    {
        stop();
        if (fd_ >= 0) close(fd_);
    }
    bool ok() const { return fd_ >= 0 && !failed_; }
    int threads() const { return threads_; }
    double deflate_seconds() const { return deflate_s_; }   // summed over the threads (valid after finish / drain)
    double waited_seconds() const { return waited_s_; }     // the caller's thread held up by a full queue or the final drain

    // One piece of text: copied into the queue; returns as soon as there is room for it.
    bool write(const void *text, size_t n)
    {
        if (!ok()) return false;
        if (!n) return true;
        start();
        const uint8_t *p = (const uint8_t *)text;
        for (size_t at = 0; at < n; at += kSlice) {
            const size_t k = n - at < kSlice ? n - at : kSlice;
            auto job = std::make_shared<Job>();
            job->in.assign(p + at, p + at + k);
            std::unique_lock<std::mutex> lk(m_);
            if (order_.size() >= (size_t)threads_ * 4) {
                const double t0 = wall_s();
                room_.wait(lk, [this] { return order_.size() < (size_t)threads_ * 4; });
                waited_s_ += wall_s() - t0;
            }
            todo_.push_back(job);
            order_.push_back(job);
            work_.notify_one();
        }
        any_ = true;
        return !failed_;
    }

    // Everything is in the file when this returns true; the file is closed.
    bool finish()
    {
        if (fd_ < 0) return false;
        drain();
        stop();
        if (!any_ && !failed_) {
            std::vector<uint8_t> m;
            if (member(nullptr, 0, m)) put(m.data(), m.size());
            else failed_ = true;
        }
        if (close(fd_) != 0) failed_ = true;
        fd_ = -1;
        return !failed_;
    }

    // Leave the file as it is -- created, and empty unless text was written -- without closing the stream: what the
    // reference leaves when it exits in front of its gzclose (gzfastq_sample.c:234-238).
    void abandon()
    {
        drain();
        stop();
        if (fd_ >= 0) close(fd_);
        fd_ = -1;
    }

    // Forget what was written (the input is read again by another route).
    bool restart()
    {
        drain();
        if (fd_ < 0 || ftruncate(fd_, 0) != 0 || lseek(fd_, 0, SEEK_SET) != 0) return false;
        any_ = false;
        return !failed_;
    }

private:
    struct Job {
        std::vector<uint8_t> in, out;
        bool done = false, bad = false;
    };
    void start()
    {
        if (!pool_.empty()) return;
        for (int t = 0; t < threads_; ++t) pool_.emplace_back([this] { deflate_loop(); });
        writer_ = std::thread([this] { write_loop(); });
    }
    void drain()   // until every queued slice is in the file
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
            const bool ok = member(job->in.data(), job->in.size(), job->out);
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
    static bool member(const uint8_t *p, size_t n, std::vector<uint8_t> &out)
    {
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        out.resize(deflateBound(&z, (uLong)n) + 32);
        z.next_in = const_cast<Bytef *>(p ? p : (const uint8_t *)"");
        z.avail_in = (uInt)n;
        z.next_out = out.data();
        z.avail_out = (uInt)out.size();
        const int r = deflate(&z, Z_FINISH);
        out.resize(z.total_out);
        deflateEnd(&z);
        return r == Z_STREAM_END;
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
    int fd_;
    int threads_ = 1;
    bool any_ = false, stop_ = false;
    std::atomic<bool> failed_{false};
    double deflate_s_ = 0, waited_s_ = 0;
    std::deque<std::shared_ptr<Job>> todo_, order_;
    std::mutex m_;
    std::condition_variable work_, done_, room_;
    std::vector<std::thread> pool_;
    std::thread writer_;
};

}  // namespace hpn
