// Small host-side tools of the runs that move bytes between files and the
// device: a stopwatch, whole-buffer read and write loops, a thread fan-out and
// the hand-off between the stages of a pipelined run.  Host only: no HIP
// include, builds with a plain host compiler (tests/c/blobsrc_check.cpp).
#pragma once

#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace cdc {

using Clock = std::chrono::steady_clock;
static double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

inline bool pread_all(int fd, uint8_t *dst, uint64_t len, uint64_t off)
{
    while (len) {
        const ssize_t r = pread(fd, dst, len, off_t(off));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        dst += r;
        off += uint64_t(r);
        len -= uint64_t(r);
    }
    return true;
}

inline bool pwrite_all(int fd, const uint8_t *src, uint64_t len, uint64_t off)
{
    while (len) {
        const ssize_t r = pwrite(fd, src, len, off_t(off));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        src += r;
        off += uint64_t(r);
        len -= uint64_t(r);
    }
    return true;
}

inline bool write_all(int fd, const uint8_t *src, uint64_t len)
{
    while (len) {
        const ssize_t r = write(fd, src, len);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        src += r;
        len -= uint64_t(r);
    }
    return true;
}

// fn(0) .. fn(n - 1) on up to `threads` threads, the caller's among them.
template <class F>
void parallel_for(int threads, size_t n, F fn)
{
    const size_t t = std::min<size_t>(size_t(std::max(threads, 1)), n);
    if (t <= 1) {
        for (size_t i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < t; ++k) th.emplace_back(work);
    work();
    for (auto &x : th) x.join();
}

// The hand-off between the stages of a pipelined run.  Each stage counts the
// batches it has passed in a counter of the run's; a stage waits for another's
// counter, and the first failure anywhere ends every wait.
struct Handoff {
    std::mutex mu;
    std::condition_variable cv;
    int fail = 0;  // CDC_OK, or the status of the first abort_run

    // Wait until `counter` reaches `want`; false when the run has failed.
    bool wait_for(const int &counter, int want)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return counter >= want || fail != 0; });
        return fail == 0;
    }
    void advance(int &counter)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            ++counter;
        }
        cv.notify_all();
    }
    void abort_run(int status)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (fail == 0) fail = status;
        }
        cv.notify_all();
    }
    bool failed()
    {
        std::lock_guard<std::mutex> lk(mu);
        return fail != 0;
    }
};

}  // namespace cdc
