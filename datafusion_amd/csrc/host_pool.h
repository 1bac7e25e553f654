// Host worker threads for the staging copies of the host paths
// (host_chunks.cpp, host_batches.cpp), and the copy tasks they run. Host only.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace dfmi {
namespace host {

using Tasks = std::vector<std::function<void()>>;

// Persistent workers for the host copies: one core's memcpy (~10-20 GB/s)
// would bound the pipeline below what PCIe Gen5 moves. Task i runs on worker
// i % (workers + 1) (the caller is worker 0); run() returns when every worker
// has finished its share of this job, so no worker ever sees a stale job.
class Pool {
   public:
    explicit Pool(int workers) {
        for (int w = 0; w < workers; ++w) th_.emplace_back([this, w] { loop(w + 1); });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void run(const Tasks& tasks) {
        if (tasks.empty()) return;
        if (th_.empty() || tasks.size() == 1) {
            for (auto& t : tasks) t();
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &tasks;
            remaining_ = (int)th_.size();
            ++epoch_;
        }
        cv_.notify_all();
        share(tasks, 0);
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return remaining_ == 0; });
        job_ = nullptr;
    }
    int ways() const { return (int)th_.size() + 1; }

   private:
    void share(const Tasks& t, int me) {
        for (size_t i = me; i < t.size(); i += th_.size() + 1) t[i]();
    }
    void loop(int me) {
        uint64_t seen = 0;
        for (;;) {
            const Tasks* J;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return stop_ || epoch_ != seen; });
                if (stop_) return;
                seen = epoch_;
                J = job_;
            }
            share(*J, me);
            std::lock_guard<std::mutex> g(m_);
            if (--remaining_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const Tasks* job_ = nullptr;
    uint64_t epoch_ = 0;
    int remaining_ = 0;
    bool stop_ = false;
};

inline int host_threads() {
    if (const char* e = getenv("DFMI_HOST_THREADS")) return std::max(1, std::min(64, atoi(e)));
    const int hw = (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(hw > 0 ? hw : 1, 8));
}

// Append a copy of n bytes as tasks of >= 4 MiB each (at most `ways` pieces).
inline void add_copy(Tasks& T, void* dst, const void* src, size_t n, int ways) {
    if (!n) return;
    constexpr size_t kMin = (size_t)4 << 20;
    const size_t k = std::max<size_t>(1, std::min<size_t>((size_t)ways, n / kMin));
    const size_t piece = ((n + k - 1) / k + 63) & ~(size_t)63;
    for (size_t o = 0; o < n; o += piece) {
        const size_t m = std::min(piece, n - o);
        T.emplace_back([=] { memcpy((uint8_t*)dst + o, (const uint8_t*)src + o, m); });
    }
}

// dst[i] = src[i] + add for i < n (Utf8 offset rebase while copying out).
inline void add_copy_rebase(Tasks& T, int32_t* dst, const int32_t* src, size_t n, int32_t add, int ways) {
    if (!n) return;
    constexpr size_t kMin = (size_t)1 << 20;
    const size_t k = std::max<size_t>(1, std::min<size_t>((size_t)ways, n / kMin));
    const size_t piece = (n + k - 1) / k;
    for (size_t o = 0; o < n; o += piece) {
        const size_t m = std::min(piece, n - o);
        T.emplace_back([=] {
            for (size_t i = 0; i < m; ++i) dst[o + i] = src[o + i] + add;
        });
    }
}

}  // namespace host
}  // namespace dfmi
