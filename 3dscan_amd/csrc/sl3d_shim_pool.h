// sl3d_shim_pool.h -- the host threads of the drop-in shim (sl3d_shim.cpp) for its short bursts (file decode, text formatting:
// tens of milliseconds), on their own: plain C++17, no HIP, no shim state, so that the test suite can compile them with
// -fsanitize=address,undefined (tests/native/shim_io_check.cpp, tests/test_shim_io.py).
//   usable_threads : how many threads a burst may use
//   WorkerPool     : the threads, started once, parked between bursts
//   parallel_for   : fn(i) for i in [0, n) on them
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <functional>
#include <mutex>
#include <sched.h>
#include <thread>
#include <vector>

namespace sl3d_pool {

// the affinity mask, at most 32.  A cgroup CPU quota is an average over its period, not a core count -- on the GPU boxes (256 cores
// visible, quota 16) 32 threads finish such a burst in 0.6 of the time 16 take -- so it is not applied here.  SL3D_SHIM_THREADS
// overrides.
inline int usable_threads()
{
    static int n = [] {
        int k = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) k = CPU_COUNT(&set);
        k = std::min(k, 32);
        if (const char *e = getenv("SL3D_SHIM_THREADS")) k = atoi(e);
        return std::max(1, std::min(k, 256));
    }();
    return n;
}

// The host threads behind parallel_for: started once, parked on a condition variable between bursts (a burst that spawns and joins
// its own std::threads pays ~0.1 ms, in a stage call of a scan that takes 2-4 ms, four times per scan).
class WorkerPool {
public:
    static WorkerPool &get()
    {
        static WorkerPool *p = new WorkerPool(usable_threads() - 1);  // (never destroyed: the workers may outlive static destruction order)
        return *p;
    }
    // runs job(i) for i in [0, n) on the calling thread and up to `helpers` workers; returns when all items are done
    void run(int n, int helpers, const std::function<void(int)> &job)
    {
        std::unique_lock<std::mutex> serial(run_mu_);  // one burst at a time
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &job;
            n_ = n;
            next_.store(0);
            pending_ = n;
            wanted_ = std::min(helpers, (int)workers_.size());
            generation_++;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return pending_ == 0 && active_ == 0; });
        wanted_ = 0;  // (a worker that has not woken yet stays parked)
        job_ = nullptr;
        if (error_) {
            std::exception_ptr e = error_;
            error_ = nullptr;
            lk.unlock();
            std::rethrow_exception(e);
        }
    }

private:
    explicit WorkerPool(int k)
    {
        for (int i = 0; i < k; i++) workers_.emplace_back([this] { loop(); }), workers_.back().detach();
    }
    void work()
    {
        int done = 0;
        for (int i; (i = next_.fetch_add(1)) < n_;) {
            try {  // (an exception must not leave a worker thread -- std::terminate -- nor stop the burst's bookkeeping: the first one
                   // is kept and rethrown by run() on the calling thread, inside the caller's own exception barrier)
                (*job_)(i);
            } catch (...) {
                std::lock_guard<std::mutex> lk(mu_);
                if (!error_) error_ = std::current_exception();
            }
            done++;
        }
        if (done) {
            std::lock_guard<std::mutex> lk(mu_);
            pending_ -= done;
            if (pending_ == 0) done_cv_.notify_all();
        }
    }
    void loop()
    {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return generation_ != seen && wanted_ > 0; });
                seen = generation_;
                wanted_--;
                active_++;
            }
            work();
            {
                std::lock_guard<std::mutex> lk(mu_);
                active_--;
                if (pending_ == 0 && active_ == 0) done_cv_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_, run_mu_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(int)> *job_ = nullptr;
    std::exception_ptr error_;
    std::atomic<int> next_{0};
    int n_ = 0, pending_ = 0, wanted_ = 0, active_ = 0;
    unsigned long long generation_ = 0;
};

// fn(i) for i in [0, n) on up to `threads` threads (work items are handed out one by one); the calling thread takes part
template <typename Fn>
void parallel_for(int n, Fn fn, int threads = usable_threads())
{
    const int t = std::min(n, threads);
    if (t <= 1) {
        for (int i = 0; i < n; i++) fn(i);
        return;
    }
    const std::function<void(int)> job = [&](int i) { fn(i); };
    WorkerPool::get().run(n, t - 1, job);
}

}  // namespace sl3d_pool
