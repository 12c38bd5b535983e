// pm_pool.h -- a small fork-join pool: run(n, fn) calls fn(0..n-1) on the workers and the caller.
// Behind host_parallel_for (pm_hostpar.cpp) and the large downloads' host copies (pm_hostio.cpp).
// No HIP header.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace pm {

class Pool {
  public:
    explicit Pool(int threads) {
        for (int i = 1; i < threads; ++i) workers_.emplace_back([this]() { loop(); });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> lock(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    int size() const { return (int)workers_.size() + 1; }
    // One generation at a time: run() publishes (job, tasks) only when no worker is inside
    // work(), and returns only when every task is done and every worker has left work(), so a
    // worker never mixes one generation's job with another's counter.  Workers take their
    // (job, tasks) snapshot under the lock.
    template <class F>
    void run(int tasks, F&& fn) {
        std::function<void(int)> f(std::forward<F>(fn));
        {
            std::unique_lock<std::mutex> lock(mu_);
            done_.wait(lock, [this]() { return active_ == 0; });
            job_ = &f;
            tasks_ = tasks;
            next_.store(0);
            pending_ = tasks;
            ++gen_;
        }
        cv_.notify_all();
        work(&f, tasks);
        std::unique_lock<std::mutex> lock(mu_);
        done_.wait(lock, [this]() { return pending_ == 0 && active_ == 0; });
        job_ = nullptr;
    }

  private:
    void work(std::function<void(int)>* job, int tasks) {
        for (int i = next_++; i < tasks; i = next_++) {
            (*job)(i);
            std::lock_guard<std::mutex> lock(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::function<void(int)>* job = nullptr;
            int tasks = 0;
            {
                std::unique_lock<std::mutex> lock(mu_);
                cv_.wait(lock, [&]() { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                if (!job_) continue;   // that generation has finished already
                job = job_;
                tasks = tasks_;
                ++active_;
            }
            work(job, tasks);
            std::lock_guard<std::mutex> lock(mu_);
            if (--active_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::function<void(int)>* job_ = nullptr;
    int tasks_ = 0, pending_ = 0, active_ = 0;
    std::atomic<int> next_{0};
    uint64_t gen_ = 0;
    bool stop_ = false;
};

}  // namespace pm
