// worker.h — a single-slot worker thread: one job handed over at a time, run on a thread of its own.
//
//   Worker<Job, Err, Sticky>   Job: copyable, with `Err run() const`; Err: its error type, whose
//                              value-initialised value (Err{}) means success.
//
//   post(job)   copy the job into the slot and wake the thread (started by the first post)
//   wait()      block until the posted job has run; returns the kept error and clears it
//   join()      stop and join the thread; a later post starts a new one (the destructor joins too)
//
// The error kept for wait(): with Sticky = false every job overwrites it with its own result; with
// Sticky = true only a failing job does, so an error stays until one wait() has read it.
// The thread sees only its copy of the job: what a job may touch is the job type's business.
// One poster at a time: post / wait / join are called from one thread (or under the caller's lock).
// Plain C++17, no device headers.
#pragma once

#include <condition_variable>
#include <mutex>
#include <thread>

namespace pth {

template <class Job, class Err, bool Sticky = false>
class Worker {
public:
    ~Worker() { join(); }   // a process that exits without joining: an idle thread, stopped

    void post(const Job& j) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!th_.joinable()) th_ = std::thread([this] { loop(); });
        job_ = j;
        task_ = busy_ = true;
        cv_.notify_all();
    }
    Err wait() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !busy_; });
        const Err e = err_;
        err_ = Err{};
        return e;
    }
    void join() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
            cv_.notify_all();
        }
        if (th_.joinable()) th_.join();
        stop_ = false;
    }

private:
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return task_ || stop_; });
            if (stop_) return;
            task_ = false;
            const Job j = job_;
            lk.unlock();
            const Err e = j.run();
            lk.lock();
            if (!Sticky || e != Err{}) err_ = e;
            busy_ = false;
            cv_.notify_all();
        }
    }

    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool task_ = false, busy_ = false, stop_ = false;
    Err err_{};
    Job job_{};
};

}  // namespace pth
