// pm_hostpar.cpp -- host plumbing that needs no GPU: the phase log every driver writes its
// host / device phase times into (pm_phase_report), and the host worker threads
// (host_parallel_for over the pool of pm_pool.h).  No HIP header: the tree planner and its
// stand-alone check link this file alone.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "pm_plan.h"
#include "pm_pool.h"

namespace pm {

// ---- phase log ---------------------------------------------------------------------------
namespace {
std::mutex g_phase_mu;
std::vector<std::pair<std::string, double>> g_phases;
constexpr size_t kMaxPhases = 4096;
}  // namespace

void phase_add(const std::string& name, double seconds) {
    std::lock_guard<std::mutex> lock(g_phase_mu);
    if (g_phases.size() < kMaxPhases) g_phases.emplace_back(name, seconds);
}

PhaseClock::PhaseClock() : t(std::chrono::steady_clock::now()) {}

double PhaseClock::lap(const char* name) {
    const auto now = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(now - t).count();
    phase_add(name, s);
    t = now;
    return s;
}

void tree_phase(PhaseClock& clock, const char* what) {
    const double s = clock.lap((std::string("tree.") + what).c_str());
    // PM_UPLOAD_TIMING=1: host phase durations on stderr
    if (std::getenv("PM_UPLOAD_TIMING") != nullptr) std::fprintf(stderr, "[pm_tree_upload] %-16s %8.2f s\n", what, s);
}

int host_threads() {
    if (const char* e = std::getenv("PM_HOST_THREADS")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 256) return v;
    }
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(16u, hc ? hc : 1u));
}

void host_parallel_for(int tasks, const std::function<void(int)>& fn) {
    if (tasks <= 0) return;
    const int t = std::min(tasks, host_threads());
    if (t <= 1) {
        for (int i = 0; i < tasks; ++i) fn(i);
        return;
    }
    Pool pool(t);
    pool.run(tasks, fn);
}

}  // namespace pm

extern "C" {

void pm_phase_reset(void) {
    std::lock_guard<std::mutex> lock(pm::g_phase_mu);
    pm::g_phases.clear();
}

int64_t pm_phase_report(char* buf, int64_t len) {
    std::string s;
    {
        std::lock_guard<std::mutex> lock(pm::g_phase_mu);
        char line[64];
        for (auto& p : pm::g_phases) {
            std::snprintf(line, sizeof line, "\t%.6f\n", p.second);
            s += p.first;
            s += line;
        }
    }
    if (buf && len > 0) {
        const size_t n = std::min<size_t>(s.size(), (size_t)len - 1);
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int64_t)s.size() + 1;
}

}  // extern "C"
