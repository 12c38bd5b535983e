// pm_dev.h -- device-side plumbing shared by the extraction drivers (pm_replay.cpp's formatter,
// pm_vcf, pm_maf, pm_gfa, pm_summary): a scoped device array, the grid size of a launch, the
// download of a text batch into a sink and the wrappers of the C entry points; and by the
// construction drivers (pm_msa, pm_pangraph, pm_gfa_in, pm_reroot, pm_subnet; their host-only
// half is pm_build.h): the one-tree handle behind an entry point, a run over the uploaded columns
// and the fetch of its records.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "pm_internal.h"
#include "pm_panman_tree.h"
#include "pm_text.h"

namespace pm {

template <class T>
struct Dev {   // a device array released on scope exit
    T* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t n, bool zero, hipStream_t s) {
        reset();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * std::max<size_t>(n, 1));
        if (e != hipSuccess) p = nullptr;
        else if (zero) e = hipMemsetAsync(p, 0, sizeof(T) * std::max<size_t>(n, 1), s);
        return e;
    }
    hipError_t put(const T* v, size_t n, hipStream_t s) {
        hipError_t e = alloc(n, false, s);
        if (e == hipSuccess && n) e = hipMemcpyAsync(p, v, sizeof(T) * n, hipMemcpyHostToDevice, s);
        return e;
    }
    hipError_t put(const std::vector<T>& v, hipStream_t s) { return put(v.data(), v.size(), s); }
    hipError_t get(std::vector<T>& v, size_t n, hipStream_t s) const {
        v.resize(n);
        return n ? hipMemcpyAsync(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost, s) : hipSuccess;
    }
};

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

inline double seconds_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

// The sink of the *_fd entry points.
inline Sink fd_sink(int fd) {
    return [fd](const char* q, size_t n) { return write_all(fd, q, n); };
}

// A sink refused a piece of the `what` text ("VCF", "MAF", ...): errno says why.
inline int write_failed(pm_ctx* c, const char* what) {
    return fail(c, PM_ERR_ARG, std::string(what) + " write: " + std::strerror(errno));
}

// The first `bytes` of c->text_buf through the pinned download slots into `sink`; `written` and
// `t_down` (seconds) carry the driver's totals.
inline int stream_text(pm_ctx* c, const char* what, int64_t bytes, const Sink& sink, int64_t& written, double& t_down) {
    const auto t0 = std::chrono::steady_clock::now();
    bool wrote = true;
    const hipError_t e = d2h_stream(c, c->text_buf, (size_t)bytes, sink, wrote);
    if (e != hipSuccess) return hip_fail(c, e, (std::string(what) + " download").c_str());
    if (!wrote) return write_failed(c, what);
    t_down += seconds_since(t0);
    written += bytes;
    return PM_OK;
}

// run() behind a C entry point: the drivers' host vectors grow with leaves x blocks or with the
// record count, and an allocation failure must not leave through the C ABI.
template <class Run>
int guarded(pm_ctx* c, const char* what, Run&& run) {
    try {
        return run();
    } catch (const std::bad_alloc&) {
        return fail(c, PM_ERR_OOM, std::string(what) + " host buffers");
    }
}

// A handle-returning entry point over its driver: run(tree) fills the one tree of a new handle.
// On failure the handle is released and *out stays null.
template <class Run>
int build_handle(pm_ctx* c, const char* what, pm_panman** out, Run&& run) {
    *out = nullptr;
    (void)hipSetDevice(c->device);
    std::unique_ptr<pm_panman> res(new (std::nothrow) pm_panman());
    if (!res) return fail(c, PM_ERR_OOM, std::string(what) + " host buffers");
    const int rc = guarded(c, what, [&]() {
        res->trees.resize(1);
        return run(res->trees[0]);
    });
    if (rc == PM_OK) *out = res.release();
    return rc;
}

// Every record of the last run, sorted by (node, site).
inline int fetch_records(pm_ctx* c, std::vector<pm_mut>& recs) {
    int64_t n = 0;
    const int rc = pm_mutation_count(c, &n);
    if (rc != PM_OK) return rc;
    recs.resize((size_t)n);
    return n ? pm_mutations_fetch(c, recs.data(), n, &n) : PM_OK;
}

// One pass over the uploaded leaf columns: the sites' packed root parent codes (and forced root
// codes, or null), the run, the records.
inline int run_columns(pm_ctx* c, int mode, const std::vector<uint8_t>& cons4, const uint8_t* forced4, std::vector<pm_mut>& recs) {
    int rc;
    if ((rc = pm_sites_upload(c, cons4.data(), forced4)) != PM_OK || (rc = pm_run(c, mode)) != PM_OK) return rc;
    return fetch_records(c, recs);
}

// A buffer-returning entry point over its driver: run(sink) writes the text, *text receives it
// NUL-terminated (the caller's, released with free / pm_free).
template <class Run>
int collect_text(pm_ctx* c, const char* what, char** text, Run&& run) {
    TextCollector out;
    const int rc = guarded(c, what, [&]() { return run(out.sink()); });
    if (rc != PM_OK) return rc;
    if (!(*text = out.release())) return fail(c, PM_ERR_OOM, std::string(what) + " host buffers");
    return PM_OK;
}

}  // namespace pm
