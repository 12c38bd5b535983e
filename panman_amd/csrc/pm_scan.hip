// pm_scan.hip -- the exclusive prefix sum of the extraction drivers (pm_vcf, pm_maf, pm_gfa):
// event, record and line counts into offsets, by hipCUB's device scan.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "pm_dev.h"

namespace pm {

namespace {

__global__ void k_scan_loaded() {}

}  // namespace

// out[0 .. n) = exclusive scan of in[0 .. n); in == out scans in place.  Synchronous on the
// context's stream.
hipError_t exclusive_scan(pm_ctx* c, const int64_t* in, int64_t* out, int64_t n) {
    if (n == 0) return hipSuccess;
    Dev<char> tmp;
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, c->stream);
    if (e == hipSuccess) e = tmp.alloc(bytes, false, c->stream);
    if (e == hipSuccess) {
        timer_begin(c, 3);
        e = hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, (int)n, c->stream);
        timer_end(c, 3);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_scan() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_scan_loaded));
}

}  // namespace pm
