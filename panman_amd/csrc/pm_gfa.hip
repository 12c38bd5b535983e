// pm_gfa.hip -- GFA extraction kernels (Tree::convertToGFA, src/gfa.cpp:119-499) over the
// replayed rows that k_replay_dfs / k_replay leave in HBM.
//
// The reference cuts every held block of every tip into chunks of 32 columns, strips '-' and
// 'x', and keeps a std::map<(start, string)> of the chunks under one mutex.  Here:
//   k_gfa_chunk     one lane per (tip, block, chunk): its up-to-32 columns (aligned dword loads,
//                   shifted: blk_lo sits on no grid), the survivors as 4-bit codes in 128 bits;
//                   the key (start code, length, string) and a non-empty flag
//   k_gfa_compact   the flagged items, numbered by the scan of the flags, become the steps
//   gfa_sort        a stable LSD radix sort of the step permutation over the key's three
//                   64-bit pieces (hipcub), so equal keys are neighbours in step order
//   k_gfa_heads     run heads by comparing whole keys with the left neighbour; a run's head is
//                   its earliest step, the node's creator
//   k_gfa_runs / k_gfa_ids   the scan of the creators in step order is the reference's
//                   insertion-order id; every step of a run receives it
//   k_gfa_step_len / k_gfa_line_len / k_gfa_write   the "P" lines: per step the bytes of its
//                   printed id, sign and comma, a scan, and one lane per step writing them
// Only vector stores.
#include <hipcub/hipcub.hpp>

#include "pm_bits.h"
#include "pm_dev.h"

namespace pm {
namespace {

// 4-bit code of a row character ("-ACMGRSVTWYHKDBN"[code]); letters only
__device__ __forceinline__ uint32_t code_of(uint32_t ch) {
    const uint32_t i = (ch - 'A') & 31u;
    const uint64_t tab = i < 16 ? 0x00F30C00B400D2E1ull : 0x0000000A09708650ull;
    return (uint32_t)(tab >> (4 * (i & 15u))) & 15u;
}

__global__ __launch_bounds__(256) void k_gfa_chunk(GfaArgs a) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= a.items) return;
    const int64_t tip = item / a.chunks;
    const int32_t slot = (int32_t)(item % a.chunks);
    const int32_t blk = a.chunk_blk[slot];
    const uint32_t held = a.held[tip * a.blocks + blk];
    if (!(held & kMafHeld)) {
        a.flag[item] = 0;
        return;
    }
    const bool forward = (held & kMafForward) != 0;
    const int64_t c = slot - a.chunk_off[blk];
    const int64_t lo = a.blk_lo[blk], hi = a.blk_hi[blk];
    int64_t c0, c1;   // the chunk's columns [c0, c1)
    if (forward) {
        c0 = lo + kGfaNode * c;
        c1 = c0 + kGfaNode < hi ? c0 + kGfaNode : hi;
    } else {   // anchored at the block's end
        c1 = hi - kGfaNode * c;
        c0 = c1 - kGfaNode > lo ? c1 - kGfaNode : lo;
    }
    // rows start on the 16-byte grid and row_stride is a multiple of 16: the aligned dwords
    // that cover [c0, c1) lie inside the row
    const char* row = a.rows + tip * a.row_stride;
    const int64_t w0 = c0 & ~(int64_t)3;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(row + w0);
    const uint32_t shift = (uint32_t)(c0 & 3);
    const int n = (int)(c1 - c0);
    uint64_t s_hi = 0, s_lo = 0;
    uint32_t len = 0;
    uint32_t prev = w[0];
#pragma unroll
    for (int k = 0; k < kGfaNode / 4; ++k) {
        if (4 * k >= n) break;
        const uint32_t next = w0 + 4 * (k + 1) < c1 ? w[k + 1] : 0u;
        const uint32_t word = __builtin_amdgcn_alignbyte(next, prev, shift);
        prev = next;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t ch = (word >> (8 * b)) & 0xffu;
            if (4 * k + b < n && ch != '-' && ch != 'x') {
                const uint64_t code = code_of(ch);
                if (len < 16) s_hi |= code << (60 - 4 * len);
                else s_lo |= code << (60 - 4 * (len - 16));
                ++len;
            }
        }
    }
    a.flag[item] = len ? 1 : 0;
    if (!len) return;
    const uint32_t start = a.start_code[(forward ? 0 : a.chunks) + slot];
    a.key[item] = ((uint64_t)start << 32) | len;
    a.key[a.items + item] = s_hi;
    a.key[2 * a.items + item] = s_lo;
}

__global__ __launch_bounds__(256) void k_gfa_compact(GfaArgs a, const int64_t* scan, GfaSteps s) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= a.items) return;
    const int64_t tip = item / a.chunks;
    const int32_t slot = (int32_t)(item % a.chunks);
    const int64_t at = scan[item];
    if (slot == 0) s.tip_off[tip] = (int32_t)at;
    if (item == a.items - 1) s.tip_off[a.tips] = (int32_t)(at + a.flag[item]);
    if (!a.flag[item]) return;
    s.key[at] = a.key[item];
    s.key[s.steps + at] = a.key[a.items + item];
    s.key[2 * s.steps + at] = a.key[2 * a.items + item];
    s.tip[at] = (int32_t)tip;
    s.forward[at] = (a.held[tip * a.blocks + a.chunk_blk[slot]] & kMafForward) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_gfa_iota(uint32_t* perm, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_gfa_gather(const uint64_t* piece, const uint32_t* perm, uint64_t* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = piece[perm[i]];
}

__global__ __launch_bounds__(256) void k_gfa_heads(GfaSteps s, const uint32_t* perm, int64_t* head, int64_t* creator) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.steps) return;
    const uint32_t p = perm[i];
    bool h = i == 0;
    if (!h) {
        const uint32_t q = perm[i - 1];
        h = s.key[p] != s.key[q] || s.key[s.steps + p] != s.key[s.steps + q] ||
            s.key[2 * s.steps + p] != s.key[2 * s.steps + q];
    }
    head[i] = h ? 1 : 0;
    if (h) creator[p] = 1;   // (creator is zeroed before the launch)
}

__global__ __launch_bounds__(256) void k_gfa_runs(GfaSteps s, const uint32_t* perm, const int64_t* head, const int64_t* hscan,
                                                  int32_t* run_first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.steps) return;
    if (head[i]) run_first[hscan[i]] = (int32_t)perm[i];
}

__global__ __launch_bounds__(256) void k_gfa_ids(GfaSteps s, const uint32_t* perm, const int64_t* head, const int64_t* hscan,
                                                 const int32_t* run_first, const int64_t* cscan, GfaNodes n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.steps) return;
    const uint32_t p = perm[i];
    const int64_t run = hscan[i] + head[i] - 1;
    const int64_t id = cscan[run_first[run]];
    s.id[p] = (int32_t)id;
    if (head[i]) {   // (p is the run's first step)
        n.key[id] = s.key[p];
        n.key[n.nodes + id] = s.key[s.steps + p];
        n.key[2 * n.nodes + id] = s.key[2 * s.steps + p];
        n.forward[id] = s.forward[p];
    }
}

__device__ __forceinline__ int32_t printed_of(const GfaText& t, int64_t s) { return t.printed[2 * (int64_t)t.id[s] + t.forward[s]]; }

// "<id><+|->," per kept step; the line's last kept step prints no comma (k_gfa_line_len)
__global__ __launch_bounds__(256) void k_gfa_step_len(GfaText t) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > t.steps) return;
    int64_t len = 0;
    if (s < t.steps) {
        const int32_t v = printed_of(t, s);
        if (v >= 0) len = digits_of((uint32_t)v) + 2;
    }
    t.step_len[s] = len;
}

// "P\t" name "\t" steps "\t*\n"
__global__ __launch_bounds__(256) void k_gfa_line_len(GfaText t) {
    const int64_t tip = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tip >= t.tips) return;
    const int64_t bytes = t.step_off[t.tip_off[tip + 1]] - t.step_off[t.tip_off[tip]];
    t.line_len[tip] = 6 + (t.name_off[tip + 1] - t.name_off[tip]) + (bytes > 0 ? bytes - 1 : 0);
}

// One lane per step of the tips [t0, t1), then one wave per line for its prefix and suffix.
__global__ __launch_bounds__(256) void k_gfa_write(GfaText t, int32_t t0, int32_t t1, const int64_t* line_off, char* text,
                                                   int64_t step_blocks) {
    if ((int64_t)blockIdx.x < step_blocks) {
        const int64_t s = t.tip_off[t0] + (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (s >= t.tip_off[t1]) return;
        const int32_t v = printed_of(t, s);
        if (v < 0) return;
        const int32_t tip = t.tip[s];
        const int64_t first = t.step_off[t.tip_off[tip]], last = t.step_off[t.tip_off[tip + 1]];
        char* p = text + line_off[tip - t0] + 3 + (t.name_off[tip + 1] - t.name_off[tip]) + (t.step_off[s] - first);
        const int d = digits_of((uint32_t)v);
        uint32_t q = (uint32_t)v;
        for (int k = d - 1; k >= 0; --k) {
            p[k] = (char)('0' + q % 10);
            q /= 10;
        }
        p[d] = t.forward[s] ? '+' : '-';
        if (t.step_off[s] + d + 2 != last) p[d + 1] = ',';   // a kept step follows
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t tip = t0 + ((int64_t)blockIdx.x - step_blocks) * kWavesPerBlock + (threadIdx.x >> 6);
    if (tip >= t1) return;   // (wave-uniform)
    char* p = text + line_off[tip - t0];
    const int64_t n0 = t.name_off[tip], nlen = t.name_off[tip + 1] - n0;
    for (int64_t k = lane; k < nlen; k += kWave) p[2 + k] = t.names[n0 + k];
    if (lane == 0) {
        p[0] = 'P';
        p[1] = '\t';
        p[2 + nlen] = '\t';
        char* e = p + t.line_len[tip] - 3;
        e[0] = '\t';
        e[1] = '*';
        e[2] = '\n';
    }
}

}  // namespace

hipError_t launch_gfa_chunk(pm_ctx* c, const GfaArgs& a) {
    if (a.items == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_chunk, dim3(blocks_of(a.items, 256)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_gfa_compact(pm_ctx* c, const GfaArgs& a, const int64_t* scan, const GfaSteps& s) {
    if (a.items == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_compact, dim3(blocks_of(a.items, 256)), dim3(256), 0, c->stream, a, scan, s);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t gfa_sort(pm_ctx* c, const GfaSteps& s, uint32_t* perm, uint64_t* scratch) {
    const int64_t n = s.steps;
    if (n == 0) return hipSuccess;
    // scratch: two key buffers, then two permutation buffers (32-bit entries)
    uint64_t *ka = scratch, *kb = scratch + n;
    uint32_t *pa = reinterpret_cast<uint32_t*>(scratch + 2 * n), *pb = reinterpret_cast<uint32_t*>(scratch + 3 * n);
    const dim3 grid(blocks_of(n, 256));
    Dev<char> tmp;
    size_t tmp_bytes = 0;
    hipcub::DoubleBuffer<uint64_t> keys(ka, kb);
    hipcub::DoubleBuffer<uint32_t> vals(pa, pb);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys, vals, (int)n, 0, 64, c->stream);
    if (e == hipSuccess) e = tmp.alloc(tmp_bytes, false, c->stream);
    timer_begin(c, 3);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gfa_iota, grid, dim3(256), 0, c->stream, vals.Current(), n);
        e = hipGetLastError();
    }
    for (int piece = 2; piece >= 0 && e == hipSuccess; --piece) {   // least significant piece first
        hipLaunchKernelGGL(k_gfa_gather, grid, dim3(256), 0, c->stream, s.key + (int64_t)piece * n, vals.Current(),
                           keys.Current(), n);
        e = hipGetLastError();
        // the low piece of (start code << 32 | length) and the string pieces use all 64 bits
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys, vals, (int)n, 0, 64, c->stream);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(perm, vals.Current(), sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream);
    timer_end(c, 3);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

hipError_t launch_gfa_heads(pm_ctx* c, const GfaSteps& s, const uint32_t* perm, int64_t* head, int64_t* creator) {
    if (s.steps == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_heads, dim3(blocks_of(s.steps, 256)), dim3(256), 0, c->stream, s, perm, head, creator);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_gfa_runs(pm_ctx* c, const GfaSteps& s, const uint32_t* perm, const int64_t* head, const int64_t* hscan,
                           int32_t* run_first) {
    if (s.steps == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_runs, dim3(blocks_of(s.steps, 256)), dim3(256), 0, c->stream, s, perm, head, hscan, run_first);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_gfa_ids(pm_ctx* c, const GfaSteps& s, const uint32_t* perm, const int64_t* head, const int64_t* hscan,
                          const int32_t* run_first, const int64_t* cscan, const GfaNodes& n) {
    if (s.steps == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_ids, dim3(blocks_of(s.steps, 256)), dim3(256), 0, c->stream, s, perm, head, hscan, run_first,
                       cscan, n);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_gfa_step_len(pm_ctx* c, const GfaText& t) {
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_step_len, dim3(blocks_of(t.steps + 1, 256)), dim3(256), 0, c->stream, t);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_gfa_line_len(pm_ctx* c, const GfaText& t) {
    if (t.tips == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_line_len, dim3(blocks_of(t.tips, 256)), dim3(256), 0, c->stream, t);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_gfa_write(pm_ctx* c, const GfaText& t, int32_t t0, int32_t t1, const int64_t* line_off, char* text,
                            int64_t batch_steps) {
    if (t1 <= t0) return hipSuccess;
    const int64_t step_blocks = (batch_steps + 255) / 256;
    const int64_t grid = step_blocks + (t1 - t0 + kWavesPerBlock - 1) / kWavesPerBlock;
    if (grid > (int64_t)0x7fffffff) return hipErrorInvalidValue;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_gfa_write, dim3((unsigned)grid), dim3(256), 0, c->stream, t, t0, t1, line_off, text, step_blocks);
    timer_end(c, 3);
    return hipGetLastError();
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_gfa() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_gfa_line_len));
}

}  // namespace pm
