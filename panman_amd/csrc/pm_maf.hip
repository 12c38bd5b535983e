// pm_maf.hip -- MAF (m-WGA) extraction kernels (Tree::printMAF, src/maf.cpp:68-188) over the
// replayed rows that k_replay_dfs / k_replay leave in HBM.
//
// row(t, b) = rows[t][blk_lo[b] .. blk_hi[b]) is what getBlockSequenceFromReference
// (src/panman.cpp:3070-3261) builds for tip t and block b: per main position its gap slots,
// then its main character, the end sentinel 'x' last.  The MAF prints it with 'x' as '-'.
//   k_maf_size      per (tip, block) the characters that are neither '-' nor 'x': 16-byte row
//                   loads with the head and tail masked, G lanes per item (4, 16 or a wave)
//   k_maf_start     per tip (one wave) the exclusive scan of the sizes over the tip's print
//                   order, its total (srcSize) and the circular adjustment
//   k_maf_line_len  per (printed block rank, tip) the bytes of its "s" line, the group's "a\n"
//                   and closing "\n" folded into the group's first and last entry
//   k_maf_write     one workgroup per (line, kMafChunk body bytes): prefix, body with x -> -,
//                   16-byte non-temporal stores on the text's own 16-byte grid
// Only vector stores and ordinary atomics.
#include "pm_bits.h"
#include "pm_dev.h"

namespace pm {
namespace {

// 0x80 in every byte of w that equals the byte repeated in `pat` (exact: no borrow between bytes)
__device__ __forceinline__ uint32_t bytes_equal(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// 0xff in the bytes [from, to) of a dword (0 <= from, to <= 4 after clamping)
__device__ __forceinline__ uint32_t byte_span(int64_t from, int64_t to) {
    const int f = (int)(from < 0 ? 0 : from > 4 ? 4 : from), t = (int)(to < 0 ? 0 : to > 4 ? 4 : to);
    if (t <= f) return 0;
    const uint32_t upto_t = t == 4 ? ~0u : (1u << (8 * t)) - 1u;
    return upto_t & ~((1u << (8 * f)) - 1u);   // (f < 4 here)
}

// ungapped characters among the row columns [lo, hi) of the 16 bytes v at column `at`
__device__ __forceinline__ uint32_t ungapped16(const uint4& v, int64_t at, int64_t lo, int64_t hi) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t gap = bytes_equal(w[k], 0x2d2d2d2du) | bytes_equal(w[k], 0x78787878u);
        n += __popc(~gap & 0x80808080u & byte_span(lo - (at + 4 * k), hi - (at + 4 * k)));
    }
    return n;
}

// G lanes per (tip, block) item, 64 / G items per wave; a lane reads the 16-byte row words
// sl, sl + G, ... of the item's aligned window (blk_lo sits on no 16-byte grid).
template <int G>
__global__ __launch_bounds__(256) void k_maf_size(MafArgs a, const int32_t* cls_blk, int32_t n) {
    constexpr int kPerWave = kWave / G;
    const int lane = threadIdx.x & 63, sub = lane / G, sl = lane % G;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t items = (int64_t)a.tips * n;
    if (wave * kPerWave >= items) return;   // (wave-uniform)
    const int64_t item = wave * kPerWave + sub;
    bool live = item < items;
    int64_t slot = 0, lo = 0, hi = 0;
    const char* row = nullptr;
    if (live) {
        const int64_t tip = item / n;
        const int32_t blk = cls_blk[item % n];
        slot = tip * a.blocks + blk;
        live = (a.held[slot] & kMafHeld) != 0;   // (size is zeroed before the launch)
        lo = a.blk_lo[blk];
        hi = a.blk_hi[blk];
        row = a.rows + tip * a.row_stride;
    }
    uint32_t cnt = 0;
    if (live)
        for (int64_t at = (lo & ~(int64_t)15) + 16 * sl; at < hi; at += 16 * G)
            cnt += ungapped16(*reinterpret_cast<const uint4*>(row + at), at, lo, hi);
#pragma unroll
    for (int d = G / 2; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if (live && sl == 0) a.size[slot] = (int32_t)cnt;
}

// One wave per tip: srcSize, then 64 print positions a round with a carry.
__global__ __launch_bounds__(256) void k_maf_start(MafArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t tip = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (tip >= a.tips) return;   // (wave-uniform)
    const int32_t* order = a.order + tip * a.blocks;
    const int32_t* size = a.size + tip * a.blocks;
    uint32_t total = 0;
    for (int32_t i = lane; i < a.blocks; i += kWave) total += (uint32_t)size[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) total += __shfl_xor(total, d, 64);
    const int32_t offset = a.circular[tip];
    uint32_t carry = 0;
    for (int32_t i0 = 0; i0 < a.blocks; i0 += kWave) {
        const int32_t i = i0 + lane;
        const int32_t blk = i < a.blocks ? order[i] : -1;
        const uint32_t v = blk >= 0 ? (uint32_t)size[blk] : 0u;
        uint32_t round;
        const uint32_t ex = wave_exclusive_scan(v, round);
        if (blk >= 0 && (a.held[tip * a.blocks + blk] & kMafHeld)) {
            int32_t st = (int32_t)(carry + ex);
            if (offset >= 0) {   // (maf.cpp:125-136: one conditional add, not a modulo)
                st -= offset;
                if (st < 0) st += (int32_t)total;
            }
            a.start[tip * a.blocks + blk] = st;
        }
        carry += round;
    }
    if (lane == 0) a.src_size[tip] = (int32_t)total;
}

__device__ __forceinline__ int signed_width(int32_t v) {
    return v < 0 ? 1 + digits_of((uint32_t)(-(int64_t)v)) : digits_of((uint32_t)v);
}

// "s\t" name "\t" start "\t" size "\t" strand "\t" srcSize "\t"
__device__ __forceinline__ int64_t prefix_len(const MafArgs& a, int64_t tip, int64_t slot) {
    return 8 + (a.name_off[tip + 1] - a.name_off[tip]) + signed_width(a.start[slot]) + digits_of((uint32_t)a.size[slot]) +
           digits_of((uint32_t)a.src_size[tip]);
}

__global__ __launch_bounds__(256) void k_maf_line_len(MafArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.ranks * a.tips) return;
    const int64_t rank = e / a.tips, tip = e % a.tips;
    const int32_t blk = a.rank_blk[rank];
    const int64_t slot = tip * a.blocks + blk;
    int64_t len = 0;
    if (a.held[slot] & kMafHeld) len = prefix_len(a, tip, slot) + (a.blk_hi[blk] - a.blk_lo[blk]) + 1;
    const uint32_t fold = a.rank_fold[rank];
    if ((fold & kMafOpens) && tip == 0) len += 2;
    if ((fold & kMafCloses) && tip == a.tips - 1) len += 1;
    a.line_len[e] = len;
}

// decimal digits of v at p[0 .. d), lane k writing digit k
__device__ __forceinline__ void put_number(char* p, uint32_t v, int d, int lane) {
    if (lane >= d) return;
    uint32_t q = v;
    for (int k = d - 1; k > lane; --k) q /= 10;
    p[lane] = (char)('0' + q % 10);
}

__device__ __forceinline__ uint32_t x_to_dash(uint32_t w) {   // 'x' (0x78) -> '-' (0x2d)
    return w ^ ((bytes_equal(w, 0x78787878u) >> 7) * 0x55u);
}

// The 16 row bytes at s (any alignment) from the two aligned words around it; `k` dwords and
// `b` bytes of shift are the same for every lane of the workgroup (rows start on the 16-byte
// grid and a chunk's units are 16 bytes apart), so the switch is uniform.
__device__ __forceinline__ uint4 load16_shifted(const char* s, const char* row_end, int k, int b) {
    const char* s0 = s - (4 * k + b);
    const uint4 q0 = *reinterpret_cast<const uint4*>(s0);
    uint4 q1 = make_uint4(0, 0, 0, 0);
    if ((k | b) && s0 + 16 < row_end) q1 = *reinterpret_cast<const uint4*>(s0 + 16);
    const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint4 o;
#define PM_MAF_PICK(K)                                                \
    o.x = __builtin_amdgcn_alignbyte(w[K + 1], w[K], (uint32_t)b);     \
    o.y = __builtin_amdgcn_alignbyte(w[K + 2], w[K + 1], (uint32_t)b); \
    o.z = __builtin_amdgcn_alignbyte(w[K + 3], w[K + 2], (uint32_t)b); \
    o.w = __builtin_amdgcn_alignbyte(w[K + 4], w[K + 3], (uint32_t)b);
    switch (k) {
        case 0: PM_MAF_PICK(0) break;
        case 1: PM_MAF_PICK(1) break;
        case 2: PM_MAF_PICK(2) break;
        default: {
            o.x = __builtin_amdgcn_alignbyte(w[4], w[3], (uint32_t)b);
            o.y = __builtin_amdgcn_alignbyte(w[5], w[4], (uint32_t)b);
            o.z = __builtin_amdgcn_alignbyte(w[6], w[5], (uint32_t)b);
            o.w = __builtin_amdgcn_alignbyte(w[7], w[6], (uint32_t)b);   // (b = 0..3: w[7]'s top bytes at most)
        }
    }
#undef PM_MAF_PICK
    return o;
}

// One workgroup per (entry, body chunk).  The first chunk's first wave writes the folded "a\n"
// and the prefix; every chunk copies its kMafChunk body bytes -- the head and tail up to the
// text's 16-byte grid byte by byte, the units between as one non-temporal 16-byte store each;
// the last chunk closes the line and writes the folded "\n".
__global__ __launch_bounds__(256) void k_maf_write(MafArgs a, MafBatch bt) {
    // (scalar) the rank whose workgroups hold blockIdx.x
    const int32_t wg = (int32_t)blockIdx.x;
    int32_t klo = 0, khi = bt.nr - 1;
    while (klo < khi) {
        const int32_t mid = (klo + khi + 1) >> 1;
        if (bt.wg_off[mid] <= wg) klo = mid;
        else khi = mid - 1;
    }
    const int64_t rank = (int64_t)bt.rank0 + klo;
    const int32_t blk = a.rank_blk[rank];
    const int64_t lo = a.blk_lo[blk], width = a.blk_hi[blk] - lo;
    const int32_t chunks = maf_chunks(width);
    const int64_t first = rank * a.tips > bt.e0 ? rank * a.tips : bt.e0;   // the rank's first entry in the batch
    const int32_t local = wg - bt.wg_off[klo];
    const int64_t e = first + local / chunks;
    const int32_t chunk = local % chunks;
    const int64_t tip = e - rank * a.tips;
    const int64_t slot = tip * a.blocks + blk;
    const uint32_t held = a.held[slot];
    const uint32_t fold = a.rank_fold[rank];
    const bool opens = (fold & kMafOpens) && tip == 0, closes = (fold & kMafCloses) && tip == a.tips - 1;
    char* out = bt.text + bt.line_off[e - bt.e0];
    const int lane = threadIdx.x & 63;
    if (chunk == 0 && threadIdx.x == 0 && opens) {
        out[0] = 'a';
        out[1] = '\n';
    }
    if (opens) out += 2;
    if (!(held & kMafHeld)) {
        if (chunk == 0 && threadIdx.x == 0 && closes) out[0] = '\n';
        return;
    }
    const int32_t start = a.start[slot];
    const uint32_t size = (uint32_t)a.size[slot], src = (uint32_t)a.src_size[tip];
    const int64_t n0 = a.name_off[tip], nlen = a.name_off[tip + 1] - n0;
    const int ws = signed_width(start), wz = digits_of(size), wr = digits_of(src);
    const int64_t plen = 8 + nlen + ws + wz + wr;
    if (chunk == 0 && threadIdx.x < kWave) {
        char* p = out;
        if (lane == 0) {
            p[0] = 's';
            p[1] = '\t';
            p[2 + nlen] = '\t';
        }
        for (int64_t k = lane; k < nlen; k += kWave) p[2 + k] = a.names[n0 + k];
        p += 3 + nlen;
        if (start < 0) {
            if (lane == 0) p[0] = '-';
            put_number(p + 1, (uint32_t)(-(int64_t)start), ws - 1, lane);
        } else {
            put_number(p, (uint32_t)start, ws, lane);
        }
        p += ws;
        put_number(p + 1, size, wz, lane);
        if (lane == 0) {
            p[0] = '\t';
            p[1 + wz] = '\t';
            p[2 + wz] = (held & kMafForward) ? '+' : '-';
            p[3 + wz] = '\t';
            p[4 + wz + wr] = '\t';
        }
        put_number(p + 4 + wz, src, wr, lane);
    }
    char* body = out + plen;
    const char* row = a.rows + tip * a.row_stride;
    const char* srow = row + lo;
    const int64_t b0 = (int64_t)chunk * kMafChunk, b1 = b0 + kMafChunk < width ? b0 + kMafChunk : width;
    if (chunk == chunks - 1 && threadIdx.x == 0) {
        body[width] = '\n';
        if (closes) body[width + 1] = '\n';
    }
    // the text buffer starts on the 16-byte grid: align by the offset inside it
    const int64_t d0 = (body - bt.text) + b0, d1 = (body - bt.text) + b1;
    int64_t a0 = (d0 + 15) & ~(int64_t)15, a1 = d1 & ~(int64_t)15;
    if (a1 < a0) a0 = a1 = d1;   // (no whole unit: everything is head)
    const int64_t shift = (body - bt.text);   // text offset of body byte 0
    // head [d0, a0) and tail [a1, d1): fewer than 16 bytes each (or the whole short chunk)
    for (int64_t d = d0 + threadIdx.x; d < a0; d += 256) {
        const char ch = srow[d - shift];
        bt.text[d] = ch == 'x' ? '-' : ch;
    }
    for (int64_t d = a1 + threadIdx.x; d < d1; d += 256) {
        const char ch = srow[d - shift];
        bt.text[d] = ch == 'x' ? '-' : ch;
    }
    const int64_t units = (a1 - a0) >> 4;
    if (units <= 0) return;
    const char* s_first = srow + (a0 - shift);
    const int sh = (int)((lo + (a0 - shift)) & 15);   // (rows start on the 16-byte grid)
    const int k = __builtin_amdgcn_readfirstlane(sh >> 2), b = __builtin_amdgcn_readfirstlane(sh & 3);
    const char* row_end = row + a.row_stride;
    for (int64_t u = threadIdx.x; u < units; u += 256) {
        uint4 v = load16_shifted(s_first + 16 * u, row_end, k, b);
        v.x = x_to_dash(v.x);
        v.y = x_to_dash(v.y);
        v.z = x_to_dash(v.z);
        v.w = x_to_dash(v.w);
        store_stream(reinterpret_cast<uint4*>(bt.text + a0 + 16 * u), v);
    }
}

}  // namespace

hipError_t launch_maf_size(pm_ctx* c, const MafArgs& a, const int32_t* cls_blk, int32_t n, int lanes) {
    if (n == 0 || a.tips == 0) return hipSuccess;
    const int64_t items = (int64_t)a.tips * n;
    const int64_t waves = (items + kWave / lanes - 1) / (kWave / lanes);
    if (waves > (int64_t)0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid(blocks_of(waves, kWavesPerBlock));
    timer_begin(c, 3);
    if (lanes == 4) hipLaunchKernelGGL(k_maf_size<4>, grid, dim3(256), 0, c->stream, a, cls_blk, n);
    else if (lanes == 16) hipLaunchKernelGGL(k_maf_size<16>, grid, dim3(256), 0, c->stream, a, cls_blk, n);
    else hipLaunchKernelGGL(k_maf_size<64>, grid, dim3(256), 0, c->stream, a, cls_blk, n);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_maf_start(pm_ctx* c, const MafArgs& a) {
    if (a.tips == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_maf_start, dim3(blocks_of(a.tips, kWavesPerBlock)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_maf_line_len(pm_ctx* c, const MafArgs& a) {
    const int64_t entries = (int64_t)a.ranks * a.tips;
    if (entries == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_maf_line_len, dim3(blocks_of(entries, 256)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_maf_write(pm_ctx* c, const MafArgs& a, const MafBatch& b, int32_t workgroups) {
    if (workgroups <= 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_maf_write, dim3((unsigned)workgroups), dim3(256), 0, c->stream, a, b);
    timer_end(c, 3);
    return hipGetLastError();
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_maf() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_maf_line_len));
}

}  // namespace pm
