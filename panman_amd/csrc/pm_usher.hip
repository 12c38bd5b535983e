// pm_usher.hip -- UShER MAT export kernels (panmanToUsher / getNodeDFS, src/panman2usher.cpp:282-604)
// over the replayed rows of every node that k_replay_dfs / k_replay leave in HBM, every block held
// forward at every node (the derived PanMAT of pm_every_node.h), so row v is the reference's running
// `sequence` after node v and a cell's position is its canonical column + 1.
//   k_usher_count    one lane per nucleotide mutation of the batch: its elements (the root's list
//                    counts; types 3 to 5 count 1)
//   k_usher_classify one lane per element: its column, ref from the pseudo-root row, par from the
//                    parent's row, the bit set of its new code; and its sort key (node, column)
//   k_usher_earlier  after the stable sort of the keys: an element whose sorted predecessor has the
//                    same key takes that element's `after` as par (usher_earlier_writers)
//   k_usher_sizes    one workgroup per node: L, the bytes of its wrapped muts, and 1 + varint_len(L) + L
//   k_usher_write    one workgroup per node: 12 varint(L), then its entries at their scanned offsets,
//                    kUsherRound entries a round with a carry
// Integer only; only vector stores.
#include <hipcub/hipcub.hpp>

#include "pm_bits.h"
#include "pm_cell.h"
#include "pm_dev.h"

namespace pm {
namespace {

// getCodeFromNucleotide of 'A' + k: 0 where it is no nucleotide ('-' and 'x' are 0 as well)
__constant__ uint8_t kUsherCode[26] = {1, 14, 2, 13, 0, 0, 4, 11, 0, 0, 12, 0, 3, 15, 0, 0, 0, 5, 6, 8, 0, 7, 9, 0, 10, 0};

__device__ __forceinline__ uint8_t code_of(char ch) {
    const uint32_t k = (uint32_t)(uint8_t)ch - (uint32_t)'A';
    return k < 26u ? kUsherCode[k] : (uint8_t)0;
}

__device__ __forceinline__ uint32_t varint_len(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }

__device__ __forceinline__ char* put_varint(char* p, uint32_t v) {
    while (v >= 128u) {
        *p++ = (char)(uint8_t)(v | 128u);
        v >>= 7;
    }
    *p++ = (char)(uint8_t)v;
    return p;
}

__device__ __forceinline__ int32_t elements_of(uint32_t info) {
    const uint32_t type = info & 7u;
    return type < 3u ? (int32_t)(info >> 4) : type < 6u ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_usher_count(UsherArgs a, UsherBatch b) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > b.m) return;
    b.elems[k] = k < b.m ? (int64_t)elements_of(a.mut_info[b.m0 + k]) : 0;
}

__global__ __launch_bounds__(256) void k_usher_classify(UsherArgs a, UsherBatch b) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= b.entries) return;
    const int64_t lo = mutation_of_element(b.elems, b.m, e);
    const int32_t j = (int32_t)(e - b.elems[lo]);
    const int64_t g = b.m0 + lo;
    const int32_t blk = a.mut_primary[g], pos = a.mut_position[g], gap = a.mut_gap[g];
    const uint32_t type = a.mut_info[g] & 7u;
    const int32_t rank = a.mut_rank[g];
    const uint64_t node_key = (uint64_t)(uint32_t)(rank - b.r0) << 32;
    UsherEntry out{0, 0, 0, 15, 0};
    b.val[e] = (uint32_t)e;
    const int64_t col = cell_column(a.pos_off, a.main_col, a.gap_col, a.blocks, blk, pos, gap, j);
    if (col < 0 || col >= a.columns) {
        atomicOr(a.error, 1);
        b.entry[e] = out;
        b.key[e] = node_key;
        return;
    }
    const int32_t prow = a.par_row[rank];
    const bool del = type == 1u || type == 5u;
    const uint32_t code = (a.mut_nucs[g] >> (4 * (5 - j))) & 15u;
    out.position = (int32_t)(a.cell_base[blk] + (col - a.blk_lo[blk])) + 1;
    out.ref = code_of(a.pseudo[col]);
    out.par = code_of(prow < 0 ? a.pseudo[col] : a.rows[(int64_t)prow * a.row_stride + col]);
    out.set = (uint8_t)(del || code == 0u ? 15u : code);
    out.after = (uint8_t)(del ? 0u : code);
    b.entry[e] = out;
    b.key[e] = node_key | (uint64_t)col;
}

__global__ __launch_bounds__(256) void k_usher_earlier(const uint64_t* key, const uint32_t* val, int64_t n, UsherEntry* entry) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (i >= n || key[i] != key[i - 1]) return;
    // (equal keys stay in element order: val[i - 1] is the last earlier writer, and its `after` is final,
    // only `par` is written here)
    entry[val[i]].par = entry[val[i - 1]].after;
}

// 0a len [08 position] [10 ref] [18 par] 22 n b..
__device__ __forceinline__ uint32_t body_len(const UsherEntry& t) {
    return 1u + varint_len((uint32_t)t.position) + (t.ref ? 2u : 0u) + (t.par ? 2u : 0u) + 2u + (uint32_t)__popc((uint32_t)t.set);
}

__device__ __forceinline__ void put_entry(char* p, const UsherEntry& t) {
    *p++ = 0x0a;
    *p++ = (char)body_len(t);
    *p++ = 0x08;
    p = put_varint(p, (uint32_t)t.position);
    if (t.ref) {
        *p++ = 0x10;
        *p++ = (char)t.ref;
    }
    if (t.par) {
        *p++ = 0x18;
        *p++ = (char)t.par;
    }
    *p++ = 0x22;
    *p++ = (char)__popc((uint32_t)t.set);
    for (int k = 0; k < 4; ++k)
        if (t.set >> k & 1) *p++ = (char)k;
}

__global__ __launch_bounds__(256) void k_usher_sizes(UsherArgs a, UsherBatch b) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int32_t s = blockIdx.x, rank = b.r0 + s;
    const int64_t e0 = b.elems[a.rank_mut[rank] - b.m0], e1 = b.elems[a.rank_mut[rank + 1] - b.m0];
    uint32_t len = 0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) len += 2u + body_len(b.entry[e]);
    uint32_t L;
    (void)block_exclusive_scan(len, sh, L);
    if (threadIdx.x == 0) {
        b.list_len[s] = L;
        b.node_off[s] = (int64_t)1 + varint_len(L) + L;
        if (s == b.n - 1) b.node_off[b.n] = 0;
    }
}

__global__ __launch_bounds__(256) void k_usher_write(UsherArgs a, UsherBatch b) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int32_t s = blockIdx.x, rank = b.r0 + s;
    const uint32_t L = b.list_len[s];
    char* at = b.out + b.node_off[s];
    if (threadIdx.x == 0) {
        at[0] = 0x12;
        (void)put_varint(at + 1, L);
    }
    at += 1 + varint_len(L);
    const int64_t e0 = b.elems[a.rank_mut[rank] - b.m0], e1 = b.elems[a.rank_mut[rank + 1] - b.m0];
    for (int64_t r0 = e0; r0 < e1; r0 += kUsherRound) {   // (uniform)
        const int64_t e = r0 + threadIdx.x;
        const bool mine = e < e1;
        UsherEntry t{0, 0, 0, 0, 0};
        if (mine) t = b.entry[e];
        uint32_t round;
        const uint32_t ex = block_exclusive_scan(mine ? 2u + body_len(t) : 0u, sh, round);
        if (mine) put_entry(at + ex, t);
        at += round;
    }
}

template <class K, class... A>
hipError_t launch(pm_ctx* c, K kernel, int64_t blocks, A... args) {
    if (blocks == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, args...);
    timer_end(c, 3);
    return hipGetLastError();
}

}  // namespace

static_assert(kUsherRound == 256, "k_usher_write: one entry per lane of a 256-thread workgroup a round");

hipError_t launch_usher_count(pm_ctx* c, const UsherArgs& a, const UsherBatch& b) {
    return launch(c, k_usher_count, blocks_of(b.m + 1, 256), a, b);
}

hipError_t launch_usher_classify(pm_ctx* c, const UsherArgs& a, const UsherBatch& b) {
    return b.entries ? launch(c, k_usher_classify, blocks_of(b.entries, 256), a, b) : hipSuccess;
}

hipError_t usher_earlier_writers(pm_ctx* c, const UsherBatch& b) {
    if (b.entries < 2) return hipSuccess;
    int end_bit = 32;   // the column, then the bits of the batch's node indices
    while (end_bit < 64 && ((uint64_t)1 << (end_bit - 32)) < (uint64_t)b.n) ++end_bit;
    hipcub::DoubleBuffer<uint64_t> keys(b.key, b.key_alt);
    hipcub::DoubleBuffer<uint32_t> vals(b.val, b.val_alt);
    Dev<char> tmp;
    size_t bytes = 0;
    hipError_t err = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys, vals, (int)b.entries, 0, end_bit, c->stream);
    if (err == hipSuccess) err = tmp.alloc(bytes, false, c->stream);
    if (err == hipSuccess) {
        timer_begin(c, 3);
        err = hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, keys, vals, (int)b.entries, 0, end_bit, c->stream);
        timer_end(c, 3);
    }
    if (err == hipSuccess) err = launch(c, k_usher_earlier, blocks_of(b.entries - 1, 256), keys.Current(), vals.Current(), b.entries, b.entry);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);   // (tmp is released on return)
    return err;
}

hipError_t launch_usher_sizes(pm_ctx* c, const UsherArgs& a, const UsherBatch& b) { return launch(c, k_usher_sizes, b.n, a, b); }

hipError_t launch_usher_write(pm_ctx* c, const UsherArgs& a, const UsherBatch& b) { return launch(c, k_usher_write, b.n, a, b); }

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_usher() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_usher_sizes));
}

}  // namespace pm
