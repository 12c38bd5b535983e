// pm_mutations.hip -- mutation printing kernels (Tree::printMutationsNew, src/panman.cpp:3699-4057)
// over the replayed rows of every node that k_replay_dfs / k_replay leave in HBM.
//
// A block's columns are in the forward walk's order (per position its gap slots, then its main
// character); a reverse-strand walk reads them backwards.  So the root coordinate of a cell
// (panMATCoordinateToGlobal, :3725-3806) comes from one count over the columns: `before[col]`, the
// characters of the root's held blocks before the column that are neither '-' nor 'x'.  In a
// block the root holds forward (or does not hold: no character counts) the coordinate is
// before[col]; in one it holds on the reverse strand it is the block's base plus the characters in
// the columns after the cell, before[lo] + before[hi] - before[col + 1].
//   k_mut_root_count / k_mut_root_map   the count per chunk of kMutChunk columns, then (after the
//                    scan of the chunks) `before` of every column
//   k_mut_count      one lane per nucleotide mutation of the batch: its elements
//   k_mut_classify   one lane per element: its column, the parent's character by the seqChar rules
//                    (:3810-3849), the kind of its entry and the coordinate it prints
//   k_mut_line_len   one workgroup per node: the bytes of its three lines
//   k_mut_write      one workgroup per line: head, name, then the node's entries of the line's kind
//                    at their scanned offsets, kMutRound entries a round with a carry
// Integer only; only vector stores.
#include "pm_bits.h"
#include "pm_cell.h"
#include "pm_dev.h"

namespace pm {
namespace {

__constant__ char kMutNuc[17] = "-ACMGRSVTWYHKDBN";           // getNucleotideFromCode
__constant__ char kMutHead[40] = "Substitutions:\tInsertions:\tDeletions:\t";
__constant__ int32_t kMutHeadAt[4] = {0, 15, 27, 38};

__device__ __forceinline__ bool real_char(char ch) { return ch != '-' && ch != 'x'; }

// the root's flag of column `col`: a character of a held block that is neither '-' nor 'x'
__device__ __forceinline__ bool root_flag(const MutArgs& a, int64_t col) {
    if (col >= a.columns || !a.col_held[col]) return false;
    return real_char(a.rows[(int64_t)a.row_of[a.root] * a.row_stride + col]);
}

__global__ __launch_bounds__(256) void k_mut_root_count(MutArgs a) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int64_t col = (int64_t)blockIdx.x * kMutChunk + threadIdx.x;
    uint32_t total;
    (void)block_exclusive_scan(root_flag(a, col) ? 1u : 0u, sh, total);
    if (threadIdx.x == 0) a.chunk[blockIdx.x] = (int64_t)total;
}

__global__ __launch_bounds__(256) void k_mut_root_map(MutArgs a) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int64_t col = (int64_t)blockIdx.x * kMutChunk + threadIdx.x;
    const uint32_t flag = root_flag(a, col) ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(flag, sh, total);
    if (col >= a.columns) return;
    const int32_t mine = (int32_t)a.chunk[blockIdx.x] + (int32_t)ex;
    a.before[col] = mine;
    if (col == a.columns - 1) a.before[a.columns] = mine + (int32_t)flag;
}

// elements of mutation g: the root's own list prints nothing (:3855)
__device__ __forceinline__ int32_t elements_of(const MutArgs& a, int64_t g) {
    const uint32_t info = a.mut_info[g], type = info & 7u;
    if (a.mut_node[g] == a.root) return 0;
    return type < 3u ? (int32_t)(info >> 4) : type == 3u ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_mut_count(MutArgs a, MutBatch b) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > b.m) return;
    b.elems[k] = k < b.m ? (int64_t)elements_of(a, b.m0 + k) : 0;
}

__global__ __launch_bounds__(256) void k_mut_classify(MutArgs a, MutBatch b) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= b.entries) return;
    const int64_t lo = mutation_of_element(b.elems, b.m, e);
    const int32_t j = (int32_t)(e - b.elems[lo]);
    const int64_t g = b.m0 + lo;
    const int32_t blk = a.mut_primary[g], pos = a.mut_position[g], gap = a.mut_gap[g];
    const uint32_t info = a.mut_info[g], type = info & 7u;
    MutEntry out{0, 0, '-', '-', 0};
    const int64_t col = cell_column(a.pos_off, a.main_col, a.gap_col, a.blocks, blk, pos, gap, j);
    if (col < 0 || col >= a.columns) {
        atomicOr(a.error, 1);
        b.entry[e] = out;
        return;
    }
    const int32_t v = a.mut_node[g], par = a.parent[v];
    const uint32_t hv = a.held[(int64_t)v * a.blocks + blk], hp = a.held[(int64_t)par * a.blocks + blk],
                   hr = a.held[(int64_t)a.root * a.blocks + blk];
    const char pc = a.rows[(int64_t)a.row_of[par] * a.row_stride + col];
    const char rc = a.rows[(int64_t)a.row_of[a.root] * a.row_stride + col];
    // seqChar of the parent: a slot has no held test; a main character of a forward block needs the
    // block held; of a reverse block it is the root's stored character (:3835)
    char old = '-';
    if (real_char(pc)) {
        if (gap != -1) old = pc;
        else if (!(hp & kMafHeld)) old = '-';
        else old = (hp & kMafForward) ? pc : rc;
    }
    const bool held = (hv & kMafHeld) != 0;
    uint8_t kind = 0;
    if (type == 0u) kind = held && real_char(old) ? 1 : 0;
    else if (type == 2u) kind = 2;
    else if (type == 1u) kind = 3;
    else if (type == 3u) kind = held ? 1 : 0;
    const bool root_held = (hr & kMafHeld) != 0;
    int32_t coord = a.before[col];
    if (root_held && !(hr & kMafForward)) coord = a.before[a.blk_lo[blk]] + a.before[a.blk_hi[blk]] - a.before[col + 1];
    const bool odd = type == 3u && kind == 1 && !real_char(old);
    out.coord1 = coord + 1;
    out.kind = kind;
    out.old_ch = old;
    out.new_ch = kMutNuc[(a.mut_nucs[g] >> (4 * (5 - j))) & 15u];
    out.flags = (uint8_t)((root_held && !real_char(rc) ? kMutGap : 0) | (odd ? kMutOdd : 0));
    b.entry[e] = out;
    if (odd) atomicAdd(a.odd, 1ull);
}

// " > " [g] [old] coord [new | old]
__device__ __forceinline__ uint32_t entry_len(const MutEntry& t) {
    return 3u + (t.flags & kMutGap) + (uint32_t)digits_of((uint32_t)t.coord1) + (t.kind == 1 ? 2u : 1u);
}

__device__ __forceinline__ void put_entry(char* p, const MutEntry& t) {
    p[0] = ' ';
    p[1] = '>';
    p[2] = ' ';
    p += 3;
    if (t.flags & kMutGap) *p++ = 'g';
    if (t.kind == 1) *p++ = t.old_ch;
    const int d = digits_of((uint32_t)t.coord1);
    put_digits(p, (uint32_t)t.coord1, d);
    p[d] = t.kind == 3 ? t.old_ch : t.new_ch;
}

__global__ __launch_bounds__(256) void k_mut_line_len(MutArgs a, MutBatch b) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int32_t s = blockIdx.x, v = b.v0 + s;
    const int64_t e0 = b.elems[b.node_mut[v] - b.m0], e1 = b.elems[b.node_mut[v + 1] - b.m0];
    uint32_t len[3] = {0, 0, 0};
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const MutEntry t = b.entry[e];
        const uint32_t el = entry_len(t);
        if (t.kind == 1) len[0] += el;
        if (t.kind == 2) len[1] += el;
        if (t.kind == 3) len[2] += el;
    }
    uint32_t sum[3];
    for (int k = 0; k < 3; ++k) (void)block_exclusive_scan(len[k], sh, sum[k]);
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;   // head, name, tab, entries, newline
        b.line_len[3 * (int64_t)s + k] = (int64_t)(kMutHeadAt[k + 1] - kMutHeadAt[k]) + (b.name_off[v + 1] - b.name_off[v]) + 1 +
                                         (int64_t)(k == 0 ? sum[0] : k == 1 ? sum[1] : sum[2]) + 1;
    }
    if (s == b.n - 1 && threadIdx.x == 3) b.line_len[3 * (int64_t)b.n] = 0;
}

__global__ __launch_bounds__(256) void k_mut_write(MutArgs a, MutBatch b) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int64_t line = blockIdx.x;
    const int32_t s = (int32_t)(line / 3), k = (int32_t)(line % 3), v = b.v0 + s;
    char* out = b.text + b.line_len[line];
    const int64_t len = b.line_len[line + 1] - b.line_len[line];
    const int32_t h0 = kMutHeadAt[k], hlen = kMutHeadAt[k + 1] - h0;
    const int64_t n0 = b.name_off[v], nlen = b.name_off[v + 1] - n0;
    if ((int32_t)threadIdx.x < hlen) out[threadIdx.x] = kMutHead[h0 + threadIdx.x];
    for (int64_t i = threadIdx.x; i < nlen; i += 256) out[hlen + i] = b.names[n0 + i];
    if (threadIdx.x == 0) {
        out[hlen + nlen] = '\t';
        out[len - 1] = '\n';
    }
    char* at = out + hlen + nlen + 1;
    const int64_t e0 = b.elems[b.node_mut[v] - b.m0], e1 = b.elems[b.node_mut[v + 1] - b.m0];
    for (int64_t r0 = e0; r0 < e1; r0 += kMutRound) {   // (uniform)
        const int64_t e = r0 + threadIdx.x;
        MutEntry t{0, 0, '-', '-', 0};
        if (e < e1) t = b.entry[e];
        const bool mine = t.kind == k + 1;
        uint32_t round;
        const uint32_t ex = block_exclusive_scan(mine ? entry_len(t) : 0u, sh, round);
        if (mine) put_entry(at + ex, t);
        at += round;
    }
}

}  // namespace

hipError_t launch_mut_root_map(pm_ctx* c, const MutArgs& a) {
    const int64_t chunks = (a.columns + kMutChunk - 1) / kMutChunk;
    if (chunks == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_mut_root_count, dim3((unsigned)chunks), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = exclusive_scan(c, a.chunk, a.chunk, chunks);
    if (e != hipSuccess) return e;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_mut_root_map, dim3((unsigned)chunks), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_mut_count(pm_ctx* c, const MutArgs& a, const MutBatch& b) {
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_mut_count, dim3(blocks_of(b.m + 1, 256)), dim3(256), 0, c->stream, a, b);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_mut_classify(pm_ctx* c, const MutArgs& a, const MutBatch& b) {
    if (b.entries == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_mut_classify, dim3(blocks_of(b.entries, 256)), dim3(256), 0, c->stream, a, b);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_mut_line_len(pm_ctx* c, const MutArgs& a, const MutBatch& b) {
    if (b.n == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_mut_line_len, dim3((unsigned)b.n), dim3(256), 0, c->stream, a, b);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_mut_write(pm_ctx* c, const MutArgs& a, const MutBatch& b) {
    if (b.n == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_mut_write, dim3(3u * (unsigned)b.n), dim3(256), 0, c->stream, a, b);
    timer_end(c, 3);
    return hipGetLastError();
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_mutations() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_mut_line_len));
}

}  // namespace pm
