// pm_aa.hip -- amino-acid translation kernels (Tree::extractAminoAcidTranslations,
// src/aaTrans.cpp:185-304) over the replayed rows of every node that k_replay_dfs / k_replay
// leave in HBM.
//
// A block's columns are in the forward walk's order (per position its gap slots, then its main
// character); a reverse-strand walk reads them backwards.  So a coordinate of
// globalCoordinateToBlockCoordinate (src/panman.cpp:5726-5798) is a column, and the window of
// getNucleotideSequenceFromBlockCoordinates (aaTrans.cpp:3-67) is a subset of the columns
// between two of them, each cell's membership decided from the cell alone.
//   k_aa_locate    one wave per node: the block of start and of end by a scan of the node's
//                  per-block sizes (k_maf_size), then a strand-aware rank-select inside that
//                  block by ballot and popcount
//   k_aa_codons    one workgroup per node: the walked cells kAaChunk a round; ballot ranks of the
//                  walked and of the A/C/G/T cells give every base its window index and its
//                  rank r; base r is stored, ranks 3c and 3c + 2 store codon c's start and end
//                  (so a codon may straddle rounds and blocks)
//   k_aa_line_len  one workgroup per node: the order-free form of the two-pointer merge
//                  (aaTrans.cpp:259-285) per codon, the bytes of the S, I and D entries
//   k_aa_write     one workgroup per line: the entries at their scanned offsets
// Integer only; only vector stores.
#include "pm_bits.h"
#include "pm_dev.h"

namespace pm {
namespace {

// the standard genetic code: the 64 codons in TCAG order, one letter each
__constant__ char kAaLetters[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
// the three-letter name of letter 'A' + k ("---": no amino acid)
__constant__ char kAaNames[79] = "Ala---CysAspGluPheGlyHisIle---LysLeuMetAsn---ProGlnArgSerThr---ValTrp---Tyr---";

__device__ __forceinline__ int base_code(char ch) { return ch == 'T' ? 0 : ch == 'C' ? 1 : ch == 'A' ? 2 : ch == 'G' ? 3 : -1; }

__device__ __forceinline__ char aa_letter(const uint8_t* base, int32_t c) {
    return kAaLetters[base[3 * (int64_t)c] * 16 + base[3 * (int64_t)c + 1] * 4 + base[3 * (int64_t)c + 2]];
}

__device__ __forceinline__ int name_len(char letter) { return letter == '*' ? 1 : 3; }

__global__ __launch_bounds__(256) void k_aa_locate(AaArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (v >= a.nodes) return;   // (wave-uniform)
    const int64_t row = a.row_of[v];
    const int32_t* size = a.size + row * a.blocks;
    const uint8_t* held = a.held + row * a.blocks;
    const char* r = a.rows + row * a.row_stride;
    uint32_t sum = 0;
    for (int32_t i = lane; i < a.blocks; i += kWave) sum += (uint32_t)size[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    const int64_t total = sum;
    AaSpan sp{-1, -1, -1, -1};
    for (int which = 0; which < 2; ++which) {
        int64_t g = which ? a.end : a.start;
        if (!(g < total)) g -= total;   // (panman.cpp:5750-5754: one wrap)
        if (g < 0 || g >= total) continue;
        // the block: per-block sizes 64 a round with a carry
        int64_t carry = 0, rem = 0;
        int32_t blk = -1;
        for (int32_t i0 = 0; i0 < a.blocks; i0 += kWave) {
            const int32_t i = i0 + lane;
            const uint32_t sz = i < a.blocks ? (uint32_t)size[i] : 0u;
            uint32_t round;
            const uint32_t ex = wave_exclusive_scan(sz, round);
            if (carry + round > g) {
                const bool mine = sz > 0 && carry + ex <= g && g < carry + ex + sz;
                const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;
                blk = i0 + src;
                rem = g - carry - (int64_t)(uint32_t)__shfl((int)ex, src, 64);
                break;
            }
            carry += round;
        }
        if (blk < 0) continue;
        // the rem-th character of the block in walk order
        const int64_t lo = a.blk_lo[blk], width = a.blk_hi[blk] - lo;
        const bool fwd = (held[blk] & kMafForward) != 0;
        int32_t found = -1;
        for (int64_t t0 = 0; t0 < width; t0 += kWave) {
            const int64_t t = t0 + lane;
            const int64_t col = fwd ? lo + t : lo + width - 1 - t;
            bool flag = false;
            if (t < width) {
                const char ch = r[col];
                flag = ch != '-' && ch != 'x';
            }
            const unsigned long long m = __ballot(flag);
            const int cnt = __popcll(m);
            if (rem < cnt) {
                const bool mine = flag && __popcll(m & ((1ull << lane) - 1ull)) == (int)rem;
                const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;
                found = __shfl((int)col, src, 64);
                break;
            }
            rem -= cnt;
        }
        if (which) {
            sp.ce = found;
            sp.b1 = blk;
        } else {
            sp.cs = found;
            sp.b0 = blk;
        }
    }
    if (lane == 0) a.span[v] = sp;
}

__global__ __launch_bounds__(256) void k_aa_codons(AaArgs a, AaTables t) {
    __shared__ int32_t s_stop;
    __shared__ uint32_t s_walk[kWavesPerBlock], s_base[kWavesPerBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = blockIdx.x;
    const int32_t v = t.node[s];
    const AaSpan sp = a.span[v];
    if (sp.cs < 0 || sp.ce < 0) {   // (uniform) not located: no table
        if (tid == 0) {
            t.codons[s] = 0;
            t.error[s] = 1;
        }
        return;
    }
    const int64_t row = a.row_of[v];
    const uint8_t* held = a.held + row * a.blocks;
    const char* r = a.rows + row * a.row_stride;
    uint8_t* base = t.base + s * t.base_cap;
    int32_t* cstart = t.cstart + s * t.codon_cap;
    int32_t* cend = t.cend + s * t.codon_cap;
    const int32_t mS = a.col_main[sp.cs];
    const int32_t k0 = sp.cs == mS ? -1 : sp.cs - a.col_first[sp.cs];
    uint32_t walked_before = 0, bases_before = 0;
    bool stopped = false;
    for (int32_t i = sp.b0; i <= sp.b1 && !stopped; ++i) {
        const int64_t lo = a.blk_lo[i], hi = a.blk_hi[i];
        if (hi <= lo) continue;   // an id that holds no block: no position
        const uint32_t h = held[i];
        const bool is_held = (h & kMafHeld) != 0, fwd = !is_held || (h & kMafForward) != 0;
        // the cells in walk order: column first + t (forward) or first - t (reverse), t < cells
        int64_t first, cells;
        if (fwd) {
            first = i == sp.b0 ? (int64_t)sp.cs : lo;
            cells = hi - first;
        } else {
            const int32_t top = i == sp.b0 ? mS : a.rev_top[i];
            if (top < 0) continue;   // (the driver refuses such a walk before this launch)
            first = top;
            cells = top - lo + 1;
        }
        for (int64_t t0 = 0; t0 < cells && !stopped; t0 += kAaChunk) {
            const int64_t tt = t0 + tid;
            const int64_t col = fwd ? first + tt : first - tt;
            bool walked = false;
            char ch = '-';
            if (tid == 0) s_stop = kAaChunk;
            __syncthreads();
            if (tt < cells) {
                const int32_t m = a.col_main[col];
                const int32_t k = col == m ? -1 : (int32_t)col - a.col_first[col];
                // forward: the slot loop starts at get<3>(start) in every position (aaTrans.cpp:17);
                // reverse: every slot, but those above get<3>(start) in the start position
                walked = fwd ? (k == -1 || (k0 >= 0 && k >= k0)) : !(i == sp.b0 && m == mS && k > k0);
                if (walked && col == sp.ce) s_stop = tid;   // (one cell at most)
                if (walked && is_held) ch = r[col];
            }
            __syncthreads();
            const int32_t stop = s_stop;
            walked = walked && tid < stop;
            const int code = walked ? base_code(ch) : -1;
            const unsigned long long wm = __ballot(walked), bm = __ballot(code >= 0);
            if (lane == 0) {
                s_walk[wave] = (uint32_t)__popcll(wm);
                s_base[wave] = (uint32_t)__popcll(bm);
            }
            __syncthreads();
            uint32_t w = walked_before, b = bases_before, w_all = 0, b_all = 0;
#pragma unroll
            for (int k = 0; k < kWavesPerBlock; ++k) {
                if (k < wave) {
                    w += s_walk[k];
                    b += s_base[k];
                }
                w_all += s_walk[k];
                b_all += s_base[k];
            }
            const unsigned long long below = (1ull << lane) - 1ull;
            w += (uint32_t)__popcll(wm & below);
            b += (uint32_t)__popcll(bm & below);
            if (code >= 0 && b < (uint32_t)t.base_cap) {
                base[b] = (uint8_t)code;
                const uint32_t c = b / 3u, part = b % 3u;
                if (c < (uint32_t)t.codon_cap) {
                    if (part == 0) cstart[c] = (int32_t)w;
                    if (part == 2) cend[c] = (int32_t)w;
                }
            }
            walked_before += w_all;
            bases_before += b_all;
            stopped = stop < kAaChunk;
            __syncthreads();   // (s_stop and the counts are rewritten next round)
        }
    }
    if (tid == 0) {
        const uint32_t whole = bases_before < (uint32_t)t.base_cap ? bases_before : (uint32_t)t.base_cap;
        const uint32_t codons = whole / 3u < (uint32_t)t.codon_cap ? whole / 3u : (uint32_t)t.codon_cap;
        t.codons[s] = stopped ? (int32_t)codons : 0;
        t.error[s] = stopped ? 0 : 1;
    }
}

// root codons that end before window index `at` (their ends ascend)
__device__ __forceinline__ int32_t ends_before(const int32_t* rend, int32_t n, int32_t at) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (rend[mid] < at) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct AaRoot {
    const uint8_t* base;
    const int32_t* cstart;
    const int32_t* cend;
    int32_t n;
};

// Codon a of a node against the root's codons: 'S' (a match whose amino acid differs), 'I', or 0
// (an equal match); `index` the root index it prints and `letter` its amino acid.
__device__ __forceinline__ char classify(const AaRoot& root, const uint8_t* base, const int32_t* cstart, int32_t a,
                                         int32_t& index, char& letter) {
    const int32_t at = cstart[a];
    const int32_t q = ends_before(root.cend, root.n, at);
    const bool inside = q < root.n && at >= root.cstart[q];
    bool taken = false;   // an earlier codon of the node matched q
    if (inside && a > 0) {
        const int32_t prev = cstart[a - 1];   // (starts ascend: the same q iff it does not end before `prev`)
        taken = prev >= root.cstart[q];
    }
    letter = aa_letter(base, a);
    if (inside && !taken) {
        index = q;
        return aa_letter(root.base, q) != letter ? 'S' : 0;
    }
    index = inside ? q + 1 : q;
    return 'I';
}

// root codon q matched by no codon of the node: the first codon that starts at or after q's start
// starts after q's end (or there is none)
__device__ __forceinline__ bool deleted(const AaRoot& root, const int32_t* cstart, int32_t n, int32_t q) {
    const int32_t from = root.cstart[q];
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cstart[mid] < from) lo = mid + 1;
        else hi = mid;
    }
    return lo == n || cstart[lo] > root.cend[q];
}

__device__ __forceinline__ uint32_t entry_len(char kind, int32_t index, char letter) {
    return kind ? 4u + (uint32_t)digits_of((uint32_t)index) + (uint32_t)name_len(letter) : 0u;   // "S:" idx ":" name ";"
}

__device__ __forceinline__ void put_entry(char* p, char kind, int32_t index, char letter) {
    const int d = digits_of((uint32_t)index);
    p[0] = kind;
    p[1] = ':';
    put_digits(p + 2, (uint32_t)index, d);
    p += 2 + d;
    if (kind == 'D') {
        p[0] = ';';
        return;
    }
    p[0] = ':';
    if (letter == '*') {
        p[1] = '*';
        p[2] = ';';
        return;
    }
    const char* nm = kAaNames + 3 * (letter - 'A');
    p[1] = nm[0];
    p[2] = nm[1];
    p[3] = nm[2];
    p[4] = ';';
}

struct AaSlot {
    AaRoot root;
    const uint8_t* base;
    const int32_t* cstart;
    int32_t n;        // the node's codons
    bool located;
};

__device__ __forceinline__ AaSlot slot_of(const AaArgs& a, const AaTables& root, const AaTables& t, int64_t s) {
    AaSlot o;
    o.root = AaRoot{root.base, root.cstart, root.cend, root.codons[0]};
    o.base = t.base + s * t.base_cap;
    o.cstart = t.cstart + s * t.codon_cap;
    o.n = t.codons[s];
    const AaSpan sp = a.span[t.node[s]];
    o.located = sp.cs >= 0 && sp.ce >= 0;
    return o;
}

__global__ __launch_bounds__(256) void k_aa_line_len(AaArgs a, AaTables root, AaTables t, AaText x) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int64_t s = blockIdx.x;
    const AaSlot o = slot_of(a, root, t, s);
    uint32_t len_s = 0, len_i = 0, len_d = 0;
    if (o.located) {
        for (int32_t c = threadIdx.x; c < o.n; c += 256) {
            int32_t index;
            char letter;
            const char kind = classify(o.root, o.base, o.cstart, c, index, letter);
            const uint32_t len = entry_len(kind, index, letter);
            if (kind == 'S') len_s += len;
            else len_i += len;
        }
        for (int32_t q = threadIdx.x; q < o.root.n; q += 256)
            if (deleted(o.root, o.cstart, o.n, q)) len_d += 3u + (uint32_t)digits_of((uint32_t)q);   // "D:" q ";"
    }
    uint32_t sum_s, sum_i, sum_d;
    (void)block_exclusive_scan(len_s, sh, sum_s);
    (void)block_exclusive_scan(len_i, sh, sum_i);
    (void)block_exclusive_scan(len_d, sh, sum_d);
    if (threadIdx.x == 0) {
        const int32_t v = t.node[s];
        const int64_t body = (int64_t)sum_s + sum_i + sum_d;
        x.line_len[s] = body ? (x.name_off[v + 1] - x.name_off[v]) + 2 + body : 0;   // name "\t" body "\n"
        x.sec[2 * s] = (int32_t)sum_s;
        x.sec[2 * s + 1] = (int32_t)sum_i;
    }
}

__global__ __launch_bounds__(256) void k_aa_write(AaArgs a, AaTables root, AaTables t, AaText x) {
    __shared__ uint32_t sh[kWavesPerBlock];
    const int64_t s = blockIdx.x;
    const int64_t len = x.line_len[s];
    if (len == 0) return;   // (uniform)
    const AaSlot o = slot_of(a, root, t, s);
    const int32_t v = t.node[s];
    const int64_t n0 = x.name_off[v], nlen = x.name_off[v + 1] - n0;
    char* out = x.text + x.line_off[s];
    for (int64_t k = threadIdx.x; k < nlen; k += 256) out[k] = x.names[n0 + k];
    if (threadIdx.x == 0) {
        out[nlen] = '\t';
        out[len - 1] = '\n';
    }
    char* at_s = out + nlen + 1;
    char* at_i = at_s + x.sec[2 * s];
    char* at_d = at_i + x.sec[2 * s + 1];
    // the node's codons 256 a round: S and I entries at their scanned offsets
    for (int32_t c0 = 0; c0 < o.n; c0 += 256) {
        const int32_t c = c0 + threadIdx.x;
        int32_t index = 0;
        char letter = 0, kind = 0;
        if (c < o.n) kind = classify(o.root, o.base, o.cstart, c, index, letter);
        const uint32_t el = entry_len(kind, index, letter);
        uint32_t round_s, round_i;
        const uint32_t ex_s = block_exclusive_scan(kind == 'S' ? el : 0u, sh, round_s);
        const uint32_t ex_i = block_exclusive_scan(kind == 'I' ? el : 0u, sh, round_i);
        if (kind == 'S') put_entry(at_s + ex_s, kind, index, letter);
        if (kind == 'I') put_entry(at_i + ex_i, kind, index, letter);
        at_s += round_s;
        at_i += round_i;
    }
    for (int32_t q0 = 0; q0 < o.root.n; q0 += 256) {
        const int32_t q = q0 + threadIdx.x;
        const bool del = q < o.root.n && deleted(o.root, o.cstart, o.n, q);
        uint32_t round;
        const uint32_t ex = block_exclusive_scan(del ? 3u + (uint32_t)digits_of((uint32_t)q) : 0u, sh, round);
        if (del) put_entry(at_d + ex, 'D', q, 0);
        at_d += round;
    }
}

}  // namespace

hipError_t launch_aa_locate(pm_ctx* c, const AaArgs& a) {
    if (a.nodes == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_aa_locate, dim3(blocks_of(a.nodes, kWavesPerBlock)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_aa_codons(pm_ctx* c, const AaArgs& a, const AaTables& t) {
    if (t.n == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_aa_codons, dim3((unsigned)t.n), dim3(256), 0, c->stream, a, t);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_aa_line_len(pm_ctx* c, const AaArgs& a, const AaTables& root, const AaTables& t, const AaText& x) {
    if (t.n == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_aa_line_len, dim3((unsigned)t.n), dim3(256), 0, c->stream, a, root, t, x);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_aa_write(pm_ctx* c, const AaArgs& a, const AaTables& root, const AaTables& t, const AaText& x) {
    if (t.n == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_aa_write, dim3((unsigned)t.n), dim3(256), 0, c->stream, a, root, t, x);
    timer_end(c, 3);
    return hipGetLastError();
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_aa() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_aa_line_len));
}

}  // namespace pm
