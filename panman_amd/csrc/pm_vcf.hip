// pm_vcf.hip -- VCF extraction kernels (Tree::printVCFParallel, src/vcf.cpp:177-382) over the
// aligned FASTA text that format_device leaves in the context's text buffer.
//
// Column i of a leaf's aligned row is text[row_base[leaf] + i + i / 70] (70-column wrap).  The
// reference compares every tip's row with the reference tip's column by column; here:
//   k_vcf_ref       the reference row without line breaks + POS of every column (one exclusive scan)
//   k_vcf_classify  per (leaf, 64 columns) two ballots: `skip` (both rows '-') and `equal`
//                   (the same base) bit-planes -- the stream over leaves x columns
//   k_vcf_starts    per leaf (one wave) the events: maximal runs of compared, unequal columns
//                   between equal columns; counted, then listed
//   k_vcf_chain     per leaf the first equal column that anchors: before it an event starts
//                   with empty strings (a leading insertion chain), after it with the equal
//                   base before it
//   k_vcf_emit      one lane per event walks it with the reference's rules: count, scan, write
//   k_vcf_text_*    the genotype text of a batch of lines (widths, offsets, characters)
// Only vector stores and ordinary atomics.
#include <hipcub/hipcub.hpp>

#include "pm_bits.h"
#include "pm_dev.h"

namespace pm {
namespace {

constexpr int kVcfWaveWords = 16;   // 64-column words per classify wave (1024 columns)
constexpr int kRefItems = 8;        // columns per thread and round of k_vcf_ref

__device__ __forceinline__ char tip_at(const char* text, int64_t base, uint32_t i) { return text[base + i + i / 70]; }

__global__ __launch_bounds__(256) void k_vcf_ref(VcfArgs a) {
    using Scan = hipcub::BlockScan<int, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t base = a.row_base[a.ref_leaf];
    const uint32_t n = (uint32_t)a.n;
    int carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 256 * kRefItems) {
        char ch[kRefItems];
        int f[kRefItems], total;
        for (int k = 0; k < kRefItems; ++k) {
            const uint32_t i = c0 + threadIdx.x * kRefItems + k;
            ch[k] = i < n ? tip_at(a.text, base, i) : '-';
            f[k] = ch[k] != '-';
        }
        Scan(tmp).ExclusiveSum(f, f, total);
        __syncthreads();
        for (int k = 0; k < kRefItems; ++k) {
            const uint32_t i = c0 + threadIdx.x * kRefItems + k;
            if (i < n) {
                a.ref[i] = ch[k];
                a.coord[i] = carry + f[k] + 1;
            }
        }
        carry += total;
    }
}

// One wave per (leaf, 1024 columns): a byte of the tip's row and of the reference row per
// lane, so each ballot is one 64-column plane word (the wrap's line breaks keep the columns
// off any 16-byte grid of the text).
__global__ __launch_bounds__(256) void k_vcf_classify(VcfArgs a, uint32_t chunks) {
    const uint32_t leaf = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (!a.live[leaf]) return;
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)chunk * kWavesPerBlock + (threadIdx.x >> 6)) * kVcfWaveWords;
    if (w0 >= a.words) return;
    const int64_t base = a.row_base[leaf];
    const uint32_t n = (uint32_t)a.n;
    uint64_t sk = 0, eq = 0;
    for (int k = 0; k < kVcfWaveWords; ++k) {
        if (w0 + k >= a.words) break;   // (wave-uniform)
        const uint32_t i = (uint32_t)((w0 + k) * 64 + lane);
        char r = '-', t = '-';
        if (i < n) {
            r = a.ref[i];
            t = tip_at(a.text, base, i);
        }
        const uint64_t s = __ballot(r == '-' && t == '-');
        const uint64_t e = __ballot(r != '-' && r == t);
        if (lane == k) {
            sk = s;
            eq = e;
        }
    }
    if (lane < kVcfWaveWords && w0 + lane < a.words) {
        a.skip[(int64_t)leaf * a.words + w0 + lane] = sk;
        a.equal[(int64_t)leaf * a.words + w0 + lane] = eq;
    }
}

__device__ __forceinline__ int top_bit(uint64_t v) { return 63 - __clzll((long long)v); }

// One wave per leaf, 64 plane words per round.  An event starts at a compared, unequal column
// whose previous compared column holds an equal base (or is the row's start).  Within a word
// that is a carry chain: adding (equal << 1 | carry-in) to the skip bits lets every equal base
// ripple through the skipped columns above it onto the next compared column.  The carry into a
// word is the last compared column of the nearest non-empty word below it.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_vcf_starts(VcfArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (leaf >= a.leaves) return;
    if (!a.live[leaf]) {
        if (!WRITE && lane == 0) a.nstart[leaf] = 0;
        return;
    }
    const uint64_t* skp = a.skip + leaf * a.words;
    const uint64_t* eqp = a.equal + leaf * a.words;
    uint64_t carry = 1;
    int64_t count = 0;                          // counting: this lane's events
    int64_t out = WRITE ? a.nstart[leaf] : 0;   // listing: the round's first slot
    for (int64_t w0 = 0; w0 < a.words; w0 += 64) {
        const int64_t w = w0 + lane;
        uint64_t s = ~0ull, e = 0;
        if (w < a.words) {
            s = skp[w];
            e = eqp[w];
        }
        const uint64_t ns = ~s;
        const bool has = ns != 0;
        const bool last_eq = has && ((e >> top_bit(ns)) & 1);
        const uint64_t has_m = __ballot(has), last_m = __ballot(last_eq);
        const uint64_t lower = has_m & ((1ull << lane) - 1);
        const uint64_t cin = lower ? (last_m >> top_bit(lower)) & 1 : carry;
        if (has_m) carry = (last_m >> top_bit(has_m)) & 1;
        uint64_t st = (((e << 1) | cin) + s) & ns & ~e;
        const int pc = __popcll(st);
        if (!WRITE) {
            count += pc;
        } else {
            int incl = pc;
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            int64_t at = out + incl - pc;
            out += __shfl(incl, 63, 64);
            while (st) {
                const int b = __ffsll((long long)st) - 1;
                st &= st - 1;
                a.ev_leaf[at] = (int32_t)leaf;
                a.ev_col[at] = (int32_t)(w * 64 + b);
                ++at;
            }
        }
    }
    if (!WRITE) {
        for (int d = 32; d > 0; d >>= 1) count += __shfl_down(count, d, 64);
        if (lane == 0) a.nstart[leaf] = count;
    }
}

// One lane per leaf: the reference's strings start empty and stay unanchored while every equal
// column follows a run of insertions only (each such run is emitted with the equal base behind
// it and the strings are cleared).  The first equal column that follows nothing, or a run
// holding a reference base, anchors; from there on every event starts with the equal base
// before it.
__global__ __launch_bounds__(256) void k_vcf_chain(VcfArgs a) {
    const int64_t leaf = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (leaf >= a.leaves || !a.live[leaf]) return;
    const uint64_t* skp = a.skip + leaf * a.words;
    const uint64_t* eqp = a.equal + leaf * a.words;
    bool seen = false, pure = true;
    int64_t found = a.n;
    for (int64_t w = 0; w < a.words && found == a.n; ++w) {
        uint64_t ns = ~skp[w];
        const uint64_t e = eqp[w];
        while (ns) {
            const int b = __ffsll((long long)ns) - 1;
            ns &= ns - 1;
            const int64_t i = w * 64 + b;
            if ((e >> b) & 1) {
                if (!seen || !pure) {
                    found = i;
                    break;
                }
                seen = false;
            } else {
                seen = true;
                if (a.ref[i] != '-') pure = false;   // a deletion or substitution column
            }
        }
    }
    a.chain[leaf] = found;
}

// One lane per event.  R and A are never stored while walking: R is the anchor (if any) plus
// the reference bases of the deletion / substitution columns of [from, j), A the anchor plus
// the tip's bases of the insertion / substitution columns; lr / la count them.  `differ`
// remembers a mismatch found at a position both strings have (they only grow until cleared),
// so the string comparisons of one event walk its columns a bounded number of times.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_vcf_emit(VcfArgs a) {
    const int64_t ev = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ev >= a.events) return;
    if (WRITE && a.ev_recs[ev + 1] == a.ev_recs[ev]) return;
    const int32_t leaf = a.ev_leaf[ev];
    const uint32_t col = (uint32_t)a.ev_col[ev], n = (uint32_t)a.n;
    const int64_t base = a.row_base[leaf];
    const char* text = a.text;
    const char* ref = a.ref;
    bool anchor = false;
    char ac = 0;
    int32_t ds = 1;
    if ((int64_t)col > a.chain[leaf]) {   // the compared column before it (chain[leaf] at the latest)
        const uint64_t* skp = a.skip + (int64_t)leaf * a.words;
        int64_t w = (col - 1) >> 6;
        uint64_t ns = ~skp[w] & (~0ull >> (63 - ((col - 1) & 63)));
        while (!ns) ns = ~skp[--w];
        const int64_t j = w * 64 + top_bit(ns);
        anchor = true;
        ac = ref[j];
        ds = a.coord[j];
    }
    uint32_t from = col, lr = 0, la = 0;
    bool differ = false;
    auto same = [&]() -> bool {   // R == A
        if (lr != la || differ) return false;
        uint32_t i = from, k = from;
        for (uint32_t m = 0; m < lr; ++m, ++i, ++k) {
            char r, t;
            for (;; ++i) {
                r = ref[i];
                if (r != '-' && tip_at(text, base, i) != r) break;
            }
            for (;; ++k) {
                t = tip_at(text, base, k);
                if (t != '-' && ref[k] != t) break;
            }
            if (r != t) {
                differ = true;
                return false;
            }
        }
        return true;
    };
    uint32_t j = col;
    bool closed = false;
    char cc = 0;
    for (; j < n; ++j) {
        const char r = ref[j], t = tip_at(text, base, j);
        if (r == '-' && t == '-') continue;
        if (r == t) {
            closed = true;
            cc = r;
            break;
        }
        const bool empty = !anchor && lr == 0 && la == 0;
        if (t == '-' || r == '-') {
            if (empty) {
                ds = a.coord[j];
                from = j;
            }
            if (t == '-') ++lr;
            else ++la;
        } else {
            if (same()) {
                anchor = false;
                lr = la = 0;
                differ = false;
                from = j;
                ds = a.coord[j];
            }
            ++lr;
            ++la;
            if (lr == la) differ = true;   // the two bases appended at the same position
        }
    }
    bool emit = false, ins = false;
    int32_t pos = ds;
    if (!same()) {
        emit = true;
        if (closed && !anchor && lr == 0) {   // an insertion with nothing before it: the equal base closes it
            ins = true;
            pos = a.coord[j];
        }
    }
    const uint32_t rlen = ins ? 1 : (anchor ? 1 : 0) + lr, alen = ins ? la + 1 : (anchor ? 1 : 0) + la;
    if (!WRITE) {
        a.ev_recs[ev] = emit ? 1 : 0;
        a.ev_bytes[ev] = emit ? (int64_t)rlen + alen : 0;
        return;
    }
    if (!emit) return;
    const int64_t off = a.ev_bytes[ev];
    a.recs[a.ev_recs[ev]] = VcfRec{leaf, pos, off, (int32_t)rlen, (int32_t)alen};
    char* p = a.pool + off;
    if (ins) {
        *p++ = cc;
    } else {
        if (anchor) *p++ = ac;
        for (uint32_t i = from; i < j; ++i) {
            const char r = ref[i];
            if (r != '-' && tip_at(text, base, i) != r) *p++ = r;
        }
        if (anchor) *p++ = ac;
    }
    for (uint32_t i = from; i < j; ++i) {
        const char t = tip_at(text, base, i);
        if (t != '-' && ref[i] != t) *p++ = t;
    }
    if (ins) *p++ = cc;
}

// ---- genotype text ------------------------------------------------------------------------

// (a tip with two ALTs of one line keeps the later one, as the reference's map assignment does)
__global__ __launch_bounds__(256) void k_vcf_gt_fill(VcfTextArgs t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= t.cells) return;
    const int32_t* c = t.cell + 3 * i;
    atomicMax(&t.gt[(int64_t)c[0] * t.samples + c[1]], (uint32_t)c[2]);
}

// One workgroup per line: prefix + ('\t' + digits) per sample + '\n'.
__global__ __launch_bounds__(256) void k_vcf_text_count(VcfTextArgs t) {
    using Reduce = hipcub::BlockReduce<int64_t, 256>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t line = blockIdx.x;
    const uint32_t* g = t.gt + line * t.samples;
    int64_t w = 0;
    for (int32_t s = threadIdx.x; s < t.samples; s += 256) w += 1 + digits_of(g[s]);
    const int64_t sum = Reduce(tmp).Sum(w);
    if (threadIdx.x == 0) t.line_off[line] = t.prefix_off[line + 1] - t.prefix_off[line] + sum + 1;
}

__global__ __launch_bounds__(256) void k_vcf_text_write(VcfTextArgs t) {
    using Scan = hipcub::BlockScan<int, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t line = blockIdx.x;
    const uint32_t* g = t.gt + line * t.samples;
    char* out = t.text + t.line_off[line];
    const int64_t plen = t.prefix_off[line + 1] - t.prefix_off[line];
    const char* pre = t.prefix + t.prefix_off[line];
    for (int64_t k = threadIdx.x; k < plen; k += 256) out[k] = pre[k];
    out += plen;
    int64_t carry = 0;
    for (int32_t s0 = 0; s0 < t.samples; s0 += 256) {
        const int32_t s = s0 + threadIdx.x;
        uint32_t v = s < t.samples ? g[s] : 0;
        const int w = s < t.samples ? 1 + digits_of(v) : 0;
        int ex, total;
        Scan(tmp).ExclusiveSum(w, ex, total);
        __syncthreads();
        if (s < t.samples) {
            char* q = out + carry + ex;
            q[0] = '\t';
            for (int k = w - 1; k >= 1; --k) {
                q[k] = (char)('0' + v % 10);
                v /= 10;
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) out[carry] = '\n';
}

}  // namespace

hipError_t launch_vcf_classify(pm_ctx* c, const VcfArgs& a) {
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_vcf_ref, dim3(1), dim3(256), 0, c->stream, a);
    const int64_t chunks = (a.words + kWavesPerBlock * kVcfWaveWords - 1) / (kWavesPerBlock * kVcfWaveWords);
    hipLaunchKernelGGL(k_vcf_classify, dim3((unsigned)(chunks * a.leaves)), dim3(256), 0, c->stream, a, (uint32_t)chunks);
    hipLaunchKernelGGL(k_vcf_starts<false>, dim3(blocks_of(a.leaves, kWavesPerBlock)), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_vcf_chain, dim3(blocks_of(a.leaves, 256)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_vcf_list(pm_ctx* c, const VcfArgs& a) {
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_vcf_starts<true>, dim3(blocks_of(a.leaves, kWavesPerBlock)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_vcf_emit(pm_ctx* c, const VcfArgs& a, bool write) {
    if (a.events == 0) return hipSuccess;
    timer_begin(c, 3);
    if (write) hipLaunchKernelGGL(k_vcf_emit<true>, dim3(blocks_of(a.events, 256)), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(k_vcf_emit<false>, dim3(blocks_of(a.events, 256)), dim3(256), 0, c->stream, a);
    timer_end(c, 3);
    return hipGetLastError();
}

hipError_t launch_vcf_text_count(pm_ctx* c, const VcfTextArgs& t) {
    if (t.lines == 0) return hipSuccess;
    timer_begin(c, 3);
    hipError_t e = hipMemsetAsync(t.gt, 0, sizeof(uint32_t) * (size_t)t.lines * t.samples, c->stream);
    if (e == hipSuccess && t.cells)
        hipLaunchKernelGGL(k_vcf_gt_fill, dim3(blocks_of(t.cells, 256)), dim3(256), 0, c->stream, t);
    if (e == hipSuccess) hipLaunchKernelGGL(k_vcf_text_count, dim3((unsigned)t.lines), dim3(256), 0, c->stream, t);
    timer_end(c, 3);
    return e == hipSuccess ? hipGetLastError() : e;
}

hipError_t launch_vcf_text_write(pm_ctx* c, const VcfTextArgs& t) {
    if (t.lines == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(k_vcf_text_write, dim3((unsigned)t.lines), dim3(256), 0, c->stream, t);
    timer_end(c, 3);
    return hipGetLastError();
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_vcf() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_vcf_classify));
}

}  // namespace pm
