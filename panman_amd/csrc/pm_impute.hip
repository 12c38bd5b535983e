// pm_impute.hip -- N imputation kernels (Tree::imputeNs, src/impute.cpp) over nucleotide records in
// list order and over the replayed rows of every node (the derived PanMAT of pm_every_node.h with
// every block held forward, so a node's row is the walk's curSequence after its list).
//   k_impute_count      imputeSubstitution (:205-225) per record: the records that take its place (an
//                       NSNPS of N: none; an NS holding an N: its non-N bases; else itself) and the
//                       bases dropped.  std::find erasing "the first equal record" gives the same list as
//                       erasing every such record in place -- equal records are all erased, each at its
//                       own turn -- so nothing is searched
//   k_impute_pack       the records at their scanned offsets: NucMut(other, i) (src/panman.hpp:233-248)
//                       for every base put back, at position + i (gap -1) or gap position + i
//   k_impute_originals  originalNucs (:161): per record the codes under its bases in the parent's row
//   k_impute_steps      the lists of the (node, candidate) pairs' path steps into the record arrays
//                       that k_subnet_count / k_subnet_expand read, inverted where the path climbs
//                       (invertMutations, src/panman.cpp:2374-2420)
//   k_impute_pair_sum   per pair the folded survivors that imputeAllSubstitutionsWithNs (:227-241)
//                       leaves: all but the substitutions with code N
//   k_impute_twice      equal neighbours among the sorted (node, cell) keys of the lists
// One lane per record (or survivor); integer only; only vector stores.
#include "pm_bits.h"
#include "pm_cell.h"
#include "pm_dev.h"

namespace pm {
namespace {

constexpr uint32_t kSnpS = 3, kSnpI = 4, kSnpD = 5, kCodeN = 15;

// getCodeFromNucleotide of 'A' + k: 0 where it is no nucleotide ('-' and 'x' are 0 as well)
__constant__ uint8_t kImputeCode[26] = {1, 14, 2, 13, 0, 0, 4, 11, 0, 0, 12, 0, 3, 15, 0, 0, 0, 5, 6, 8, 0, 7, 9, 0, 10, 0};

__device__ __forceinline__ uint32_t code_of(char ch) {
    const uint32_t k = (uint32_t)(uint8_t)ch - (uint32_t)'A';
    return k < 26u ? kImputeCode[k] : 0u;
}

__device__ __forceinline__ uint32_t code_at(uint32_t nucs, int i) { return (nucs >> (4 * (5 - i))) & 15u; }

// the N codes among the record's first length() codes; 0 for a record that is no substitution
__device__ __forceinline__ int sub_ns(uint32_t info, uint32_t nucs) {
    const uint32_t type = info & 7u;
    if (type != PM_MUT_NS && type != kSnpS) return 0;
    int ns = 0;
    for (int i = 0; i < (int)(info >> 4); ++i) ns += code_at(nucs, i) == kCodeN;
    return ns;
}

__global__ __launch_bounds__(256) void k_impute_count(ImputeRecs in, int64_t keep0, int64_t keep1, int64_t* off,
                                                      unsigned long long* imputed) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > in.n) return;
    if (r == in.n) {
        off[r] = 0;
        return;
    }
    const uint32_t info = in.info[r];
    const int len = (int)(info >> 4), ns = r >= keep0 && r < keep1 ? 0 : sub_ns(info, in.nucs[r]);
    if (ns == 0) {
        off[r] = 1;
        return;
    }
    const int back = (info & 7u) == PM_MUT_NS ? len - ns : 0;   // (an NSNPS puts nothing back)
    off[r] = back;
    atomicAdd(imputed, (unsigned long long)(len - back));
}

__global__ __launch_bounds__(256) void k_impute_pack(ImputeRecs in, int64_t keep0, int64_t keep1, const int64_t* off, ImputeRecsOut out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= in.n) return;
    int64_t at = off[r];
    const int n = (int)(off[r + 1] - at);
    if (n == 0) return;
    const uint32_t info = in.info[r], nucs = in.nucs[r];
    const int32_t node = in.node ? in.node[r] : 0, primary = in.primary[r], pos = in.pos[r], gap = in.gap[r];
    const int len = (int)(info >> 4);
    const bool whole = (r >= keep0 && r < keep1) || sub_ns(info, nucs) == 0;
    if (whole) {
        if (out.node) out.node[at] = node;
        out.primary[at] = primary;
        out.pos[at] = pos;
        out.gap[at] = gap;
        out.info[at] = (uint8_t)info;
        out.nucs[at] = nucs;
        return;
    }
    for (int i = 0; i < len; ++i) {
        const uint32_t code = code_at(nucs, i);
        if (code == kCodeN) continue;
        if (out.node) out.node[at] = node;
        out.primary[at] = primary;
        out.pos[at] = gap == -1 ? pos + i : pos;
        out.gap[at] = gap == -1 ? -1 : gap + i;
        out.info[at] = (uint8_t)((1u << 4) | kSnpS);
        out.nucs[at] = code << 20;
        ++at;
    }
}

__global__ __launch_bounds__(256) void k_impute_originals(ImputeRecs in, ImputeRows w, uint32_t* orig) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= in.n) return;
    const int32_t prow = w.par_row[in.node[r]];
    uint32_t o = 0;
    if (prow >= 0) {
        const int32_t blk = in.primary[r], pos = in.pos[r], gap = in.gap[r];
        const int len = (int)(in.info[r] >> 4);
        for (int i = 0; i < len; ++i) {
            const int64_t col = cell_column(w.pos_off, w.main_col, w.gap_col, w.blocks, blk, pos, gap, i);
            if (col < 0 || col >= w.columns) {
                atomicOr(w.error, 1);
                continue;
            }
            o |= code_of(w.rows[(int64_t)prow * w.row_stride + col]) << (4 * (5 - i));
        }
    }
    orig[r] = o;
}

__global__ __launch_bounds__(256) void k_impute_steps(ImputeSteps s, ImputeRecs src, const uint32_t* orig,
                                                      ImputeRecsOut dst) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= s.records) return;
    const int64_t k = mutation_of_element(s.dst_off, s.steps, r);
    const int64_t from = s.src0[k] + (r - s.dst_off[k]);
    uint32_t info = src.info[from], nucs = src.nucs[from];
    if (s.inverted[k]) {
        const uint32_t type = info & 7u, len = info & 0xf0u;
        // an insertion becomes a deletion of code 0, a deletion an insertion of the originals, a
        // substitution goes back to the originals
        if (type == PM_MUT_NI || type == kSnpI) {
            info = len | (type == PM_MUT_NI ? (uint32_t)PM_MUT_ND : kSnpD);
            nucs = 0;
        } else {
            if (type == PM_MUT_ND || type == kSnpD) info = len | (type == PM_MUT_ND ? (uint32_t)PM_MUT_NI : kSnpI);
            nucs = orig[from];
        }
    }
    dst.node[r] = s.pair[k];
    dst.primary[r] = src.primary[from];
    dst.pos[r] = src.pos[from];
    dst.gap[r] = src.gap[from];
    dst.info[r] = (uint8_t)info;
    dst.nucs[r] = nucs;
}

__global__ __launch_bounds__(256) void k_impute_pair_sum(SubnetLive live, unsigned long long* sum) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= live.m) return;
    const uint32_t tc = live.tc[i];
    if ((tc >> 4) == kSnpS && (tc & 15u) == kCodeN) return;
    atomicAdd(sum + live.node[i], 1ull);
}

__global__ __launch_bounds__(256) void k_impute_twice(const uint64_t* key, int64_t n, int32_t* error) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (i < n && key[i] == key[i - 1]) atomicOr(error, 1);
}

template <class K, class... A>
hipError_t launch(pm_ctx* c, K kernel, int64_t n, A... args) {
    if (n <= 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(kernel, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, args...);
    timer_end(c, 3);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_impute_count(pm_ctx* c, const ImputeRecs& in, int64_t keep0, int64_t keep1, int64_t* off,
                               unsigned long long* imputed) {
    return launch(c, k_impute_count, in.n + 1, in, keep0, keep1, off, imputed);
}

hipError_t launch_impute_pack(pm_ctx* c, const ImputeRecs& in, int64_t keep0, int64_t keep1, const int64_t* off, const ImputeRecsOut& out) {
    return launch(c, k_impute_pack, in.n, in, keep0, keep1, off, out);
}

hipError_t launch_impute_originals(pm_ctx* c, const ImputeRecs& in, const ImputeRows& rows, uint32_t* orig) {
    return launch(c, k_impute_originals, in.n, in, rows, orig);
}

hipError_t launch_impute_steps(pm_ctx* c, const ImputeSteps& s, const ImputeRecs& src, const uint32_t* orig, const ImputeRecsOut& dst) {
    return launch(c, k_impute_steps, s.records, s, src, orig, dst);
}

hipError_t launch_impute_pair_sum(pm_ctx* c, const SubnetLive& live, unsigned long long* sum) {
    return launch(c, k_impute_pair_sum, live.m, live, sum);
}

hipError_t launch_impute_twice(pm_ctx* c, const uint64_t* key, int64_t n, int32_t* error) {
    return launch(c, k_impute_twice, n - 1, key, n, error);
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_impute() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_impute_count));
}

}  // namespace pm
