// pm_subnet.hip -- subnetwork extraction kernels (Tree::consolidateNucMutations, src/panman.cpp:
// 2233-2322, with replaceMutation, :2058-2085) over the mutation records of every merged chain at once.
//
// The reference re-consolidates a merged node's list through a hash map at every merge down a chain,
// which is quadratic along the chain.  One left fold per coordinate over the chain's lists, top first,
// gives the same survivors, so here:
//   k_subnet_count    bases per record (types 3-5: one, whatever the length nibble says); checks the
//                     record's coordinates against its block and gap slots
//   k_subnet_expand   per base the key (new node << 32 | rank of the coordinate in tuple order) and the
//                     value (entry number << 8 | SNP type << 4 | code), plus the coordinate by entry number
//   subnet_sort       hipCUB's LSD radix sort of the pairs by key.  LSD radix sort is stable: entries of
//                     one coordinate stay in entry order, which is list order down the chain.  The fold
//                     relies on that (and checks it: the entry numbers of a segment must ascend)
//   k_subnet_fold     one lane per entry; the lane at the head of a key segment walks the segment with
//                     the replaceMutation table.  Sequential on purpose: the table is not known to be
//                     associative, and a segment is as short as the chain is deep
//   k_subnet_compact  the surviving heads, numbered by the scan of their flags, stay in sorted order
//   k_subnet_runs     heads of the maximal runs (same node, block and type; consecutive positions at gap
//                     -1, or consecutive gap slots of one position); an inclusive max-scan of
//                     (head ? index : 0) gives every survivor its run's head -- one scan whatever the
//                     run lengths, where a backward walk would need the head's own offset first
//   k_subnet_starts   a record starts wherever (index - run head) % 6 == 0: the reference's greedy cut
//   k_subnet_pack     one lane per record start: up to 6 codes, info = length << 4 | type
// Only vector stores.
#include <hipcub/hipcub.hpp>

#include "pm_dev.h"

namespace pm {
namespace {

constexpr uint32_t kSnpS = 3, kSnpI = 4, kSnpD = 5;   // NucMutationType::NSNPS / NSNPI / NSNPD

__device__ __forceinline__ int bases_of(uint32_t info) { return (info & 7u) >= 3 ? 1 : (int)(info >> 4); }

// 0, or why the record's bases do not all lie inside the block (the host has checked type and length)
__device__ __forceinline__ int32_t check_record(const SubnetArgs& a, int64_t r) {
    const int32_t id = a.rec_primary[r];
    if (id < 0 || id >= a.blocks || a.blk_len[id] < 0) return kSubnetBadBlock;
    const int32_t len = a.blk_len[id], pos = a.rec_pos[r], gap = a.rec_gap[r];
    const int n = bases_of(a.rec_info[r]);
    if (pos < 0 || pos > len) return kSubnetBadPos;
    if (gap == -1) return (int64_t)pos + n - 1 > len ? kSubnetBadPos : 0;
    const uint32_t* pb = a.pos_base + a.pos_off[id] + pos;
    const int64_t slots = (int64_t)(pb[1] - pb[0]) - 1;
    return gap < 0 || (int64_t)gap + n > slots ? kSubnetBadGap : 0;
}

__global__ __launch_bounds__(256) void k_subnet_count(SubnetArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > a.records) return;
    if (r == a.records) {
        a.rec_off[r] = 0;
        return;
    }
    const int32_t bad = check_record(a, r);
    if (bad) atomicMax(a.error, bad);
    a.rec_off[r] = bad ? 0 : bases_of(a.rec_info[r]);
}

__global__ __launch_bounds__(256) void k_subnet_expand(SubnetArgs a, SubnetEntries e) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.records) return;
    const int64_t at = a.rec_off[r];
    const int n = (int)(a.rec_off[r + 1] - at);   // (0 for a record k_subnet_count refused)
    if (n == 0) return;
    const int32_t id = a.rec_primary[r], pos = a.rec_pos[r], gap = a.rec_gap[r];
    const uint32_t info = a.rec_info[r], nucs = a.rec_nucs[r];
    uint32_t type = info & 7u;
    type = type == PM_MUT_NS ? kSnpS : type == PM_MUT_NI ? kSnpI : type == PM_MUT_ND ? kSnpD : type;
    const uint64_t node = (uint64_t)(uint32_t)a.rec_node[r] << 32;
    const uint32_t* pb = a.pos_base + a.pos_off[id];
    const uint32_t base = a.block_base[id];
    for (int j = 0; j < n; ++j) {
        const int32_t p = gap == -1 ? pos + j : pos, g = gap == -1 ? -1 : gap + j;
        const uint32_t rank = base + pb[p] + (uint32_t)(g + 1);
        const uint32_t code = (nucs >> (4 * (5 - j))) & 15u;
        e.key[at + j] = node | rank;
        e.val[at + j] = ((uint64_t)(at + j) << 8) | (type << 4) | code;
        e.blk[at + j] = id;
        e.pos[at + j] = p;
        e.gap[at + j] = g;
    }
}

// replaceMutation (src/panman.cpp:2058-2085) folded over one coordinate's entries in list order; a
// deletion after an insertion removes the coordinate, and the next entry starts afresh.
__global__ __launch_bounds__(256) void k_subnet_fold(const uint64_t* key, const uint64_t* val, int64_t n, int64_t* alive,
                                                     uint8_t* tc, int32_t* error) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        alive[i] = 0;
        return;
    }
    const uint64_t k = key[i];
    if (i > 0 && key[i - 1] == k) {
        alive[i] = 0;
        return;
    }
    bool have = false, unstable = false;
    uint32_t type = 0, code = 0;
    uint64_t last = 0;
    for (int64_t j = i; j < n && key[j] == k; ++j) {
        const uint64_t v = val[j];
        const uint32_t t = (uint32_t)(v >> 4) & 7u, cd = (uint32_t)v & 15u;
        unstable |= j > i && (v >> 8) <= last;
        last = v >> 8;
        if (!have || t == type) {
            have = true;
            type = t;
        } else if (type == kSnpS) {
            type = t == kSnpD ? kSnpD : kSnpS;
        } else if (type == kSnpI) {
            if (t == kSnpD) have = false;
        } else {   // a deletion: an insertion makes it a substitution, a substitution an insertion
            type = t == kSnpI ? kSnpS : kSnpI;
        }
        code = cd;
    }
    if (unstable) atomicMax(error, kSubnetUnstable);
    alive[i] = have ? 1 : 0;
    tc[i] = (uint8_t)((type << 4) | code);
}

__global__ __launch_bounds__(256) void k_subnet_compact(const uint64_t* key, const uint64_t* val, int64_t n, const int64_t* ascan,
                                                        const uint8_t* tc, SubnetEntries e, SubnetLive s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || ascan[i + 1] == ascan[i]) return;
    const int64_t at = ascan[i], entry = (int64_t)(val[i] >> 8);
    s.node[at] = (int32_t)(key[i] >> 32);
    s.blk[at] = e.blk[entry];
    s.pos[at] = e.pos[entry];
    s.gap[at] = e.gap[entry];
    s.tc[at] = tc[i];
}

__global__ __launch_bounds__(256) void k_subnet_runs(SubnetLive s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.m) return;
    bool joins = false;
    if (i > 0 && s.node[i] == s.node[i - 1] && s.blk[i] == s.blk[i - 1] && (s.tc[i] >> 4) == (s.tc[i - 1] >> 4)) {
        const int32_t g0 = s.gap[i - 1], g1 = s.gap[i], p0 = s.pos[i - 1], p1 = s.pos[i];
        joins = g0 == -1 ? (g1 == -1 && p1 == p0 + 1) : (p1 == p0 && g1 == g0 + 1);
    }
    s.head[i] = joins ? 0 : i;
}

__global__ __launch_bounds__(256) void k_subnet_starts(SubnetLive s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > s.m) return;
    s.start[i] = i < s.m && (i - s.head[i]) % 6 == 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_subnet_pack(SubnetLive s, SubnetOut o) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.m || s.start[i + 1] == s.start[i]) return;   // (start holds its exclusive scan by now)
    const int64_t at = s.start[i], head = s.head[i];
    const uint32_t type = s.tc[i] >> 4;
    uint32_t nucs = (uint32_t)(s.tc[i] & 15u) << 20;
    int len = 1;
    while (len < 6 && i + len < s.m && s.head[i + len] == head) {
        nucs |= (uint32_t)(s.tc[i + len] & 15u) << (4 * (5 - len));
        ++len;
    }
    // NucMut(tuple) keeps the SNP type; NucMut(array, i, j) maps it back to NS / NI / ND (src/panman.hpp:98-189)
    const uint32_t run_type = type == kSnpS ? PM_MUT_NS : type == kSnpI ? PM_MUT_NI : PM_MUT_ND;
    o.primary[at] = s.blk[i];
    o.pos[at] = s.pos[i];
    o.gap[at] = s.gap[i];
    o.info[at] = (uint8_t)((len << 4) | (len == 1 ? type : run_type));
    o.nucs[at] = nucs;
    atomicAdd(o.node_count + s.node[i], 1);
}

struct MaxOp {
    __host__ __device__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};

template <class K, class... A>
hipError_t launch(pm_ctx* c, K kernel, int64_t n, A... args) {
    if (n == 0) return hipSuccess;
    timer_begin(c, 3);
    hipLaunchKernelGGL(kernel, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, args...);
    timer_end(c, 3);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_subnet_count(pm_ctx* c, const SubnetArgs& a) { return launch(c, k_subnet_count, a.records + 1, a); }

hipError_t launch_subnet_expand(pm_ctx* c, const SubnetArgs& a, const SubnetEntries& e) {
    return launch(c, k_subnet_expand, a.records, a, e);
}

hipError_t subnet_sort(pm_ctx* c, const SubnetEntries& e, uint64_t* key_alt, uint64_t* val_alt, int end_bit, uint64_t** key_out,
                       uint64_t** val_out) {
    hipcub::DoubleBuffer<uint64_t> keys(e.key, key_alt), vals(e.val, val_alt);
    Dev<char> tmp;
    size_t bytes = 0;
    hipError_t err = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys, vals, (int)e.n, 0, end_bit, c->stream);
    if (err == hipSuccess) err = tmp.alloc(bytes, false, c->stream);
    if (err == hipSuccess) {
        timer_begin(c, 3);
        err = hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, keys, vals, (int)e.n, 0, end_bit, c->stream);
        timer_end(c, 3);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);   // (tmp is released on return)
    *key_out = keys.Current();
    *val_out = vals.Current();
    return err;
}

hipError_t launch_subnet_fold(pm_ctx* c, const uint64_t* key, const uint64_t* val, int64_t n, int64_t* alive, uint8_t* tc,
                              int32_t* error) {
    return launch(c, k_subnet_fold, n + 1, key, val, n, alive, tc, error);
}

hipError_t launch_subnet_compact(pm_ctx* c, const uint64_t* key, const uint64_t* val, int64_t n, const int64_t* ascan,
                                 const uint8_t* tc, const SubnetEntries& e, const SubnetLive& s) {
    return launch(c, k_subnet_compact, n, key, val, n, ascan, tc, e, s);
}

hipError_t subnet_runs(pm_ctx* c, const SubnetLive& s) {
    if (s.m == 0) return hipSuccess;
    hipError_t err = launch(c, k_subnet_runs, s.m, s);
    Dev<char> tmp;
    size_t bytes = 0;
    if (err == hipSuccess) err = hipcub::DeviceScan::InclusiveScan(nullptr, bytes, s.head, s.head, MaxOp(), (int)s.m, c->stream);
    if (err == hipSuccess) err = tmp.alloc(bytes, false, c->stream);
    if (err == hipSuccess) {
        timer_begin(c, 3);
        err = hipcub::DeviceScan::InclusiveScan(tmp.p, bytes, s.head, s.head, MaxOp(), (int)s.m, c->stream);
        timer_end(c, 3);
    }
    if (err == hipSuccess) err = launch(c, k_subnet_starts, s.m + 1, s);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);   // (tmp is released on return)
    return err;
}

hipError_t launch_subnet_pack(pm_ctx* c, const SubnetLive& s, const SubnetOut& o) {
    return launch(c, k_subnet_pack, s.m, s, o);
}

// This file's code object, loaded ahead of its first launch (pm_warmup).
hipError_t warm_subnet() {
    hipFuncAttributes at;
    return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_subnet_starts));
}

}  // namespace pm
