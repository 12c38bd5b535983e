// pm_host.cpp -- host side of the C-ABI: context, uploads, results.
//
// The reference keeps the tree as Node* with children vectors and rebuilds an
// unordered_map<string,int> per column (src/panman.cpp:1409-1417).  Here the topology is
// flattened once (pm_tree_upload: the host plan of pm_plan.cpp, then its arrays to the
// device): dense internal indices, height levels for the post-order and depth levels for
// the pre-order, children encoded for the kernels.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "pm_internal.h"

namespace pm {

int fail(pm_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

int hip_fail(pm_ctx* c, hipError_t e, const char* what) {
    return fail(c, PM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

namespace {

template <class T>
hipError_t dev_alloc(T** p, size_t count) {
    if (count == 0) count = 1;
    return hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * count);
}

template <class T>
void dev_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

template <class T>
hipError_t upload(T** dst, const std::vector<T>& v, hipStream_t s) {
    hipError_t e = dev_alloc(dst, v.size());
    if (e != hipSuccess || v.empty()) return e;
    e = hipMemcpyAsync(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);   // host vectors may die after return
}

// Every device array of the tree, in upload order: X(DevTree pointer, its host vector in a
// TreePlan p).  The one list behind free_tree and upload_tree.
#define PM_TREE_ARRAYS(X)                 \
    X(child_off, p.ht.child_off)          \
    X(child_enc, p.ht.child_enc)          \
    X(parent_dense, p.parent_dense)       \
    X(internal_id, p.ht.internal_id)      \
    X(leaf_id, p.ht.leaf_id)              \
    X(up_order, p.up_order)               \
    X(down_order, p.down_order)           \
    X(leaf_parent, p.leaf_parent)         \
    X(leaf_down, p.leaf_down)             \
    X(child_enc_v, p.child_enc_v)         \
    X(up_order_v, p.up_order_v)           \
    X(down_order_v, p.down_order_v)       \
    X(down_desc, p.down_desc)             \
    X(up_desc, p.up_desc)                 \
    X(up_desc_v, p.up_desc_v)             \
    X(down_desc_v, p.down_desc_v)         \
    X(vleaf, p.vleaf)                     \
    X(tail_desc, p.tail_desc)             \
    X(tail_desc_v, p.tail_desc_v)         \
    X(part_desc, p.part_desc)             \
    X(part_desc_v, p.part_desc_v)         \
    X(part_desc_k, p.part_desc_k)         \
    X(part_desc_gs, p.part_desc_gs)       \
    X(child_enc_k, p.child_enc_k)         \
    X(up_desc_k, p.up_desc_k)             \
    X(up_desc_g, p.up_desc_g)             \
    X(up_desc_gs, p.up_desc_gs)           \
    X(down_desc_k, p.down_desc_k)         \
    X(down_desc_ks, p.down_desc_ks)       \
    X(pslot_k, p.pslot_k)                 \
    X(pslot_g, p.pslot_g)                 \
    X(pslot_gs, p.pslot_gs)               \
    X(vinner, p.vinner)                   \
    X(tail_desc_k, p.tail_desc_k)         \
    X(lvl, p.lvl)                         \
    X(cl_items, p.ht.cl.items)            \
    X(cl_down_items, p.ht.cl.down_items)  \
    X(cl_wg_off, p.ht.cl.wg_off)          \
    X(cl_slot_of, p.ht.cl.slot_of)        \
    X(pslot_kc, p.pslot_kc)               \
    X(pslot_gc, p.pslot_gc)               \
    X(cl_pslot, p.cl_pslot)

void free_tree(DevTree& t) {
#define X(field, host) dev_free(t.field);
    PM_TREE_ARRAYS(X)
#undef X
    t = DevTree{};
}

// The plan's arrays on the device and their bytes (pm_memory_footprint); on a failure nothing
// stays allocated.
hipError_t upload_tree(const TreePlan& p, hipStream_t s, DevTree& dt, size_t& bytes) {
    dt = DevTree{};
    dt.num_internal = (int32_t)p.ht.internal_id.size();
    dt.num_leaves = (int32_t)p.ht.leaf_id.size();
    dt.root_dense = p.ht.dense_of[p.ht.root];
    bytes = 0;
    hipError_t e = hipSuccess;
#define X(field, host)                                  \
    if (e == hipSuccess) {                              \
        bytes += sizeof((host)[0]) * (host).size();     \
        e = upload(&dt.field, host, s);                 \
    }
    PM_TREE_ARRAYS(X)
#undef X
    if (e != hipSuccess) free_tree(dt);
    return e;
}

void drop_graph(pm_ctx* c) {
    if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
    c->graph_exec = nullptr;
    c->graph_key = 0;
}

void free_columns(pm_ctx* c) {
    drop_graph(c);
    dev_free(c->leaf_planes);
    dev_free(c->leaf_present);
    dev_free(c->leaf_flag);
    dev_free(c->cons);
    dev_free(c->forced);
    dev_free(c->score);
    dev_free(c->root_code);
    dev_free(c->root_final);
    dev_free(c->sub_planes);
    c->sub_planes_bytes = 0;
    c->sub_planes_ok = false;
    c->has_leaves = c->has_sites = c->has_forced = false;
    c->ran = false;
}

void free_work(pm_ctx* c) {
    drop_graph(c);
    dev_free(c->sets);
    dev_free(c->cmask);
    dev_free(c->upm);
    c->upm_bytes = 0;
    dev_free(c->finals);
    dev_free(c->sk_parts);
    dev_free(c->recs);
    dev_free(c->shard_cnt);
    c->sets_bytes = c->finals_bytes = c->cmask_bytes = c->sk_parts_bytes = 0;
    c->shard_cap = 0;
}

int64_t wpad_of(const pm_ctx* c) { return (int64_t)((c->words + kWave - 1) / kWave) * kWave; }

// Allocate per-shard column buffers (leaf planes, consensus, outputs) for S sites.
int alloc_columns(pm_ctx* c, int64_t sites) {
    free_columns(c);
    c->num_sites = sites;
    c->words = (int32_t)((sites + 31) / 32);
    const int64_t wpad = wpad_of(c);
    hipError_t e;
    if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->leaf_planes), sizeof(uint4) * (size_t)c->dt.num_leaves * wpad)) != hipSuccess ||
        (e = dev_alloc(&c->leaf_flag, (size_t)c->dt.num_leaves)) != hipSuccess ||
        (e = dev_alloc(&c->cons, (size_t)std::max<int64_t>(wpad, 4 * kWave))) != hipSuccess ||   // cx_base reads 4 tiles
        (e = dev_alloc(&c->forced, (size_t)wpad)) != hipSuccess ||
        (e = dev_alloc(&c->score, (size_t)sites)) != hipSuccess ||
        (e = dev_alloc(&c->root_code, (size_t)sites)) != hipSuccess ||
        (e = dev_alloc(&c->root_final, (size_t)wpad)) != hipSuccess) {
        free_columns(c);
        return fail(c, PM_ERR_OOM, std::string("column buffers: ") + hipGetErrorString(e));
    }
    (void)hipMemsetAsync(c->cons, 0, sizeof(uint4) * std::max<int64_t>(wpad, 4 * kWave), c->stream);
    return PM_OK;
}

// Work buffers sized for the current shard and mode; records get a first-guess capacity
// that pm_mutation_count grows on overflow.
int alloc_work(pm_ctx* c, int mode) {
    const int64_t wpad = wpad_of(c);
    const bool fitch = mode == PM_MODE_FITCH || mode == PM_MODE_BLOCK_FITCH;
    const size_t planes = fitch ? 4 * kFitchRecQuads : 36;   // records of kFitchRec / kSankoffRec uint4 per tile
    const size_t need_sets = (size_t)c->dt.num_internal * wpad * planes * 4;
    const size_t need_mask = (size_t)c->dt.num_internal * (wpad / kWave) * kMaskWords * sizeof(uint64_t);
    hipError_t e;
    if (need_sets > c->sets_bytes) {
        dev_free(c->sets);
        if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->sets), need_sets)) != hipSuccess)
            return fail(c, PM_ERR_OOM, std::string("state sets: ") + hipGetErrorString(e));
        c->sets_bytes = need_sets;
    }
    if (need_mask > c->cmask_bytes) {
        dev_free(c->cmask);
        if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->cmask), need_mask)) != hipSuccess)
            return fail(c, PM_ERR_OOM, std::string("set masks: ") + hipGetErrorString(e));
        c->cmask_bytes = need_mask;
    }
    // up slots: Fitch / Sankoff, subtree form (every leaf present, some S2 / S3 node)
    if ((mode == PM_MODE_FITCH || mode == PM_MODE_SANKOFF) && c->subtree_form && c->ht.num_sshape > 0) {
        const size_t items = (size_t)std::max(c->ht.cl.upm_base + c->ht.cl.n_items,
                                              std::max(c->ht.up_items_k, std::max(c->ht.up_items_g, c->ht.up_items_gs)));
        const size_t need = items * (wpad / kWave) * 4 * sizeof(uint64_t);
        if (need > c->upm_bytes) {
            dev_free(c->upm);
            c->upm_bytes = 0;
            if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->upm), need)) != hipSuccess)
                return fail(c, PM_ERR_OOM, std::string("up slots: ") + hipGetErrorString(e));
            c->upm_bytes = need;
        }
    }
    if (!fitch) {   // Sankoff nodes of out-degree > 255: part counters
        const size_t parts = (size_t)std::max(c->ht.part_off.empty() ? 0 : c->ht.part_off.back(),
                                              std::max(c->ht.part_off_v.empty() ? 0 : c->ht.part_off_v.back(),
                                                       std::max(c->ht.part_off_k.empty() ? 0 : c->ht.part_off_k.back(),
                                                                c->ht.part_off_gs.empty() ? 0 : c->ht.part_off_gs.back())));
        const size_t need = parts * kPartPlanes * wpad * sizeof(uint32_t);
        if (need > c->sk_parts_bytes) {
            dev_free(c->sk_parts);
            if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->sk_parts), need)) != hipSuccess)
                return fail(c, PM_ERR_OOM, std::string("Sankoff part counters: ") + hipGetErrorString(e));
            c->sk_parts_bytes = need;
        }
    }
    if (!c->shard_cnt && (e = dev_alloc(&c->shard_cnt, kShards)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "shard counters");
    if (c->shard_cap == 0) {
        const double nodes = (double)c->dt.num_internal + c->dt.num_leaves;
        const double guess = std::max(65536.0, 0.01 * nodes * (double)c->num_sites);
        const int64_t cap = c->record_cap > 0 ? c->record_cap : (int64_t)(guess * 1.5 / kShards) + 256;
        if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->recs), sizeof(pm_mut) * (size_t)cap * kShards)) != hipSuccess)
            return fail(c, PM_ERR_OOM, std::string("mutation records: ") + hipGetErrorString(e));
        c->shard_cap = cap;
    }
    return PM_OK;
}

// The run's schedule (pm_schedule.cpp), executed by the build of the passes it names: ordinary
// or non-temporal set-record loads (pm_fitch_nt.hip / pm_sankoff_nt.hip; RunPaths::nt).
hipError_t launch_all(pm_ctx* c, int mode) {
    const Schedule s = schedule_run(c->ht, run_opts_of(c), mode);
    // up slots: the subtree form's kernels (alloc_work sizes them for its up orders)
    if (s.paths.sub && c->upm == nullptr) return hipErrorInvalidValue;
    const bool nt = s.paths.nt;
    phase_add("run.nt_loads", nt ? 1.0 : 0.0);   // which build of the passes a launch sequence took
    hipError_t e = s.paths.sankoff ? (nt ? launch_sankoff_nt(c, s) : launch_sankoff(c, s))
                                   : (nt ? launch_fitch_nt(c, s) : launch_fitch(c, s));
    if (e == hipSuccess) e = launch_score(c);
    return e;
}

// Everything a captured run depends on: a different value means a different graph.
uint64_t graph_key_of(const pm_ctx* c, int mode) {
    const RunOpts o = run_opts_of(c);   // every option and fact the schedule reads
    const uint64_t parts[] = {(uint64_t)mode, (uint64_t)(uintptr_t)c->upm, (uint64_t)(uintptr_t)c->sk_parts, (uint64_t)c->num_sites,
                              (uint64_t)c->shard_cap, (uint64_t)(uintptr_t)c->recs, (uint64_t)(uintptr_t)c->sets,
                              (uint64_t)(uintptr_t)c->cmask, (uint64_t)(uintptr_t)c->root_final,
                              (uint64_t)(uintptr_t)c->leaf_planes, (uint64_t)(uintptr_t)c->leaf_present,
                              (uint64_t)(uintptr_t)c->leaf_flag, (uint64_t)(uintptr_t)c->cons,
                              (uint64_t)(uintptr_t)c->forced, (uint64_t)(uintptr_t)c->score,
                              (uint64_t)(uintptr_t)c->root_code, (uint64_t)(uintptr_t)c->shard_cnt,
                              (uint64_t)(uintptr_t)c->sub_planes,
                              (uint64_t)(uintptr_t)c->dt.child_off, (uint64_t)(uintptr_t)c->stream};
    uint64_t h = 1469598103934665603ull;
    const unsigned char* ob = reinterpret_cast<const unsigned char*>(&o);
    for (size_t k = 0; k < sizeof(o); ++k) h = (h ^ ob[k]) * 1099511628211ull;
    for (uint64_t v : parts) h = (h ^ v) * 1099511628211ull;
    return h | 1;
}

int run_once(pm_ctx* c, int mode) {
    hipError_t e;
    if (!c->use_graph) {
        e = launch_all(c, mode);
        if (e != hipSuccess) return hip_fail(c, e, "parsimony launch");
    } else {
        const uint64_t key = graph_key_of(c, mode);
        if (key != c->graph_key) {
            drop_graph(c);
            const bool prof = c->profiling;
            c->profiling = false;   // per-kernel events are not part of the graph
            hipGraph_t g = nullptr;
            e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                const hipError_t le = launch_all(c, mode);
                e = hipStreamEndCapture(c->stream, &g);
                if (e == hipSuccess) e = le;
            }
            c->profiling = prof;
            if (e == hipSuccess) e = hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0);
            if (g) (void)hipGraphDestroy(g);
            if (e != hipSuccess) {
                drop_graph(c);
                return hip_fail(c, e, "graph capture");
            }
            c->graph_key = key;
        }
        timer_begin(c, 4);
        e = hipGraphLaunch(c->graph_exec, c->stream);
        timer_end(c, 4);
        if (e != hipSuccess) return hip_fail(c, e, "graph launch");
    }
    c->ran = true;
    c->last_mode = mode;
    return PM_OK;
}

// Synchronise; if any shard overflowed, grow the record buffer to fit and run again.
int settle(pm_ctx* c, std::vector<uint32_t>& counts) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        counts.assign(kShards, 0);
        hipError_t e = hipMemcpyAsync(counts.data(), c->shard_cnt, sizeof(uint32_t) * kShards,
                                      hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "result sync");
        const uint32_t worst = *std::max_element(counts.begin(), counts.end());
        if ((int64_t)worst <= c->shard_cap) return PM_OK;
        dev_free(c->recs);
        const int64_t cap = (int64_t)worst + worst / 8 + 256;
        if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->recs), sizeof(pm_mut) * (size_t)cap * kShards)) != hipSuccess)
            return fail(c, PM_ERR_OOM, std::string("mutation records: ") + hipGetErrorString(e));
        c->shard_cap = cap;
        int rc = run_once(c, c->last_mode);
        if (rc != PM_OK) return rc;
    }
    return fail(c, PM_ERR_STATE, "mutation record buffer still overflowing");
}

}  // namespace

int settle_run(pm_ctx* c) {
    std::vector<uint32_t> counts;
    return settle(c, counts);
}

hipError_t side_fork(pm_ctx* c) {
    hipError_t e = hipEventRecord(c->ev_fork, c->stream);
    return e == hipSuccess ? hipStreamWaitEvent(c->side, c->ev_fork, 0) : e;
}

hipError_t side_join(pm_ctx* c) {
    hipError_t e = hipEventRecord(c->ev_join, c->side);
    return e == hipSuccess ? hipStreamWaitEvent(c->stream, c->ev_join, 0) : e;
}

void timer_begin(pm_ctx* c, int cls) {
    if (!c->profiling) return;
    auto& v = c->timers[cls];
    if (c->timers_used[cls] == v.size()) {
        Timer t;
        (void)hipEventCreate(&t.a);
        (void)hipEventCreate(&t.b);
        v.push_back(t);
    }
    (void)hipEventRecord(v[c->timers_used[cls]].a, c->stream);
}

void timer_end(pm_ctx* c, int cls) {
    if (!c->profiling) return;
    (void)hipEventRecord(c->timers[cls][c->timers_used[cls]].b, c->stream);
    ++c->timers_used[cls];
}

}  // namespace pm

using namespace pm;

namespace pm {

int build_sub_planes(pm_ctx* c) {
    // (only the subtree form reads it, and that form needs every leaf present)
    if (c->sub_planes_ok || !c->has_tree || !c->has_leaves || !c->leaves_all_present) return PM_OK;
    hipError_t e = hipSuccess;
    if (c->ht.num_tail_s == 0) {
        c->sub_planes_ok = true;
        return PM_OK;
    }
    const size_t need = (size_t)c->ht.num_tail_s * (size_t)wpad_of(c) * 4 * sizeof(uint4);
    if (need > c->sub_planes_bytes) {
        dev_free(c->sub_planes);
        c->sub_planes_bytes = 0;
        if ((e = malloc_or_release(c, reinterpret_cast<void**>(&c->sub_planes), need)) != hipSuccess)
            return fail(c, PM_ERR_OOM, std::string("subtree leaf layout: ") + hipGetErrorString(e));
        c->sub_planes_bytes = need;
    }
    PhaseClock clock;
    if ((e = launch_sub_planes(c)) != hipSuccess) return hip_fail(c, e, "subtree leaf layout");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return hip_fail(c, e, "subtree leaf layout");
    clock.lap("upload.sub_planes");
    c->sub_planes_ok = true;
    return PM_OK;
}

// Leaf columns already on the device (packed codes, [row][row_stride]); every leaf with a
// row is fully present.  Used by drivers that produce the columns on the GPU (reroot).
int leaves_install(pm_ctx* c, int64_t S, const uint8_t* d_codes4, int64_t row_stride, const int32_t* node_row) {
    if (!c->has_tree) return fail(c, PM_ERR_STATE, "upload the tree first");
    if (S <= 0 || S >= (int64_t)1 << 24 || row_stride < (S + 1) / 2) return fail(c, PM_ERR_ARG, "bad leaf columns");
    const int32_t L = c->dt.num_leaves;
    std::vector<int32_t> row_of_leaf(L);
    std::vector<uint8_t> flag(L);
    for (int32_t l = 0; l < L; ++l) {
        row_of_leaf[l] = node_row[c->ht.leaf_id[l]];
        flag[l] = row_of_leaf[l] < 0 ? kLeafAbsent : kLeafPresent;
    }
    int rc = alloc_columns(c, S);
    if (rc != PM_OK) return rc;
    int32_t* d_rows = nullptr;
    hipError_t e = upload(&d_rows, row_of_leaf, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->leaf_flag, flag.data(), L, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_pack_codes(c, d_codes4, row_stride, d_rows, nullptr, 0);
    c->leaves_all_present = std::all_of(flag.begin(), flag.end(), [](uint8_t f) { return f == kLeafPresent; });
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_rows);
    if (e != hipSuccess) return hip_fail(c, e, "leaf install");
    c->has_leaves = true;
    c->sub_planes_ok = false;
    return build_sub_planes(c);
}

}  // namespace pm

extern "C" {

int pm_create(int device, pm_ctx** out) {
    if (!out) return PM_ERR_ARG;
    *out = nullptr;
    PhaseClock clock;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return PM_ERR_HIP;
    if (device < 0 || device >= n) return PM_ERR_ARG;
    if ((e = hipSetDevice(device)) != hipSuccess) return PM_ERR_HIP;
    pm_ctx* c = new pm_ctx();
    c->device = device;
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess) {
        if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
        if (c->side) (void)hipStreamDestroy(c->side);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        delete c;
        return PM_ERR_HIP;
    }
    c->stream = c->own_stream;
    *out = c;
    clock.lap("hip.create_context");
    return PM_OK;
}

int pm_warmup(int device) {
    PhaseClock clock;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return PM_ERR_HIP;
    if (device < 0 || device >= n) return PM_ERR_ARG;
    if ((e = hipSetDevice(device)) != hipSuccess) return PM_ERR_HIP;
    for (auto warm : {warm_fitch, warm_sankoff, warm_fitch_nt, warm_sankoff_nt, warm_replay, warm_synth, warm_sort, warm_scan, warm_vcf, warm_maf, warm_gfa, warm_subnet, warm_aa, warm_mutations, warm_usher, warm_impute})
        if ((e = warm()) != hipSuccess) return PM_ERR_HIP;
    // the runtime's first allocation and staged copies
    void* d = nullptr;
    uint8_t h[4096] = {0};
    if ((e = hipMalloc(&d, sizeof h)) != hipSuccess) return PM_ERR_HIP;
    e = hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    clock.lap("hip.warmup");
    return e == hipSuccess ? PM_OK : PM_ERR_HIP;
}

void pm_destroy(pm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_work(c);
    free_columns(c);
    free_tree(c->dt);
    free_replay(c);
    comm_release(c);
    free_hostio(c);
    for (auto& v : c->timers)
        for (auto& t : v) {
            (void)hipEventDestroy(t.a);
            (void)hipEventDestroy(t.b);
        }
    if (c->side) (void)hipStreamSynchronize(c->side);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* pm_last_error(const pm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pm_set_stream(pm_ctx* c, void* s) {
    if (!c) return PM_ERR_ARG;
    c->stream = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
    return PM_OK;
}

int pm_set_option(pm_ctx* c, int option, int64_t value) {
    if (!c) return PM_ERR_ARG;
    if (option == PM_OPT_SUBTREE) {
        c->subtree_form = value != 0;
        return PM_OK;
    }
    if (option == PM_OPT_VIRTUAL) {
        c->virtual_leaf_parents = value != 0;
        return PM_OK;
    }
    if (option == PM_OPT_NARROW) {
        if (value < 0 || value > 1024) return fail(c, PM_ERR_ARG, "PM_OPT_NARROW: 0..1024 items per level");
        c->narrow_max = (int32_t)value;
        return PM_OK;
    }
    if (option == PM_OPT_UP_GROUP) {
        c->up_group = value != 0;
        return PM_OK;
    }
    if (option == PM_OPT_PLAIN_UP) {   // 0 off, 1 on (default threshold), >= 2: on from that many waves
        if (value < 0) return fail(c, PM_ERR_ARG, "PM_OPT_PLAIN_UP: 0, 1 or a wave threshold >= 2");
        c->plain_up = value != 0;
        c->plain_min_waves = value >= 2 ? value : 0;
        return PM_OK;
    }
    if (option == PM_OPT_SUB_DOWN) {
        c->sub_down = value != 0;
        return PM_OK;
    }
    if (option == PM_OPT_TAIL_PACK) {   // 0 off, 1 on (default threshold), >= 2: on from that many waves, -1: on at any size
        if (value < -1) return fail(c, PM_ERR_ARG, "PM_OPT_TAIL_PACK: -1, 0, 1 or a wave threshold >= 2");
        c->tail_pack = value != 0;
        c->tail_pack_min_waves = value >= 2 ? value : value < 0 ? -1 : 0;
        return PM_OK;
    }
    if (option == PM_OPT_DOWN_PACK) {   // 0 off, 1 on (default threshold), >= 2: on from that many waves, -1: on at any size
        if (value < -1) return fail(c, PM_ERR_ARG, "PM_OPT_DOWN_PACK: -1, 0, 1 or a wave threshold >= 2");
        c->down_pack = value != 0;
        c->down_pack_min_waves = value >= 2 ? value : value < 0 ? -1 : 0;
        return PM_OK;
    }
    if (option == PM_OPT_VCF_BATCH_BYTES) {
        if (value < 4096) return fail(c, PM_ERR_ARG, "PM_OPT_VCF_BATCH_BYTES: at least 4096");
        c->vcf_batch_bytes = value;
        return PM_OK;
    }
    if (option == PM_OPT_MAF_BATCH_BYTES) {
        if (value < 4096) return fail(c, PM_ERR_ARG, "PM_OPT_MAF_BATCH_BYTES: at least 4096");
        c->maf_batch_bytes = value;
        return PM_OK;
    }
    if (option == PM_OPT_GFA_BATCH_BYTES) {
        if (value < 4096) return fail(c, PM_ERR_ARG, "PM_OPT_GFA_BATCH_BYTES: at least 4096");
        c->gfa_batch_bytes = value;
        return PM_OK;
    }
    if (option == PM_OPT_AA_BATCH_BYTES) {
        if (value < 4096) return fail(c, PM_ERR_ARG, "PM_OPT_AA_BATCH_BYTES: at least 4096");
        c->aa_batch_bytes = value;
        return PM_OK;
    }
    if (option == PM_OPT_MUTATIONS_BATCH_BYTES) {
        if (value < 4096) return fail(c, PM_ERR_ARG, "PM_OPT_MUTATIONS_BATCH_BYTES: at least 4096");
        c->mutations_batch_bytes = value;
        return PM_OK;
    }
    if (option == PM_OPT_USHER_BATCH_BYTES) {
        if (value < 4096) return fail(c, PM_ERR_ARG, "PM_OPT_USHER_BATCH_BYTES: at least 4096");
        c->usher_batch_bytes = value;
        return PM_OK;
    }
    if (option == PM_OPT_GFA_IN_BATCH_SITES) {
        if (value < 1 || value > kMaxUploadSites) return fail(c, PM_ERR_ARG, "PM_OPT_GFA_IN_BATCH_SITES: 1 .. 2^24 - 1 sites");
        c->gfa_in_batch_sites = value;
        return PM_OK;
    }
    if (option == PM_OPT_SUBNET_BATCH_ENTRIES) {
        if (value < 1 || value >= ((int64_t)1 << 31) - 1) return fail(c, PM_ERR_ARG, "PM_OPT_SUBNET_BATCH_ENTRIES: 1 .. 2^31 - 2 bases");
        c->subnet_batch_entries = value;
        return PM_OK;
    }
    if (option == PM_OPT_IMPUTE_BATCH_ENTRIES) {
        if (value < 1 || value >= ((int64_t)1 << 31) - 1) return fail(c, PM_ERR_ARG, "PM_OPT_IMPUTE_BATCH_ENTRIES: 1 .. 2^31 - 2 bases");
        c->impute_batch_entries = value;
        return PM_OK;
    }
    if (option == PM_OPT_REROOT_CHUNK_SITES) {
        if (value < 0 || value > kMaxRerootChunk) return fail(c, PM_ERR_ARG, "PM_OPT_REROOT_CHUNK_SITES: 0 (by the tree's size) or 1 .. 2^24 - 4096 columns");
        c->reroot_chunk_sites = value;
        return PM_OK;
    }
    if (option == PM_OPT_GROUP_WAVES) {
        if (value < 0) return fail(c, PM_ERR_ARG, "PM_OPT_GROUP_WAVES: >= 0 waves");
        c->group_waves = value;
        return PM_OK;
    }
    if (option == PM_OPT_GROUP_LEVELS) {
        if (value < 2 || value > 4) return fail(c, PM_ERR_ARG, "PM_OPT_GROUP_LEVELS: 2 to 4");
        c->group_levels = (int32_t)value;
        return PM_OK;
    }
    if (option == PM_OPT_RECORD_CAP) {
        if (value < 1 || value > ((int64_t)1 << 31)) return fail(c, PM_ERR_ARG, "PM_OPT_RECORD_CAP: 1 .. 2^31 records per shard");
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        drop_graph(c);
        dev_free(c->recs);
        c->shard_cap = 0;   // the next run allocates record_cap per shard
        c->record_cap = value;
        c->ran = false;
        return PM_OK;
    }
    if (option == PM_OPT_NT_LOADS) {
        if (value < -1 || value > 1) return fail(c, PM_ERR_ARG, "PM_OPT_NT_LOADS: -1 (by level size), 0 or 1");
        c->nt_loads = (int32_t)value;
        return PM_OK;
    }
    // 0 off (and no plan at the next tree upload: the grouped post-order covers every level);
    // 1 on (the default plan); >= 2 on, that level threshold and no bushiness test (next tree upload)
    if (option == PM_OPT_CLUSTER) {
        if (value < 0 || value > ((int64_t)1 << 30)) return fail(c, PM_ERR_ARG, "PM_OPT_CLUSTER: 0, 1 or a level size >= 2");
        c->cluster = value != 0;
        c->cluster_max_level = value == 0 ? 0 : value == 1 ? kClMaxLevel : (int32_t)value;
        c->cluster_chain = value == 1;
        return PM_OK;
    }
    if (option == PM_OPT_GRAPH) {
        c->use_graph = value != 0;
        if (!c->use_graph) drop_graph(c);
        return PM_OK;
    }
    return fail(c, PM_ERR_ARG, "unknown option");
}

int pm_set_profiling(pm_ctx* c, int enable) {
    if (!c) return PM_ERR_ARG;
    c->profiling = enable != 0;
    for (auto& u : c->timers_used) u = 0;
    return PM_OK;
}

int pm_tree_upload(pm_ctx* c, const pm_tree* t) {
    if (!c || !t || !t->child_offsets || t->num_nodes < 2) return fail(c, PM_ERR_ARG, "bad tree");
    (void)hipSetDevice(c->device);
    c->sub_planes_ok = false;   // its S2 / S3 nodes are this tree's
    // the host plan (pm_plan.cpp); a tree it refuses leaves the context's tree as it was
    TreePlan p;
    std::string err;
    if (const int rc = plan_tree(*t, c->cluster_max_level, c->cluster_chain, p, err)) return fail(c, rc, err);
    PhaseClock clock;
    free_work(c);
    free_columns(c);
    free_tree(c->dt);
    DevTree dt;
    size_t tree_bytes = 0;
    const hipError_t e = upload_tree(p, c->stream, dt, tree_bytes);
    if (e != hipSuccess) return hip_fail(c, e, "tree upload");
    ClusterPlan& cl = p.ht.cl;
    cl.items.clear();   // (device only)
    cl.items.shrink_to_fit();
    cl.down_items.clear();
    cl.down_items.shrink_to_fit();
    cl.item_of.clear();
    cl.item_of.shrink_to_fit();
    c->dt = dt;
    c->tree_bytes = tree_bytes;
    c->ht = std::move(p.ht);
    c->max_degree = 0;
    for (int32_t d = 0; d < dt.num_internal; ++d) c->max_degree = std::max(c->max_degree, c->ht.child_off[d + 1] - c->ht.child_off[d]);
    c->has_tree = true;
    tree_phase(clock, "device upload");
    return PM_OK;
}

int pm_leaves_upload(pm_ctx* c, int64_t S, const uint8_t* codes4, int64_t row_stride, const int32_t* node_row,
                     const uint8_t* present, int64_t present_stride) {
    if (!c) return PM_ERR_ARG;
    if (!c->has_tree) return fail(c, PM_ERR_STATE, "upload the tree first");
    if (S <= 0 || S >= (int64_t)1 << 24 || !codes4 || !node_row || row_stride < (S + 1) / 2)
        return fail(c, PM_ERR_ARG, "bad leaf matrix arguments (0 < sites < 2^24)");
    if (present && present_stride < (S + 7) / 8) return fail(c, PM_ERR_ARG, "bad presence stride");
    (void)hipSetDevice(c->device);
    const int32_t L = c->dt.num_leaves;
    std::vector<int32_t> row_of_leaf(L);
    std::vector<uint8_t> flag(L);
    int32_t rows = 0;
    for (int32_t l = 0; l < L; ++l) {
        row_of_leaf[l] = node_row[c->ht.leaf_id[l]];
        flag[l] = row_of_leaf[l] < 0 ? kLeafAbsent : (present ? kLeafPartial : kLeafPresent);
        rows = std::max(rows, row_of_leaf[l] + 1);
    }
    int rc = alloc_columns(c, S);
    if (rc != PM_OK) return rc;
    const int64_t wpad = wpad_of(c);
    hipError_t e;
    if (present && (e = dev_alloc(&c->leaf_present, (size_t)L * wpad)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "presence planes");
    uint8_t* d_codes = nullptr;
    uint8_t* d_present = nullptr;
    int32_t* d_rows = nullptr;
    const size_t code_bytes = (size_t)rows * row_stride;
    const size_t pres_bytes = present ? (size_t)rows * present_stride : 0;
    if ((e = dev_alloc(&d_codes, code_bytes)) != hipSuccess || (e = upload(&d_rows, row_of_leaf, c->stream)) != hipSuccess ||
        (present && (e = dev_alloc(&d_present, pres_bytes)) != hipSuccess)) {
        dev_free(d_codes);
        dev_free(d_rows);
        dev_free(d_present);
        return fail(c, PM_ERR_OOM, "leaf staging");
    }
    e = hipMemcpyAsync(d_codes, codes4, code_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && present) e = hipMemcpyAsync(d_present, present, pres_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->leaf_flag, flag.data(), L, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_pack_codes(c, d_codes, row_stride, d_rows, d_present, present_stride);
    c->leaves_all_present = std::all_of(flag.begin(), flag.end(), [](uint8_t f) { return f == kLeafPresent; });
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d_codes);
    dev_free(d_rows);
    dev_free(d_present);
    if (e != hipSuccess) return hip_fail(c, e, "leaf upload");
    c->has_leaves = true;
    c->sub_planes_ok = false;
    return build_sub_planes(c);
}

int pm_leaves_upload_sparse(pm_ctx* c, int64_t S, int32_t num_rows, const int64_t* row_off, const int32_t* site,
                            const uint8_t* code, uint8_t fill_code, const int32_t* node_row) {
    if (!c) return PM_ERR_ARG;
    if (!c->has_tree) return fail(c, PM_ERR_STATE, "upload the tree first");
    if (S <= 0 || S >= (int64_t)1 << 24 || num_rows < 0 || !row_off || !node_row || fill_code > 15)
        return fail(c, PM_ERR_ARG, "bad leaf matrix arguments (0 < sites < 2^24)");
    if (row_off[0] != 0) return fail(c, PM_ERR_ARG, "sparse leaf rows: row_off[0] must be 0");
    const int64_t nnz = row_off[num_rows];
    if (nnz > 0 && (!site || !code)) return fail(c, PM_ERR_ARG, "bad leaf matrix arguments (0 < sites < 2^24)");
    for (int32_t r = 0; r < num_rows; ++r) {
        if (row_off[r + 1] < row_off[r]) return fail(c, PM_ERR_ARG, "sparse leaf rows: row_off decreases at row " + std::to_string(r));
        for (int64_t i = row_off[r]; i < row_off[r + 1]; ++i) {
            if (site[i] < 0 || site[i] >= S)
                return fail(c, PM_ERR_ARG, "sparse leaf rows: site out of range in row " + std::to_string(r));
            if (i > row_off[r] && site[i] <= site[i - 1])
                return fail(c, PM_ERR_ARG, "sparse leaf rows: sites not strictly increasing in row " + std::to_string(r));
            if (code[i] > 15) return fail(c, PM_ERR_ARG, "sparse leaf rows: code above 15 in row " + std::to_string(r));
        }
    }
    for (int32_t l = 0; l < c->dt.num_leaves; ++l)
        if (node_row[c->ht.leaf_id[l]] >= num_rows)
            return fail(c, PM_ERR_ARG, "sparse leaf rows: node_row names row " + std::to_string(node_row[c->ht.leaf_id[l]]) +
                                           " of " + std::to_string(num_rows));
    (void)hipSetDevice(c->device);
    // staging rows of whole 32-bit words, expanded on the device from the three arrays
    const int64_t stride_words = ((S + 1) / 2 + 3) / 4;
    int64_t* d_off = nullptr;
    int32_t* d_site = nullptr;
    uint8_t* d_code = nullptr;
    uint32_t* d_rows4 = nullptr;
    hipError_t e;
    if ((e = dev_alloc(&d_off, (size_t)num_rows + 1)) != hipSuccess || (e = dev_alloc(&d_site, (size_t)nnz)) != hipSuccess ||
        (e = dev_alloc(&d_code, (size_t)nnz)) != hipSuccess ||
        (e = dev_alloc(&d_rows4, (size_t)num_rows * stride_words)) != hipSuccess) {
        dev_free(d_off);
        dev_free(d_site);
        dev_free(d_code);
        dev_free(d_rows4);
        return fail(c, PM_ERR_OOM, "leaf staging");
    }
    e = hipMemcpyAsync(d_off, row_off, sizeof(int64_t) * ((size_t)num_rows + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(d_site, site, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(d_code, code, (size_t)nnz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_expand_sparse(c, d_off, d_site, d_code, fill_code, num_rows, stride_words, d_rows4);
    int rc = PM_OK;
    if (e != hipSuccess) rc = hip_fail(c, e, "leaf upload");
    // (leaves_install synchronises the stream before it returns: the host arrays are free then)
    else rc = leaves_install(c, S, reinterpret_cast<const uint8_t*>(d_rows4), stride_words * 4, node_row);
    if (e != hipSuccess) (void)hipStreamSynchronize(c->stream);
    dev_free(d_off);
    dev_free(d_site);
    dev_free(d_code);
    dev_free(d_rows4);
    return rc;
}

int pm_sites_upload(pm_ctx* c, const uint8_t* consensus4, const uint8_t* forced4) {
    if (!c || !consensus4) return fail(c, PM_ERR_ARG, "consensus required");
    if (!c->has_leaves) return fail(c, PM_ERR_STATE, "upload the leaves first");
    (void)hipSetDevice(c->device);
    const size_t bytes = (size_t)(c->num_sites + 1) / 2;
    uint8_t* d = nullptr;
    hipError_t e = dev_alloc(&d, bytes);
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, "site staging");
    e = hipMemcpyAsync(d, consensus4, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_pack_sites(c, d, c->cons);
    if (e == hipSuccess && forced4) {
        e = hipMemcpyAsync(d, forced4, bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = launch_pack_sites(c, d, c->forced);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d);
    if (e != hipSuccess) return hip_fail(c, e, "site upload");
    c->has_forced = forced4 != nullptr;
    c->has_sites = true;
    return PM_OK;
}

int pm_run(pm_ctx* c, int mode) {
    if (!c) return PM_ERR_ARG;
    if (mode < PM_MODE_FITCH || mode > PM_MODE_BLOCK_SANKOFF) return fail(c, PM_ERR_ARG, "unknown mode");
    if (!c->has_tree || !c->has_leaves || !c->has_sites) return fail(c, PM_ERR_STATE, "tree, leaves and sites first");
    (void)hipSetDevice(c->device);
    int rc = alloc_work(c, mode);
    if (rc == PM_OK) rc = build_sub_planes(c);   // (current after every upload; a new tree resets it)
    if (rc != PM_OK) return rc;
    return run_once(c, mode);
}

int pm_mutation_count(pm_ctx* c, int64_t* count) {
    if (!c || !count) return PM_ERR_ARG;
    if (!c->ran) return fail(c, PM_ERR_STATE, "nothing ran");
    std::vector<uint32_t> counts;
    int rc = settle(c, counts);
    if (rc != PM_OK) return rc;
    int64_t n = 0;
    for (uint32_t k : counts) n += k;
    *count = n;
    return PM_OK;
}

int pm_mutations_fetch(pm_ctx* c, pm_mut* out, int64_t cap, int64_t* count) {
    if (!c || !count) return PM_ERR_ARG;
    if (!c->ran) return fail(c, PM_ERR_STATE, "nothing ran");
    std::vector<uint32_t> counts;
    int rc = settle(c, counts);
    if (rc != PM_OK) return rc;
    int64_t n = 0;
    for (uint32_t k : counts) n += k;
    *count = n;
    if (!out) return PM_OK;
    if (cap < n) return fail(c, PM_ERR_ARG, "output capacity too small");
    if (n <= INT32_MAX) {   // device radix sort (pm_sort.hip), one D2H copy
        const hipError_t e = sort_records_to_host(c, counts, n, out);
        return e == hipSuccess ? PM_OK : hip_fail(c, e, "record sort");
    }
    int64_t at = 0;
    for (int s = 0; s < kShards; ++s) {
        if (!counts[s]) continue;
        hipError_t e = hipMemcpyAsync(out + at, c->recs + (size_t)s * c->shard_cap, sizeof(pm_mut) * counts[s],
                                      hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "record download");
        at += counts[s];
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "record download");
    std::sort(out, out + n, [](const pm_mut& a, const pm_mut& b) {
        return a.node != b.node ? a.node < b.node : a.site_info < b.site_info;
    });
    return PM_OK;
}

int pm_site_results(pm_ctx* c, int32_t* score, uint8_t* root_code) {
    if (!c) return PM_ERR_ARG;
    if (!c->ran) return fail(c, PM_ERR_STATE, "nothing ran");
    std::vector<uint32_t> counts;
    int rc = settle(c, counts);
    if (rc != PM_OK) return rc;
    hipError_t e = hipSuccess;
    if (score) e = hipMemcpyAsync(score, c->score, sizeof(int32_t) * c->num_sites, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && root_code)
        e = hipMemcpyAsync(root_code, c->root_code, c->num_sites, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? PM_OK : hip_fail(c, e, "site results");
}

int pm_site_results_device(pm_ctx* c, void* score_device, void* root_device) {
    if (!c) return PM_ERR_ARG;
    if (!c->ran) return fail(c, PM_ERR_STATE, "nothing ran");
    const int rc = settle_run(c);
    if (rc != PM_OK) return rc;
    hipError_t e = hipSuccess;
    if (score_device)
        e = hipMemcpyAsync(score_device, c->score, sizeof(int32_t) * c->num_sites, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && root_device)
        e = hipMemcpyAsync(root_device, c->root_code, c->num_sites, hipMemcpyDeviceToDevice, c->stream);
    return e == hipSuccess ? PM_OK : hip_fail(c, e, "site results (device)");
}

int pm_kernel_times(pm_ctx* c, double* ms, int64_t* launches, int classes) {
    if (!c || !ms || !launches) return PM_ERR_ARG;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "timer sync");
    for (int k = 0; k < classes; ++k) {
        ms[k] = 0.0;
        launches[k] = 0;
        if (k >= kClasses) continue;
        for (size_t i = 0; i < c->timers_used[k]; ++i) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, c->timers[k][i].a, c->timers[k][i].b) == hipSuccess) ms[k] += t;
        }
        launches[k] = (int64_t)c->timers_used[k];
        c->timers_used[k] = 0;
    }
    return PM_OK;
}

int pm_synth_columns(pm_ctx* c, int64_t site_begin, int64_t S, uint64_t seed) {
    if (!c) return PM_ERR_ARG;
    if (!c->has_tree) return fail(c, PM_ERR_STATE, "upload the tree first");
    if (S <= 0 || S >= (int64_t)1 << 24 || site_begin < 0) return fail(c, PM_ERR_ARG, "bad site range");
    (void)hipSetDevice(c->device);
    int rc = alloc_columns(c, S);
    if (rc != PM_OK) return rc;
    // the generator stages internal sequences in `finals` ([I][W] uint4), scratch freed after it
    // (15 GB at 1M leaves x 30k sites that a run does not need)
    hipError_t e = dev_alloc(&c->finals, (size_t)c->dt.num_internal * wpad_of(c));
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, std::string("generator scratch: ") + hipGetErrorString(e));
    c->finals_bytes = sizeof(uint4) * (size_t)c->dt.num_internal * wpad_of(c);
    std::vector<uint8_t> flag(c->dt.num_leaves, kLeafPresent);
    e = hipMemcpyAsync(c->leaf_flag, flag.data(), flag.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_synth(c, site_begin, seed);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(c->finals);
    c->finals_bytes = 0;
    if (e != hipSuccess) return hip_fail(c, e, "synthetic columns");
    c->has_leaves = c->has_sites = true;
    c->leaves_all_present = true;
    c->has_forced = false;
    c->sub_planes_ok = false;
    return build_sub_planes(c);
}

int pm_leaf_codes_fetch(pm_ctx* c, int64_t s0, int64_t ns, uint8_t* out) {
    if (!c || !out || s0 < 0 || ns <= 0) return fail(c, PM_ERR_ARG, "bad range");
    if (!c->has_leaves || s0 + ns > c->num_sites) return fail(c, PM_ERR_STATE, "range outside the uploaded sites");
    (void)hipSetDevice(c->device);
    uint8_t* d = nullptr;
    const size_t bytes = (size_t)c->dt.num_leaves * ns;
    hipError_t e = dev_alloc(&d, bytes);
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, "fetch staging");
    e = launch_unpack_leaf_codes(c, s0, ns, d);
    std::vector<uint8_t> by_rank(bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(by_rank.data(), d, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d);
    if (e != hipSuccess) return hip_fail(c, e, "leaf fetch");
    // rows by leaf rank (tree order) -> rows in increasing node-id order
    std::vector<int32_t> ranks(c->dt.num_leaves);
    std::iota(ranks.begin(), ranks.end(), 0);
    std::sort(ranks.begin(), ranks.end(), [&](int32_t x, int32_t y) { return c->ht.leaf_id[x] < c->ht.leaf_id[y]; });
    for (size_t k = 0; k < ranks.size(); ++k)
        std::memcpy(out + k * ns, by_rank.data() + (size_t)ranks[k] * ns, (size_t)ns);
    return PM_OK;
}

int pm_consensus_fetch(pm_ctx* c, int64_t s0, int64_t ns, uint8_t* out) {
    if (!c || !out || s0 < 0 || ns <= 0) return fail(c, PM_ERR_ARG, "bad range");
    if (!c->has_sites || s0 + ns > c->num_sites) return fail(c, PM_ERR_STATE, "range outside the uploaded sites");
    (void)hipSetDevice(c->device);
    uint8_t* d = nullptr;
    hipError_t e = dev_alloc(&d, (size_t)ns);
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, "fetch staging");
    e = launch_unpack_sites(c, c->cons, s0, ns, d);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, ns, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(d);
    return e == hipSuccess ? PM_OK : hip_fail(c, e, "consensus fetch");
}

}  // extern "C"
