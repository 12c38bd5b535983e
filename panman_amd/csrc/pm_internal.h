// pm_internal.h -- context layout shared by the host side and the kernel launchers.
//
// HBM layout (one pm_ctx = one GPU = one shard of S sites, W = ceil(S/32) words):
//   leaf planes   [L][W] uint4     4 code bit-planes of 32 sites (16 B / 32 sites)
//   leaf present  [L][W] uint32    only for leaves with partially present columns
//   Fitch sets    [I][tile] records: 4 code planes per word; a word holding a multi-code or
//                 empty set adds its multi-code sites' 16-bit sets (compact complex lanes,
//                 pm_kernels.h store_fitch_set)
//   Sankoff sets  [I][W][32] u32   Z0 (optimal codes) + Z1 (one above optimal) planes
//   finals        the root's in root_final [W] uint4; every other internal node's in its
//                 record (complex lanes: quad 0 of the lane's slot; others: the record code)
//   consensus     [W] uint4        root's parent state; forced [W] uint4 (optional)
//   records       [shards][cap]    pm_mut, sharded write cursors (one atomic per wave)
// Internal nodes are addressed by a dense index (0..I-1), leaves by their rank among
// leaf node ids (0..L-1).  A child is encoded as its dense internal index (>= 0) or
// -(leaf rank + 1).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/panman_gpu.h"
#include "pm_schedule.h"   // over pm_plan.h (the planner's constants and records, HostTree, the phase log and host threads): the launch schedule and the constants it reads

namespace pm {

#ifndef PM_SHARDS
#define PM_SHARDS 1024
#endif
constexpr int kShards = PM_SHARDS;
constexpr int kClasses = 6;   // post-order, pre-order levels, score, replay, whole graph, pre-order tail
// Record quads per word (kCxCompact: pm_schedule.h): simple area + complex areas.
constexpr int kFitchRecQuads = kCxCompact ? 6 : 5;
constexpr int kMaskWords = 8;     // record masks per (node, tile): complex, simple, dirty, parent's
                                  // complex, parent's simple, an S2 / S3 node's pushed dirty lanes,
                                  // Fitch: the first / second child's dirty lanes (one 64-B line)
// The most sites one leaf upload takes (a record's site field is 24 bits; pm_leaves_upload).
constexpr int64_t kMaxUploadSites = ((int64_t)1 << 24) - 1;
// The most canonical columns pm_reroot hands the nucleotide Fitch at once (PM_OPT_REROOT_CHUNK_SITES).
constexpr int64_t kMaxRerootChunk = ((int64_t)1 << 24) - 4096;
// pm_subnet's default batch (PM_OPT_SUBNET_BATCH_ENTRIES), in expanded bases.  hipCUB takes its item count as an
// int, so a batch must stay below 2^31; a base costs about 110 B of device memory across the pipeline (two
// 8-B key and two 8-B value buffers, 12 B of coordinates, 9 B of fold results, then up to 33 B per survivor and
// 17 B per record), and hipCUB's temporaries are histograms, independent of the count.  2^25 bases is 1 / 64 of
// the int range and about 3.5 GiB, a small part of the device's memory.
constexpr int64_t kSubnetBatchEntries = (int64_t)1 << 25;

enum LeafFlag : uint8_t { kLeafAbsent = 0, kLeafPresent = 1, kLeafPartial = 2 };

// The tree on the device: the arrays of a TreePlan (pm_plan.h), each under the same name.
struct DevTree {
    int32_t num_internal = 0;
    int32_t num_leaves = 0;
    int32_t root_dense = -1;          // dense index of the root (internal)
    int32_t* child_off = nullptr;     // [I+1] over dense internal index
    int32_t* child_enc = nullptr;     // [E]
    int32_t* parent_dense = nullptr;  // [I] parent dense index, -1 for the root
    int32_t* internal_id = nullptr;   // [I] caller node id
    int32_t* leaf_id = nullptr;       // [L] caller node id
    int32_t* up_order = nullptr;      // [I] dense indices grouped by height (post-order levels)
    int32_t* down_order = nullptr;    // [I] dense indices grouped by depth (pre-order levels)
    int32_t* leaf_parent = nullptr;   // [L] parent dense index (synthetic generator)
    int32_t* leaf_down = nullptr;     // [L] leaf ranks grouped by depth (synthetic generator)
    // Fitch with "virtual" leaf-parents: an internal node whose children are all leaves
    // (<= 4) is never materialised; its parent evaluates it from the leaves in both passes
    int32_t* child_enc_v = nullptr;   // [E] as child_enc, virtual children tagged kVirtualBit
    int32_t* up_order_v = nullptr;    // [I'] materialised internal nodes by height
    int32_t* down_order_v = nullptr;  // [I'] materialised internal nodes by depth
    // down-pass item descriptors {node, parent, first child, end child} (int4), in
    // down_order / down_order_v order, and each virtual node's leaves (int4, -1 padded)
    NodeDesc* down_desc = nullptr;
    NodeDesc* up_desc = nullptr;      // in up_order order
    NodeDesc* up_desc_v = nullptr;
    NodeDesc* down_desc_v = nullptr;
    int32_t* vleaf = nullptr;
    TailDesc* tail_desc = nullptr;     // tails over child_enc
    TailDesc* tail_desc_v = nullptr;   // tails over child_enc_v
    // Sankoff parts of the nodes of out-degree > 255 ([0] over child_enc, [1] over child_enc_v)
    PartDesc* part_desc = nullptr;
    PartDesc* part_desc_v = nullptr;
    PartDesc* part_desc_k = nullptr;   // subtree form (Sankoff)
    PartDesc* part_desc_gs = nullptr;  // grouped subtree form (Sankoff)
    // subtree form (Fitch, all leaves present): S2 / S3 nodes inline in their parent too
    int32_t* child_enc_k = nullptr;   // [E] shapes in bits 28-29
    NodeDesc* up_desc_k = nullptr;
    NodeDesc* up_desc_g = nullptr;     // grouped post-order launches of the subtree form
    NodeDesc* up_desc_gs = nullptr;    // ... Sankoff's (binary recomputed children; pad0 = first part above 255 children)
    NodeDesc* down_desc_k = nullptr;
    NodeDesc* down_desc_ks = nullptr;  // ... with their S2 / S3 children kept (PM_OPT_SUB_DOWN)
    int32_t* vinner = nullptr;        // [I][2] an S2 / S3 node's cherries (dense), -1 padded
    // up slots (UpArgs::upm): per up_desc_k / up_desc_g item, parent item * 2 + slot, or -1
    int32_t* pslot_k = nullptr;
    int32_t* pslot_g = nullptr;
    int32_t* pslot_gs = nullptr;      // ... of up_desc_gs (Sankoff's groups)
    TailDesc* tail_desc_k = nullptr;  // tails of the leaf-parent form + every S2 / S3 node
    // LDS-staged post-order sweeps (ClusterPlan on the device)
    NodeDesc* cl_items = nullptr;
    NodeDesc* cl_down_items = nullptr;
    int32_t* cl_wg_off = nullptr;
    int32_t* cl_slot_of = nullptr;
    // up slots with the sweeps (UpArgs::upm: the level items', then the sweep items' at
    // up_items_k + item): the level items' pslot, and each sweep item's (its parent in a later band)
    int32_t* pslot_kc = nullptr;
    int32_t* pslot_gc = nullptr;
    int32_t* cl_pslot = nullptr;
    // level tables on the device (the narrow-band launches walk several levels): the host
    // arrays up_class_off{,_v,_k}, down_level_off{,_v,_k}, down_dense_base_k back to back
    int32_t* lvl = nullptr;
};

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
};

}  // namespace pm

namespace pm { struct ReplayState; }

struct pm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    // a second stream for independent launches of one level (side_fork / side_join)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;

    pm::HostTree ht;
    pm::DevTree dt;
    size_t tree_bytes = 0;            // device bytes of the flattened tree (descriptors, level tables)
    bool has_tree = false;
    int32_t max_degree = 0;
    bool virtual_leaf_parents = true; // Fitch: leaf-parents evaluated inline (PM_OPT_VIRTUAL)
    bool subtree_form = true;         // Fitch, all leaves present: S2 / S3 inline too (PM_OPT_SUBTREE)
    int32_t narrow_max = 16;          // Fitch: runs of levels this narrow go to one band launch (PM_OPT_NARROW)
    int64_t group_waves = 32768;      // Fitch: pre-order levels grouped into one launch up to this many waves (PM_OPT_GROUP_WAVES)
    int32_t group_levels = 4;         // ... and up to this many levels (PM_OPT_GROUP_LEVELS)
    bool up_group = true;             // Fitch subtree form: grouped post-order launches (PM_OPT_UP_GROUP)
    bool sub_down = false;            // Fitch subtree form: S2 / S3 records in their parent's pre-order wave (PM_OPT_SUB_DOWN)
    bool tail_pack = true;            // Fitch subtree form: the tail's S2 / S3 items in groups per wave, dirty words gathered into full waves (PM_OPT_TAIL_PACK)
    int64_t tail_pack_min_waves = 0;  // ... from this many (S item, tile) waves (0: kTailPackMinWaves, -1: always)
    bool down_pack = true;            // Fitch, all leaves present: large dense pre-order levels in groups per wave, live words gathered into full waves (PM_OPT_DOWN_PACK)
    int64_t down_pack_min_waves = 0;  // ... from this many (item, tile) waves (0: kDownPackMinWaves, -1: always)
    bool plain_up = true;             // grouped subtree form: plain nodes in the lean post-order kernels (PM_OPT_PLAIN_UP)
    int64_t plain_min_waves = 0;      // ... from this many (node, tile) waves (0: kPlainMinWaves)
    bool cluster = true;              // Fitch subtree form: LDS-staged post-order sweeps above ht.cl.h0 (PM_OPT_CLUSTER)
    int32_t cluster_max_level = pm::kClMaxLevel;   // ... their plan's level threshold (at tree upload)
    bool cluster_chain = true;        // ... and only above the last bushy band (the default; an explicit threshold: off)

    // column shard
    int64_t num_sites = 0;
    int32_t words = 0;
    uint4* leaf_planes = nullptr;     // [L][W]
    uint32_t* leaf_present = nullptr; // [L][W] (allocated only when needed)
    uint8_t* leaf_flag = nullptr;     // [L]
    uint4* cons = nullptr;            // [W]
    uint4* forced = nullptr;          // [W]
    bool has_forced = false;
    bool has_leaves = false;
    bool leaves_all_present = false;   // every leaf row present at every site
    bool has_sites = false;

    // work buffers
    uint32_t* sets = nullptr;         // Fitch: [I][tile] 320 uint4 records; Sankoff: [I][W][32]
    size_t sets_bytes = 0;
    uint64_t* cmask = nullptr;        // Fitch: [I][tile] complex-lane masks
    size_t cmask_bytes = 0;
    uint64_t* upm = nullptr;          // Fitch subtree form: [up items][tile][4] up slots (UpArgs::upm)
    size_t upm_bytes = 0;
    uint4* finals = nullptr;          // [I][W] synthetic generator scratch (internal sequences)
    size_t finals_bytes = 0;
    uint32_t* sk_parts = nullptr;     // Sankoff part counters [parts][kPartPlanes][wpad]
    size_t sk_parts_bytes = 0;
    uint4* root_final = nullptr;      // [W] the root's final codes (other finals live in the records)
    pm_mut* recs = nullptr;           // [kShards][shard_cap]
    int64_t shard_cap = 0;
    int64_t record_cap = 0;           // PM_OPT_RECORD_CAP: first allocation per shard (0 = a guess)
    uint32_t* shard_cnt = nullptr;    // [kShards]
    // subtree form: each S2 / S3 node's three or four leaf words side by side per word
    // ([num_tail_s][wpad][4] uint4, built from leaf_planes by build_sub_planes), so a wave that
    // reads a subtree's leaves at scattered lanes draws one 64-B sector per lane, not four
    uint4* sub_planes = nullptr;
    size_t sub_planes_bytes = 0;
    bool sub_planes_ok = false;
    int32_t* score = nullptr;         // [S]
    uint8_t* root_code = nullptr;     // [S]
    bool ran = false;
    int last_mode = -1;

    // profiling
    bool profiling = false;
    std::vector<pm::Timer> timers[pm::kClasses];
    size_t timers_used[pm::kClasses] = {0, 0, 0, 0, 0, 0};

    // hipGraph of one pm_run (PM_OPT_GRAPH): captured on first use, replayed while the
    // launch sequence and every buffer it touches stay the same (graph_key)
    bool use_graph = false;
    int32_t nt_loads = -1;            // PM_OPT_NT_LOADS: -1 by level size (RunPaths::nt), 0 off, 1 on
    hipGraphExec_t graph_exec = nullptr;
    uint64_t graph_key = 0;

    // replay (pm_replay.cpp)
    pm::ReplayState* replay = nullptr;

    // multi-GPU column shards (pm_rccl.hip): RCCL communicator + gather buffers
    void* comm = nullptr;             // ncclComm_t
    int comm_rank = 0, comm_size = 1;
    void* gather_buf = nullptr;       // [send chunk | ranks x chunk] packed site results
    size_t gather_bytes = 0;

    // grow-only buffers kept between calls (pm_hostio.cpp): pinned download slots, the FASTA
    // text and replay rows on the device
    void* stage = nullptr;
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr};
    void* text_buf = nullptr;
    size_t text_cap = 0;
    void* rows_buf = nullptr;
    size_t rows_cap = 0;

    int64_t vcf_batch_bytes = (int64_t)1 << 30;   // pm_vcf: genotype text per device batch (PM_OPT_VCF_BATCH_BYTES)
    int64_t maf_batch_bytes = (int64_t)1 << 30;   // pm_maf: text per device batch of whole lines (PM_OPT_MAF_BATCH_BYTES)
    int64_t gfa_batch_bytes = (int64_t)1 << 30;   // pm_gfa: text per device batch of whole P lines (PM_OPT_GFA_BATCH_BYTES)
    int64_t gfa_in_batch_sites = pm::kMaxUploadSites; // pm_gfa_build: block columns per upload and run (PM_OPT_GFA_IN_BATCH_SITES)
    int64_t aa_batch_bytes = (int64_t)1 << 30;    // pm_aa: codon tables and text per device batch of nodes (PM_OPT_AA_BATCH_BYTES)
    int64_t mutations_batch_bytes = (int64_t)1 << 30;   // pm_print_mutations: entry records and text per device batch of nodes (PM_OPT_MUTATIONS_BATCH_BYTES)
    int64_t usher_batch_bytes = (int64_t)1 << 30;   // pm_to_usher: entry records, sort keys and bytes per device batch of nodes (PM_OPT_USHER_BATCH_BYTES)
    int64_t subnet_batch_entries = pm::kSubnetBatchEntries;   // pm_subnet: expanded bases sorted per batch (PM_OPT_SUBNET_BATCH_ENTRIES)
    int64_t impute_batch_entries = pm::kSubnetBatchEntries;   // pm_impute: expanded bases of whole pairs sorted per batch (PM_OPT_IMPUTE_BATCH_ENTRIES)
    int64_t reroot_chunk_sites = 0;               // pm_reroot: canonical columns per Fitch chunk, 0 = by the tree's size (PM_OPT_REROOT_CHUNK_SITES)
};

namespace pm {

int fail(pm_ctx* c, int code, const std::string& msg);
// Synchronise after a run; if a record shard overflowed, grow the buffer and run again (the
// per-site score only counts stored records).  pm_host.cpp.
int settle_run(pm_ctx* c);
int hip_fail(pm_ctx* c, hipError_t e, const char* what);

// Work queued on c->side between side_fork and side_join runs concurrently with the work
// queued on c->stream meanwhile (in a captured graph: parallel branches).
hipError_t side_fork(pm_ctx* c);
hipError_t side_join(pm_ctx* c);
void timer_begin(pm_ctx* c, int cls);
void timer_end(pm_ctx* c, int cls);

// kernel launchers (pm_fitch.hip / pm_sankoff.hip / pm_synth.hip)
hipError_t launch_fitch(pm_ctx* c, const Schedule& s);
hipError_t launch_sankoff(pm_ctx* c, const Schedule& s);
hipError_t launch_fitch_nt(pm_ctx* c, const Schedule& s);     // non-temporal set-record loads
hipError_t launch_sankoff_nt(pm_ctx* c, const Schedule& s);
// What a run's launch sequence depends on besides the tree (schedule_run, graph_key_of).
inline RunOpts run_opts_of(const pm_ctx* c) {   // (in RunOpts' field order)
    return RunOpts{c->virtual_leaf_parents, c->subtree_form, c->narrow_max, c->group_waves, c->group_levels, c->up_group,
                   c->sub_down, c->tail_pack, c->tail_pack_min_waves, c->down_pack, c->down_pack_min_waves, c->plain_up,
                   c->plain_min_waves, c->cluster, c->nt_loads, c->leaves_all_present, c->has_forced,
                   (c->words + kWave - 1) / kWave};
}
// Records of the last run, sorted by (node, site) on the device, copied to host `out`.
// pm_warmup: one kernel of each code object looked up, so the object is loaded
hipError_t warm_fitch();
hipError_t warm_sankoff();
hipError_t warm_fitch_nt();
hipError_t warm_sankoff_nt();
hipError_t warm_replay();
hipError_t warm_synth();
hipError_t warm_sort();
hipError_t warm_scan();
hipError_t sort_records_to_host(pm_ctx* c, const std::vector<uint32_t>& counts, int64_t n, pm_mut* out);
// (Re)build the S2 / S3 leaf layout after the leaf columns or the tree changed (no-op when
// it is current or the tree has no S2 / S3 node).
int build_sub_planes(pm_ctx* c);
static_assert(sizeof(pm_mut) == 8, "pm_mut is {node, site_info}");
hipError_t launch_score(pm_ctx* c);
hipError_t launch_pack_codes(pm_ctx* c, const uint8_t* d_codes4, int64_t row_stride, const int32_t* d_row_of_leaf,
                             const uint8_t* d_present, int64_t present_stride);
hipError_t launch_expand_sparse(pm_ctx* c, const int64_t* d_row_off, const int32_t* d_site, const uint8_t* d_code,
                                uint8_t fill_code, int32_t rows, int64_t stride_words, uint32_t* d_out);
hipError_t launch_pack_sites(pm_ctx* c, const uint8_t* d_codes4, uint4* dst);
hipError_t launch_synth(pm_ctx* c, int64_t site_begin, uint64_t seed);
hipError_t launch_unpack_leaf_codes(pm_ctx* c, int64_t s0, int64_t ns, uint8_t* d_out);
hipError_t launch_sub_planes(pm_ctx* c);
hipError_t launch_unpack_sites(pm_ctx* c, const uint4* src, int64_t s0, int64_t ns, uint8_t* d_out);
void free_replay(pm_ctx* c);
void comm_release(pm_ctx* c);   // pm_rccl.hip
int leaves_install(pm_ctx* c, int64_t S, const uint8_t* d_codes4, int64_t row_stride, const int32_t* node_row);

// host plumbing (pm_hostio.cpp; the phase log, PhaseClock, host_threads and host_parallel_for:
// pm_plan.h)
// hipMalloc that, on failure, releases the context's cached text / rows buffers and retries
hipError_t malloc_or_release(pm_ctx* c, void** p, size_t bytes);
void release_cached(pm_ctx* c);
// malloc with transparent huge pages requested for large blocks (released with free / pm_free)
void* host_alloc_large(size_t n);
// dst (pageable host) <- src (device), n bytes, through pinned slots drained by host threads;
// synchronous on the ctx stream
hipError_t d2h_large(pm_ctx* c, void* dst, const void* src, size_t n);
// (device) src, n bytes, through the same slots, each landed chunk handed to `sink` in order
hipError_t d2h_stream(pm_ctx* c, const void* src, size_t n, const std::function<bool(const char*, size_t)>& sink,
                      bool& sink_ok);
bool write_all(int fd, const char* p, size_t n);   // write(2) until done; false on an error
// *buf grown (contents dropped) to hold `need` bytes
hipError_t grow_device(void** buf, size_t* cap, size_t need);
void free_hostio(pm_ctx* c);
// out[0 .. n) = exclusive scan of in[0 .. n) on the device, in == out: in place (pm_scan.hip)
hipError_t exclusive_scan(pm_ctx* c, const int64_t* in, int64_t* out, int64_t n);

// replay kernels (pm_replay.hip)
struct ReplayDev {
    int32_t leaves = 0;
    int64_t row_stride = 0;      // bytes per leaf row (multiple of 16)
    int64_t columns = 0;
    int32_t max_depth = 0;
    int32_t presence_words = 0;  // u32 words of block-presence bits per leaf
    char* rows = nullptr;        // [leaves][row_stride]
    const char* cons_row = nullptr;   // [row_stride]
    const int32_t* parent = nullptr;  // [N]
    const int32_t* leaf_node = nullptr;   // [leaves]
    const uint32_t* presence = nullptr;   // [leaves][presence_words]
    const int64_t* edit_off = nullptr;    // [N+1]
    const uint32_t* edit_col = nullptr;
    const uint8_t* edit_chr = nullptr;
    // blocks' column ranges [blk_lo, blk_hi) (id order = column order) and, per column tile,
    // the first block ending inside or after it: an absent block's columns are restored to
    // the consensus after the edits, so edits need no per-edit presence test
    int32_t blocks = 0;
    const int64_t* blk_lo = nullptr;
    const int64_t* blk_hi = nullptr;
    const int32_t* tile_blk = nullptr;   // [tiles + 1]
    // column tiles of kReplayTile bytes.  A node's edits are [plain | overriding] (an
    // overriding edit rewrites a column an ancestor edits), each part column-sorted; per
    // (node, tile) the first edit of each part in that tile
    int32_t tiles = 0;
    const int2* tile2 = nullptr;   // [N][tiles + 1] {plain, overriding}
    int32_t ring = 0;              // path nodes per leaf whose tile bounds a workgroup keeps in LDS
    int32_t tile_bytes = 0;        // column tile size of tile2 / tile_blk: kReplayTile or kDfsTile
    // k_replay_dfs: leaves in depth-first order (dfs_row = their rows), cut into groups
    // [g_leaf_off[g], g_leaf_off[g + 1]); a group's path nodes g_union[g_union_off[g] ..] in
    // order of first appearance; per leaf its path length and the prefix shared with the
    // previous leaf of its group (0 for a group's first)
    bool dfs = false;
    int32_t groups = 0;
    const int32_t* dfs_row = nullptr;
    const uint16_t* dfs_len = nullptr;
    const uint16_t* dfs_lpfx = nullptr;
    const int32_t* g_leaf_off = nullptr;
    const int32_t* g_union_off = nullptr;
    const int32_t* g_union = nullptr;
    const int64_t* path_off = nullptr;    // [leaves + 1] root-to-leaf node lists
    const int32_t* path = nullptr;
    // (leaf, tile) rows k_replay_dfs rebuilt from the consensus because an undo stack would
    // overflow, summed over the runs since replay_prepare (phase "replay.dfs_rebuilds")
    int32_t* dfs_rebuilds = nullptr;
};
#ifndef PM_REPLAY_TILE
#define PM_REPLAY_TILE 16384
#endif
constexpr int64_t kReplayTile = PM_REPLAY_TILE;   // leaf-row bytes assembled in LDS per workgroup
constexpr uint8_t kEditOverrides = 0x80;   // edit_chr flag: an ancestor edits the same column
constexpr int32_t kReplayRingMax = 512;     // ReplayDev::ring cap (deeper path nodes: bounds from HBM)
// k_replay_dfs: column tile per wave, leaves and path nodes per leaf group
#ifndef PM_DFS_TILE
#define PM_DFS_TILE 4096
#endif
constexpr int64_t kDfsTile = PM_DFS_TILE;
#ifndef PM_DFS_LEAVES
#define PM_DFS_LEAVES 16
#endif
constexpr int32_t kDfsLeaves = PM_DFS_LEAVES;
#ifndef PM_DFS_UNION
#define PM_DFS_UNION 128
#endif
constexpr int32_t kDfsUnionCap = PM_DFS_UNION;

// FASTA formatting on the device (printSequenceLinesNew, src/fasta.cpp:155-254): one
// segment per (leaf, print position) -- a block read forward or reverse-complemented from
// the leaf's row, or a run of dashes for an absent block (aligned output).
struct FmtSeg {
    int64_t src;     // first row column of the block, -1 for a dash run
    int64_t width;   // columns of the block, or the dash count
    int32_t rev;     // reverse strand: read backwards, complemented
    int32_t pad;
};
struct FmtArgs {
    const char* rows;
    int64_t row_stride;
    int32_t positions;        // print positions per leaf
    bool aligned;
    const FmtSeg* seg;        // [leaves][positions]
    int64_t* seg_len;         // [leaves][positions] chars each segment prints
    const int64_t* seg_off;   // [leaves][positions] offset in the leaf's line
    const int64_t* line_len;  // [leaves]
    const int64_t* start;     // [leaves] rotation of the line (circular offset)
    const int64_t* text_off;  // [leaves] byte offset of the leaf's record
    const int64_t* name_off;  // [leaves + 1] into names
    const char* names;
    char* text;
};
hipError_t launch_fmt_count(pm_ctx* c, const FmtArgs& f, int32_t leaves);
hipError_t launch_fmt_write(pm_ctx* c, const FmtArgs& f, int32_t leaves);
hipError_t launch_replay(pm_ctx* c, const ReplayDev& d);

// VCF extraction (pm_vcf.hip; printVCFParallel, src/vcf.cpp:177-382) over the aligned FASTA text
// of format_device: column i of a leaf's row is text[row_base[leaf] + i + i / 70].
struct VcfRec {
    int32_t leaf, pos;     // the tip (replay leaf index) and POS
    int64_t off;           // REF at pool[off .. off + rlen), ALT behind it
    int32_t rlen, alen;
};
struct VcfArgs {
    const char* text;
    const int64_t* row_base;   // [leaves]
    const uint8_t* live;       // [leaves] 1: compared (not the reference, same row length)
    int32_t leaves;
    int32_t ref_leaf;
    int64_t n;                 // columns of the reference row
    int64_t words;             // 64-column words per leaf
    char* ref;                 // [n] the reference row without line breaks
    int32_t* coord;            // [n] POS of a column: 1 + reference bases before it
    uint64_t* skip;            // [leaves][words] both rows '-' (and the columns past n)
    uint64_t* equal;           // [leaves][words] the same base in both rows
    int64_t* nstart;           // [leaves + 1] events per leaf, then their exclusive scan
    int64_t* chain;            // [leaves] first column whose equal base anchors (n: none)
    int64_t events;
    int32_t* ev_leaf;          // [events]
    int32_t* ev_col;           // [events] first column of the event
    int64_t* ev_recs;          // [events + 1] 1: the event yields a record; then the scan
    int64_t* ev_bytes;         // [events + 1] its REF + ALT bytes; then the scan
    VcfRec* recs;
    char* pool;
};
hipError_t launch_vcf_classify(pm_ctx* c, const VcfArgs& a);            // ref, coord, planes, nstart, chain
hipError_t launch_vcf_list(pm_ctx* c, const VcfArgs& a);                // ev_leaf / ev_col from the scanned nstart
hipError_t launch_vcf_emit(pm_ctx* c, const VcfArgs& a, bool write);    // count, or records + pool
// Genotype text of a batch of lines: cells (line in batch, sample, ALT index), per line the
// host's prefix; line lengths, offsets and text on the device.
struct VcfTextArgs {
    int32_t lines, samples;
    int64_t cells;
    const int32_t* cell;        // [cells][3]
    uint32_t* gt;               // [lines][samples]
    const int64_t* prefix_off;  // [lines + 1] into prefix
    const char* prefix;
    int64_t* line_off;          // [lines + 1] lengths, then their exclusive scan
    char* text;
};
hipError_t launch_vcf_text_count(pm_ctx* c, const VcfTextArgs& t);
hipError_t launch_vcf_text_write(pm_ctx* c, const VcfTextArgs& t);
hipError_t warm_vcf();
// MAF extraction (pm_maf.hip; Tree::printMAF, src/maf.cpp:68-188) over the replayed rows:
// row(t, b) = rows[t][blk_lo[b] .. blk_hi[b]).  Lines are addressed as entries
// rank * tips + tip, rank = the block's place in the printed (group, block-list) order.
constexpr int32_t kMafChunk = 4096;      // body bytes per workgroup of k_maf_write
// workgroups per line of a block `width` columns wide (a line without a body still has its prefix)
__host__ __device__ inline int32_t maf_chunks(int64_t width) {
    return width > kMafChunk ? (int32_t)((width + kMafChunk - 1) / kMafChunk) : 1;
}
constexpr int32_t kMafHeld = 1, kMafForward = 2;      // MafArgs::held bits
constexpr int32_t kMafOpens = 1, kMafCloses = 2;      // MafArgs::rank_fold bits
struct MafArgs {
    const char* rows;
    int64_t row_stride;
    int32_t tips, blocks;          // blocks: ids 0..max_id
    const int64_t* blk_lo;         // [blocks]
    const int64_t* blk_hi;
    const uint8_t* held;           // [tips][blocks] kMafHeld | kMafForward
    const int32_t* order;          // [tips][blocks] block ids in the tip's print order
    const int32_t* circular;       // [tips] circular offset, < 0: none
    int32_t* size;                 // [tips][blocks] ungapped characters (0 when not held)
    int32_t* start;                // [tips][blocks]
    int32_t* src_size;             // [tips]
    int32_t ranks;
    const int32_t* rank_blk;       // [ranks] block id
    const uint8_t* rank_fold;      // [ranks] kMafOpens: "a\n" before its first entry; kMafCloses: "\n" after its last
    const int64_t* name_off;       // [tips + 1] into names
    const char* names;
    int64_t* line_len;             // [ranks * tips] bytes of each entry, folds included
};
// size[t][b] for the blocks cls_blk[0 .. n) of one width class: G lanes per (tip, block) item
// (G = 4: at most kMafNarrow4 columns, 16: at most kMafNarrow16, 64: any width)
constexpr int64_t kMafNarrow4 = 49, kMafNarrow16 = 241;
hipError_t launch_maf_size(pm_ctx* c, const MafArgs& a, const int32_t* cls_blk, int32_t n, int lanes);
hipError_t launch_maf_start(pm_ctx* c, const MafArgs& a);
hipError_t launch_maf_line_len(pm_ctx* c, const MafArgs& a);
// The text of the entries [e0, e1) at text + line_off[e - e0]; wg_off[k] = first workgroup of
// rank rank0 + k's entries inside the batch (its tips x its chunks), wg_off[nr] = the grid.
struct MafBatch {
    int64_t e0, e1;
    int32_t rank0, nr;
    const int32_t* wg_off;         // [nr + 1]
    const int64_t* line_off;       // [e1 - e0]
    char* text;
};
hipError_t launch_maf_write(pm_ctx* c, const MafArgs& a, const MafBatch& b, int32_t workgroups);
hipError_t warm_maf();
// GFA extraction (pm_gfa.hip; Tree::convertToGFA, src/gfa.cpp:3-500) over the replayed rows.
// A tip's walk is cut into items (tip, block, chunk): item = tip * chunks + chunk_off[block] + c,
// which is the schedule order (tips in order, blocks ascending, chunks in walk order).  An item
// of a held block whose columns are not all '-' / 'x' is a path step.
constexpr int32_t kGfaNode = 32;   // columns per chunk (node_len, gfa.cpp:120)
__host__ __device__ inline int32_t gfa_chunks(int64_t width) { return (int32_t)((width + kGfaNode - 1) / kGfaNode); }
constexpr uint32_t kGfaReverseStart = 0x80000000u;   // start code: a reverse-strand start tuple
struct GfaArgs {
    const char* rows;
    int64_t row_stride;
    int32_t tips, blocks;          // blocks: ids 0..max_id
    const int64_t* blk_lo;         // [blocks]
    const int64_t* blk_hi;
    const uint8_t* held;           // [tips][blocks] kMafHeld | kMafForward
    int32_t chunks;                // chunks of all blocks together (items per tip)
    const int32_t* chunk_off;      // [blocks + 1] first chunk of a block
    const int32_t* chunk_blk;      // [chunks] the block of a chunk
    const uint32_t* start_code;    // [2][chunks] forward, reverse: separates the start tuples
    int64_t items;                 // tips * chunks
    uint64_t* key;                 // [3][items] (start code << 32 | length), string bits 127..64, 63..0
    int64_t* flag;                 // [items] 1: a step
};
hipError_t launch_gfa_chunk(pm_ctx* c, const GfaArgs& a);
// The steps: items with a set flag, numbered by `scan` (the exclusive scan of the flags).
struct GfaSteps {
    int64_t steps;
    uint64_t* key;                 // [3][steps]
    int32_t* tip;                  // [steps]
    uint8_t* forward;              // [steps] the path strand
    int32_t* tip_off;              // [tips + 1] first step of a tip
    int32_t* id;                   // [steps] node id: the rank of the node's first step
};
hipError_t launch_gfa_compact(pm_ctx* c, const GfaArgs& a, const int64_t* scan, const GfaSteps& s);
// perm <- the steps sorted by the whole key, stable (equal keys stay in step order); scratch
// holds 4 x steps 64-bit words
hipError_t gfa_sort(pm_ctx* c, const GfaSteps& s, uint32_t* perm, uint64_t* scratch);
// head[i] = 1 where the key at perm[i] differs from its left neighbour's; creator[perm[i]] = 1 there
hipError_t launch_gfa_heads(pm_ctx* c, const GfaSteps& s, const uint32_t* perm, int64_t* head, int64_t* creator);
// run_first[r] = first (earliest) step of the r-th run; hscan / cscan: scans of head / creator
hipError_t launch_gfa_runs(pm_ctx* c, const GfaSteps& s, const uint32_t* perm, const int64_t* head, const int64_t* hscan,
                           int32_t* run_first);
// id[step] = cscan[its run's first step]; per node its key (length, string) and creator strand
struct GfaNodes {
    uint64_t* key;                 // [3][nodes]
    uint8_t* forward;              // [nodes]
    int64_t nodes;
};
hipError_t launch_gfa_ids(pm_ctx* c, const GfaSteps& s, const uint32_t* perm, const int64_t* head, const int64_t* hscan,
                          const int32_t* run_first, const int64_t* cscan, const GfaNodes& n);
// "P" lines: printed[2 * id + forward] is the step's printed id, -1 when the step is dropped.
struct GfaText {
    int64_t steps;
    int32_t tips;
    const int32_t* id;             // [steps]
    const uint8_t* forward;        // [steps]
    const int32_t* tip;            // [steps]
    const int32_t* tip_off;        // [tips + 1]
    const int32_t* printed;
    int64_t* step_len;             // [steps + 1] bytes of a step with its comma (0: dropped; [steps] = 0)
    const int64_t* step_off;       // [steps + 1] their exclusive scan
    const int64_t* name_off;       // [tips + 1] into names
    const char* names;
    int64_t* line_len;             // [tips]
};
hipError_t launch_gfa_step_len(pm_ctx* c, const GfaText& t);
hipError_t launch_gfa_line_len(pm_ctx* c, const GfaText& t);
// the lines of tips [t0, t1) at text + line_off[t - t0]; batch_steps = tip_off[t1] - tip_off[t0]
hipError_t launch_gfa_write(pm_ctx* c, const GfaText& t, int32_t t0, int32_t t1, const int64_t* line_off, char* text,
                            int64_t batch_steps);
hipError_t warm_gfa();
// Subnetwork extraction (pm_subnet.hip; consolidateNucMutations, src/panman.cpp:2233-2322) over the
// mutation records of the merged chains of one batch, in chain order (top first, list order within
// a node).  A coordinate's rank in (primary, position, gap position) tuple order is
// block_base[primary] + pos_base[pos_off[primary] + position] + gap position + 1.
constexpr int32_t kSubnetBadBlock = 1, kSubnetBadPos = 2, kSubnetBadGap = 3, kSubnetUnstable = 4;   // SubnetArgs::error
struct SubnetArgs {
    int64_t records;
    const int32_t* rec_node;       // [records] new node id
    const int32_t* rec_primary;
    const int32_t* rec_pos;
    const int32_t* rec_gap;        // -1: main position
    const uint8_t* rec_info;       // (length << 4) | type
    const uint32_t* rec_nucs;
    int32_t blocks;                // block ids 0 .. blocks - 1
    const int32_t* blk_len;        // [blocks] main positions 0 .. len (the sentinel included); -1: no such block
    const uint32_t* block_base;    // [blocks]
    const int64_t* pos_off;        // [blocks] into pos_base
    const uint32_t* pos_base;      // per block len + 2 entries: prefix of 1 + gap length at the position
    int64_t* rec_off;              // [records + 1] bases per record, then their exclusive scan
    int32_t* error;                // [1] the largest kSubnet* code met, 0: none
};
// One expanded base: key = new node << 32 | rank; val = entry number << 8 | SNP type << 4 | code.
struct SubnetEntries {
    int64_t n;
    uint64_t* key;                 // [n]
    uint64_t* val;                 // [n]
    int32_t* blk;                  // [n] the coordinate, by entry number
    int32_t* pos;
    int32_t* gap;
};
hipError_t launch_subnet_count(pm_ctx* c, const SubnetArgs& a);
hipError_t launch_subnet_expand(pm_ctx* c, const SubnetArgs& a, const SubnetEntries& e);
// key / val sorted by key over bits [0, end_bit), stable: equal keys stay in entry order.  key_alt / val_alt: the
// second halves of the double buffers; *key_out / *val_out: where the sorted arrays ended up.
hipError_t subnet_sort(pm_ctx* c, const SubnetEntries& e, uint64_t* key_alt, uint64_t* val_alt, int end_bit, uint64_t** key_out,
                       uint64_t** val_out);
// alive[i] = 1 and tc[i] = type << 4 | code at the first entry of every key whose fold survives (alive: n + 1
// entries, the last 0); launch_subnet_compact takes its exclusive scan
hipError_t launch_subnet_fold(pm_ctx* c, const uint64_t* key, const uint64_t* val, int64_t n, int64_t* alive, uint8_t* tc,
                              int32_t* error);
// The survivors in sorted order (launch_subnet_compact).
struct SubnetLive {
    int64_t m;
    int32_t* node;                 // [m]
    int32_t* blk;
    int32_t* pos;
    int32_t* gap;
    uint8_t* tc;                   // type << 4 | code
    int64_t* head;                 // [m] own index at the head of a maximal run, else 0; then the nearest head
    int64_t* start;                // [m + 1] 1: a record starts here; then the exclusive scan
};
hipError_t launch_subnet_compact(pm_ctx* c, const uint64_t* key, const uint64_t* val, int64_t n, const int64_t* ascan,
                                 const uint8_t* tc, const SubnetEntries& e, const SubnetLive& s);
hipError_t subnet_runs(pm_ctx* c, const SubnetLive& s);     // head (scanned) and start (flags)
struct SubnetOut {
    int32_t* primary;              // [records out]
    int32_t* pos;
    int32_t* gap;
    uint8_t* info;
    uint32_t* nucs;
    int32_t* node_count;           // [new nodes] records per new node (zeroed by the caller)
};
hipError_t launch_subnet_pack(pm_ctx* c, const SubnetLive& s, const SubnetOut& o);
hipError_t warm_subnet();
// The rank tables of SubnetArgs, indexed by primary block id (as the replay's block tables are), and the text
// of a kSubnet* code (pm_subnet.cpp; pm_impute sorts the same coordinates).
struct RankTables {
    std::vector<int32_t> blk_len;
    std::vector<uint32_t> block_base, pos_base;
    std::vector<int64_t> pos_off;
};
int rank_tables(pm_ctx* c, const pm_panmat* p, RankTables& t);
const char* coordinate_error(int32_t code);
// N imputation (pm_impute.hip; Tree::imputeNs, src/impute.cpp) over nucleotide records in list order.
struct ImputeRecs {
    int64_t n;
    const int32_t* node;           // [n] the record's node (launch_impute_steps' source: unread)
    const int32_t* primary;
    const int32_t* pos;
    const int32_t* gap;            // -1: main position
    const uint8_t* info;           // (length << 4) | type
    const uint32_t* nucs;
};
struct ImputeRecsOut {
    int32_t* node;                 // nullable
    int32_t* primary;
    int32_t* pos;
    int32_t* gap;
    uint8_t* info;
    uint32_t* nucs;
};
// imputeSubstitution (src/impute.cpp:205-225) per record: off[r] = the records that take its place -- 0 for an
// NSNPS of N, the non-N bases of an NS holding an N, else 1 -- (off: n + 1 entries, the last 0; launch_impute_pack
// takes the exclusive scan) and *imputed += the bases dropped.  Records [keep0, keep1) are kept as they are.
hipError_t launch_impute_count(pm_ctx* c, const ImputeRecs& in, int64_t keep0, int64_t keep1, int64_t* off,
                               unsigned long long* imputed);
hipError_t launch_impute_pack(pm_ctx* c, const ImputeRecs& in, int64_t keep0, int64_t keep1, const int64_t* off, const ImputeRecsOut& out);
// originalNucs (src/impute.cpp:161): orig[r] = the codes under the record's bases in its node's parent's replayed
// row, packed as nucs are (0 for the root's records, par_row -1).  *error is set when a cell does not exist.
struct ImputeRows {
    const char* rows;
    int64_t row_stride, columns;
    int32_t blocks;                // ids 0..max_id
    const int64_t* pos_off;        // [blocks + 1] into main_col / gap_col (a block's positions 0..n_b)
    const int32_t* main_col;
    const int32_t* gap_col;
    const int32_t* par_row;        // [nodes] the replayed row of the node's parent; -1: the root
    int32_t* error;
};
hipError_t launch_impute_originals(pm_ctx* c, const ImputeRecs& in, const ImputeRows& rows, uint32_t* orig);
// The lists of a batch's path steps back to back: step s is records [src0[s], src0[s] + dst_off[s + 1] - dst_off[s])
// of `src`, written at dst_off[s] with node = pair[s]; an inverted step's records as MutationList::invertMutations
// (src/panman.cpp:2374-2420) leaves them, the originals from `orig`.
struct ImputeSteps {
    int64_t steps, records;        // records = dst_off[steps]
    const int64_t* dst_off;        // [steps + 1]
    const int64_t* src0;           // [steps]
    const uint8_t* inverted;       // [steps]
    const int32_t* pair;           // [steps] the batch's pair index
};
hipError_t launch_impute_steps(pm_ctx* c, const ImputeSteps& s, const ImputeRecs& src, const uint32_t* orig, const ImputeRecsOut& dst);
// sum[pair] += the pair's survivors that are not a substitution with code N (sum zeroed by the caller)
hipError_t launch_impute_pair_sum(pm_ctx* c, const SubnetLive& live, unsigned long long* sum);
// *error |= 1 when two neighbours of the sorted keys are equal: a cell written twice in one list
hipError_t launch_impute_twice(pm_ctx* c, const uint64_t* key, int64_t n, int32_t* error);
hipError_t warm_impute();
// Amino-acid translation (pm_aa.hip; Tree::extractAminoAcidTranslations, src/aaTrans.cpp:185-304)
// over the replayed rows of every node: node v's row is rows[row_of[v]].  A cell of the canonical
// row is a column; col_main / col_first give the column of its position's main character and of the
// position's first gap slot, so its slot index is column - col_first (-1 at col_main).
constexpr int32_t kAaChunk = 256;        // window cells per round of k_aa_codons' workgroup
struct AaSpan {
    int32_t cs, ce;                // the columns of locate(start) and locate(end); -1: not found
    int32_t b0, b1;                // their blocks
};
struct AaArgs {
    const char* rows;
    int64_t row_stride;
    int32_t nodes, blocks;         // blocks: ids 0..max_id
    const int32_t* row_of;         // [nodes]
    const int64_t* blk_lo;         // [blocks]
    const int64_t* blk_hi;
    const uint8_t* held;           // [rows][blocks] kMafHeld | kMafForward
    const int32_t* size;           // [rows][blocks] characters that are neither '-' nor 'x' (0 when not held)
    const int32_t* col_main;       // [columns]
    const int32_t* col_first;      // [columns]
    const int32_t* rev_top;        // [blocks] the main column of position n_0 in the block; -1: none
    int64_t start, end;            // the global coordinates
    AaSpan* span;                  // [nodes]
};
hipError_t launch_aa_locate(pm_ctx* c, const AaArgs& a);
// The codon tables of nodes node[0 .. n): slot s holds bases (2-bit codes in TCAG order, one
// byte each) at base + s * base_cap and the codons' window indices at cstart / cend + s * codon_cap.
struct AaTables {
    int32_t n;
    const int32_t* node;           // [n]
    int32_t base_cap, codon_cap;
    uint8_t* base;
    int32_t* cstart;
    int32_t* cend;
    int32_t* codons;               // [n] complete codons; 0 when the window is "ERROR"
    uint8_t* error;                // [n] 1: the walk met no stop
};
hipError_t launch_aa_codons(pm_ctx* c, const AaArgs& a, const AaTables& t);
// The lines of a batch against the root's tables (slot 0 of `root`).
struct AaText {
    const int64_t* name_off;       // [nodes + 1] into names
    const char* names;
    int64_t* line_len;             // [n] bytes of the slot's line; 0: no line
    int32_t* sec;                  // [n][2] bytes of the line's S and I entries
    const int64_t* line_off;       // [n] exclusive scan of line_len
    char* text;
};
hipError_t launch_aa_line_len(pm_ctx* c, const AaArgs& a, const AaTables& root, const AaTables& t, const AaText& x);
hipError_t launch_aa_write(pm_ctx* c, const AaArgs& a, const AaTables& root, const AaTables& t, const AaText& x);
hipError_t warm_aa();
// Mutation printing (pm_mutations.hip; Tree::printMutationsNew, src/panman.cpp:3699-4057) over the
// replayed rows of every node.  A cell (block, position, slot) of the reference's maps is a column
// of the canonical row: main_col[pos_off[block] + position], or gap_col[..] + slot.
constexpr int32_t kMutChunk = 256;       // columns per workgroup of the root map's two passes
constexpr int32_t kMutRound = 256;       // entries per round of k_mut_write's workgroup
constexpr uint8_t kMutGap = 1, kMutOdd = 2;   // MutEntry::flags
struct MutEntry {                  // one element of a nucleotide mutation
    int32_t coord1;                // the root coordinate it prints (coord + 1)
    uint8_t kind;                  // 0: no entry; 1, 2, 3: line S, I, D
    char old_ch, new_ch;
    uint8_t flags;                 // kMutGap: "g"; kMutOdd: a kept NSNPS over no base
};
static_assert(sizeof(MutEntry) == 8, "MutEntry is 8 bytes");
struct MutArgs {
    const char* rows;
    int64_t row_stride, columns;
    int32_t nodes, blocks, root;   // blocks: ids 0..max_id
    const int32_t* row_of;         // [nodes]
    const int32_t* parent;         // [nodes]
    const uint8_t* held;           // [nodes][blocks] kMafHeld | kMafForward, as getSequenceFromReference leaves them
    const int64_t* blk_lo;         // [blocks]
    const int64_t* blk_hi;
    const int64_t* pos_off;        // [blocks + 1] into main_col / gap_col (a block's positions 0..n_b)
    const int32_t* main_col;
    const int32_t* gap_col;
    // the root map: real characters of the root's held blocks
    const uint8_t* col_held;       // [columns] 1: the root holds the column's block
    int64_t* chunk;                // [chunks of kMutChunk columns] their real characters; then the exclusive scan
    int32_t* before;               // [columns + 1] the real characters before the column
    // the tree's nucleotide mutations in list order
    const int32_t* mut_node;
    const int32_t* mut_primary;
    const int32_t* mut_position;
    const int32_t* mut_gap;
    const uint8_t* mut_info;
    const uint32_t* mut_nucs;
    unsigned long long* odd;       // [1] kept NSNPS entries whose old character is no base
    int32_t* error;                // [1] set when a mutation's cell does not exist
};
hipError_t launch_mut_root_map(pm_ctx* c, const MutArgs& a);
// One batch: the mutations [m0, m0 + m) of nodes [v0, v0 + n).
struct MutBatch {
    int64_t m0, m, entries;
    int32_t v0, n;
    const int64_t* node_mut;       // [nodes + 1] the PanMAT's nuc_mut_offsets
    int64_t* elems;                // [m + 1] elements per mutation (the last 0); then the exclusive scan
    MutEntry* entry;               // [entries]
    const int64_t* name_off;       // [nodes + 1] into names
    const char* names;
    int64_t* line_len;             // [3 n + 1] bytes of node s's line k at 3 s + k (the last 0); then the scan
    char* text;
};
hipError_t launch_mut_count(pm_ctx* c, const MutArgs& a, const MutBatch& b);
hipError_t launch_mut_classify(pm_ctx* c, const MutArgs& a, const MutBatch& b);
hipError_t launch_mut_line_len(pm_ctx* c, const MutArgs& a, const MutBatch& b);
hipError_t launch_mut_write(pm_ctx* c, const MutArgs& a, const MutBatch& b);
hipError_t warm_mutations();
// UShER MAT export (pm_usher.hip; panmanToUsher, src/panman2usher.cpp:564-604) over the replayed rows
// of every node, every block held forward at every node.  Nodes are addressed by pre-order rank; the
// tree's nucleotide mutations are in rank order, list order within a node.
constexpr int32_t kUsherRound = 256;     // entries per round of k_usher_write's workgroup
constexpr int32_t kUsherMutBytes = 18;   // the most bytes of a wrapped `mut`: 0a len 08 p(5) 10 r 18 p 22 n b(4)
struct UsherEntry {                // one element of a nucleotide mutation: one Parsimony::mut
    int32_t position;              // 1 + the cells before it
    uint8_t ref, par;              // 4-bit codes, 0 for '-' and 'x'
    uint8_t set;                   // bit k: mut_nuc holds k (15 for a deletion and for code 0)
    uint8_t after;                 // the code of the running character the element leaves (0: '-')
};
static_assert(sizeof(UsherEntry) == 8, "UsherEntry is 8 bytes");
struct UsherArgs {
    const char* rows;
    int64_t row_stride, columns;
    const char* pseudo;            // [columns] the pseudo-root row: consensus, '-' in gap slots, 'x' at sentinels
    int32_t blocks;                // ids 0..max_id
    const int64_t* pos_off;        // [blocks + 1] into main_col / gap_col (a block's positions 0..n_b)
    const int32_t* main_col;
    const int32_t* gap_col;
    const int64_t* blk_lo;         // [blocks] the block's first column
    const int64_t* cell_base;      // [blocks] the cells of the blocks of smaller id
    const int32_t* par_row;        // [ranks] the replayed row of the rank's parent; -1 (the root): the pseudo-root row
    const int64_t* rank_mut;       // [ranks + 1] the mutations of a rank
    const int32_t* mut_rank;       // [mutations]
    const int32_t* mut_primary;
    const int32_t* mut_position;
    const int32_t* mut_gap;
    const uint8_t* mut_info;
    const uint32_t* mut_nucs;
    int32_t* error;                // [1] set when a mutation's cell does not exist
};
// One batch: the mutations [m0, m0 + m) of ranks [r0, r0 + n).
struct UsherBatch {
    int64_t m0, m, entries;
    int32_t r0, n;
    int64_t* elems;                // [m + 1] elements per mutation (the last 0); then the exclusive scan
    UsherEntry* entry;             // [entries]
    uint64_t* key;                 // [entries] (rank - r0) << 32 | column, and its double buffer
    uint64_t* key_alt;
    uint32_t* val;                 // [entries] the element's index, and its double buffer
    uint32_t* val_alt;
    uint32_t* list_len;            // [n] L: the bytes of the node's wrapped muts
    int64_t* node_off;             // [n + 1] 1 + varint_len(L) + L (the last 0); then the scan
    char* out;
};
hipError_t launch_usher_count(pm_ctx* c, const UsherArgs& a, const UsherBatch& b);
hipError_t launch_usher_classify(pm_ctx* c, const UsherArgs& a, const UsherBatch& b);
// An element whose cell an earlier element of its node's list wrote takes that element's `after`
// as `par`: a stable sort of (key, val) and one look at the sorted predecessor.
hipError_t usher_earlier_writers(pm_ctx* c, const UsherBatch& b);
hipError_t launch_usher_sizes(pm_ctx* c, const UsherArgs& a, const UsherBatch& b);
hipError_t launch_usher_write(pm_ctx* c, const UsherArgs& a, const UsherBatch& b);
hipError_t warm_usher();
// rows[leaf][c0 .. c0+n) chars -> packed codes out[leaf][(n+1)/2] ('-', 'x' -> 0)
hipError_t launch_rows_to_codes(pm_ctx* c, const char* rows, int64_t row_stride, int32_t leaves, int64_t c0,
                                int64_t n, uint8_t* out, int64_t out_stride);

}  // namespace pm
