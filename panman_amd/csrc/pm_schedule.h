// pm_schedule.h -- the launch sequence of one pm_run as data (pm_schedule.cpp): which kernels
// launch_fitch / launch_sankoff issue, over which items, on which stream, inside which timer
// span.  Over pm_plan.h alone, no HIP header: the decisions build and run without a GPU
// (tests/test_schedule_host.py).  DESIGN.md, "Shared plumbing of the run launchers".
#pragma once

#include "pm_plan.h"

namespace pm {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;

// The constants the decisions read; the kernels include the same definitions.
#ifndef PM_CX_COMPACT   // compact complex lanes of the Fitch records (pm_kernels.h cx_store); 0 = the 16-plane format
#define PM_CX_COMPACT 0
#endif
constexpr bool kCxCompact = PM_CX_COMPACT != 0;
#ifndef PM_MIXED_MAX_WAVES   // a level of both out-degree kinds is one mixed launch up to this many narrow waves
#define PM_MIXED_MAX_WAVES 4096
#endif
constexpr int64_t kMixedMaxWaves = PM_MIXED_MAX_WAVES;
// a plain post-order prefix (PM_OPT_PLAIN_UP) gets its own launch from this many (node, tile) waves: the lean
// kernel's occupancy pays on levels that fill the chip many times over (C3 with a split at every level: +0.2 ms)
#ifndef PM_PLAIN_MIN_WAVES
#define PM_PLAIN_MIN_WAVES 65536
#endif
constexpr int64_t kPlainMinWaves = PM_PLAIN_MIN_WAVES;
#ifndef PM_GROUP_LEVELS   // most pre-order levels in one launch (DownArgs::split / dense_g)
#define PM_GROUP_LEVELS 4
#endif
constexpr int kGroupLevels = PM_GROUP_LEVELS;
#ifndef PM_DOWN_PACK   // PM_OPT_DOWN_PACK: items per wave of a packed level ...
#define PM_DOWN_PACK 8
#endif
constexpr int kDownPack = PM_DOWN_PACK;
#ifndef PM_DOWN_PACK_MIN_WAVES   // ... and the (item, tile) waves from which a level is packed
#define PM_DOWN_PACK_MIN_WAVES 65536
#endif
constexpr int64_t kDownPackMinWaves = PM_DOWN_PACK_MIN_WAVES;
#ifndef PM_TAIL_PACK   // PM_OPT_TAIL_PACK: S2 / S3 items per wave of the packed tail ...
#define PM_TAIL_PACK 8
#endif
constexpr int kTailPack = PM_TAIL_PACK;
#ifndef PM_TAIL_PACK_MIN_WAVES   // ... and its threshold in (S item, tile) waves
#define PM_TAIL_PACK_MIN_WAVES 65536
#endif
constexpr int64_t kTailPackMinWaves = PM_TAIL_PACK_MIN_WAVES;

// Grids of the level launches: one wave, or one workgroup, per (item, tile); count * tiles stays far below 2^31.
#ifndef PM_TILE_FAST   // (pm_kernels.h wave_item)
#define PM_TILE_FAST 1
#endif
inline uint32_t wave_grid_x(int32_t count, int32_t tiles) {
    return (uint32_t)(((int64_t)count * (PM_TILE_FAST ? tiles : 1) + kWavesPerBlock - 1) / kWavesPerBlock);
}
inline uint32_t block_grid_x(int32_t count, int32_t tiles) { return (uint32_t)((int64_t)count * (PM_TILE_FAST ? tiles : 1)); }

// Everything outside the tree that the launch sequence depends on: the options, under pm_ctx's names, and the
// run's facts.  Hashed as bytes (graph_key_of).
struct RunOpts {
    int64_t virtual_leaf_parents = 0, subtree_form = 0, narrow_max = 0, group_waves = 0, group_levels = 0, up_group = 0,
            sub_down = 0, tail_pack = 0, tail_pack_min_waves = 0, down_pack = 0, down_pack_min_waves = 0, plain_up = 0,
            plain_min_waves = 0, cluster = 0, nt_loads = 0, leaves_all_present = 0, has_forced = 0, tiles = 0;
};
static_assert(sizeof(RunOpts) == 18 * sizeof(int64_t), "RunOpts is hashed as bytes: no padding");

// The paths a run takes, each predicate under one name (the rules: run_paths, and DESIGN.md).
struct RunPaths {
    bool sankoff, block;
    bool ap;         // every leaf present at every site
    bool virt, sub;  // leaf-parents evaluated inline; ... and S2 / S3 subtrees (the subtree form)
    bool planned;    // sub, PM_OPT_CLUSTER on and the tree has a sweep plan
    bool clu, cld;   // post-order / pre-order sweeps
    bool grp;        // grouped post-order launches
    bool sub_down;   // Fitch: S2 / S3 children in their parent's pre-order descriptor
    bool nt;         // the non-temporal build of the passes
    int form;        // 0 plain, 1 leaf-parent, 2 subtree form (HostTree::lvl_down)
    int up_form;     // ... 3 its Fitch groups, 4 its Sankoff groups (HostTree::lvl_up)
};
RunPaths run_paths(const HostTree& ht, const RunOpts& o, int mode);

// The host tables of the chosen form, picked once (null: the form has none).
struct RunForm {
    const std::vector<int32_t>*up_level_off, *up_class_off, *down_level_off, *part_off, *up_degree, *up_plain, *dense_base_k;
    const std::vector<uint8_t>*up_leafy, *up_recomp;
    int32_t num_tail;
    bool dense;      // a pre-order level is one range of dense indices, from dense_base(level)
    int32_t dense_base(int l) const { return !dense ? -1 : dense_base_k ? (*dense_base_k)[l] : (*down_level_off)[l]; }
};
RunForm run_form(const HostTree& ht, const RunPaths& p);

enum class StepKind : uint8_t {
    kFork, kJoin, kSpan,   // no launch: the side stream opens / closes; an empty timer span
    kUpBand, kUpMixed, kUpWide, kUpNarrow, kUpSweep, kUpParts, kUpMerge,
    kDownSweep, kDownBand, kDownLevel, kDownGroup, kDownPacked, kTail, kTailPacked,
    kCount
};
enum Narrow : uint8_t { kNarrowBase, kNarrowLeafy, kNarrowRecomp, kNarrowPlain };   // Step::variant of kUpNarrow

// One launch (or kFork / kJoin / kSpan), in issue order.
struct Step {
    StepKind kind = StepKind::kCount;
    // kUpNarrow: Narrow; kUpWide / kUpMixed: Sankoff's counter width 4 / 8; kUpMerge: 16 / 32; kDownBand: 1 = groups inside
    uint8_t variant = 0;
    bool side = false;       // on the side stream (between a kFork and its kJoin)
    // Timer spans (pm_kernel_times) are the launchers' own from before they shared a schedule.  Fitch: a level's
    // plain prefix and the rest of its narrow class share a span, which closes after the join; a forked wide
    // launch is untimed.  Sankoff: two spans, the join after them; side launches timed; parts and merge share a
    // span, and on a level it does not mix an empty span (kSpan) precedes them.
    bool timer_open = false, timer_close = false;
    uint8_t cls = 0;         // timer class: 0 post-order, 1 pre-order levels, 5 tail
    int32_t h0 = 0, h1 = 0;  // levels [h0, h1): heights (post-order) or depths (pre-order)
    // items [first, first + count) of the pass's order (kUpParts: parts; sweeps: clusters; bands: the levels)
    int32_t first = 0, count = 0;
    uint32_t grid_x = 0;
    int32_t count2 = 0;      // kUpMixed: the wide nodes behind the narrow ones; kTail: S2 / S3 items among them
    int32_t split[3] = {0, 0, 0}, dense_g[4] = {-1, -1, -1, -1}, dense_base = -1;   // DownArgs' (kDownGroup)
};

struct Schedule {
    RunPaths paths;
    std::vector<Step> steps;
    size_t first_down = 0;   // steps[first_down ..): the pre-order (the shard counters are cleared before it)
    // what launch_fitch logs and pm_design_bytes reads: down_pack_ranges = the levels PM_OPT_DOWN_PACK takes, or
    // switched off would take, as (first dense index, items) pairs
    int32_t packed_levels = 0;
    std::vector<int32_t> down_pack_ranges;
    bool tail_pack = false;
    int64_t tail_s_waves = 0;
};
// A pass over the level tables (no per-node work but the widest of a level's nodes above 255 children).
Schedule schedule_run(const HostTree& ht, const RunOpts& o, int mode);

}  // namespace pm
