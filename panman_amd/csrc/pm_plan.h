// pm_plan.h -- the host plan of a tree (pm_plan.cpp, pm_cluster.cpp): the constants and records
// the planner shares with the kernels, the host tables of a flattened tree (HostTree) and
// everything pm_tree_upload sends to the device (TreePlan).  No HIP header: the planner, the
// sweeps' schedule and the host plumbing they use (pm_hostpar.cpp) build and run without a GPU
// (tests/test_plan_host.py).
#pragma once

#include <chrono>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/panman_gpu.h"

namespace pm {

constexpr int kDegreeClasses = 4;
// Grouped post-order launches (PM_OPT_UP_GROUP): heights of at most this many nodes group.
#ifndef PM_UP_GROUP_NODES
#define PM_UP_GROUP_NODES 2048
#endif
constexpr int32_t kUpGroupNodes = PM_UP_GROUP_NODES;

// ... and a node recomputes same-launch descendants at most this many levels down (a node
// recomputing a child that itself recomputes one: depth 2; such a chain holds one child per level).
#ifndef PM_UP_GROUP_DEPTH
#define PM_UP_GROUP_DEPTH 2
#endif
constexpr int kUpGroupDepth = PM_UP_GROUP_DEPTH;
inline int degree_class(int32_t deg) { return deg <= 3 ? 0 : deg <= 15 ? 1 : deg <= 255 ? 2 : 3; }

// Level item of the Fitch / Sankoff passes: everything a wave needs to start its loads,
// in one 64-B scalar load (node, parent, child range, the first two children's encodings
// and, for virtual leaf-parent children, their leaves).
struct alignas(64) NodeDesc {
    int32_t node, parent, e0, e1;
    int32_t c0, c1, pad0, pad1;    // pad0: Sankoff up parts -- the first part; pre-order -- the grandparent, pad1 the great-grandparent (dense, -1)
    int32_t vl0[4], vl1[4];
};

// A leaf or virtual child beyond a node's first two (polytomies): its records need only
// the parent's final, so they are emitted by one flat launch after the pre-order levels
// instead of serially inside the parent's wave.
// Everything the tail wave needs is in the descriptor (one 64-B scalar load): no dependent
// id lookups (leaf_id[vl], internal_id[vinner]) between the descriptor and the records.
struct alignas(64) TailDesc {
    int32_t parent, enc, ix, iy;   // ix / iy: an S2 / S3 child's cherries (caller node ids), else -1
    int32_t vl[4];                 // a virtual child's leaves (ranks), -1 padded
    int32_t id[5];                 // caller node ids: the child itself, then its leaves vl[0..3]
    int32_t pad[3];
};

// Sankoff nodes of out-degree > 255: their children are cut into parts of kPartChildren,
// counted separately into 8-bit counters (16 codes x 8 planes + the finite plane).
constexpr int kPartChildren = 255;
constexpr int kPartPlanes = 16 * 8 + 1;
struct PartDesc {
    int32_t item;     // the node's position in its up-order descriptor array
    int32_t sub;      // children [e0 + sub * kPartChildren, ...)
    int32_t global;   // scratch slot
    int32_t pad;
};

// LDS-staged post-order sweeps (PM_OPT_CLUSTER, pm_cluster.cpp): LDS set slots per cluster wave
// (4 KiB each), most nodes per cluster, most heights per band
#ifndef PM_CL_SLOTS
#define PM_CL_SLOTS 4
#endif
constexpr int kClSlots = PM_CL_SLOTS;
#ifndef PM_CL_MAX_STEPS
#define PM_CL_MAX_STEPS 64
#endif
constexpr int32_t kClMaxSteps = PM_CL_MAX_STEPS;
#ifndef PM_CL_BAND
#define PM_CL_BAND 32
#endif
constexpr int32_t kClBandHeights = PM_CL_BAND;
// default PM_OPT_CLUSTER: the sweeps take the post-order from the first height whose level
// and every level above it hold at most this many materialised nodes (and above the last band
// whose clusters are bushy: more than kClChain nodes per level in its longest cluster)
#ifndef PM_CL_MAX_LEVEL
#define PM_CL_MAX_LEVEL (1 << 20)
#endif
#ifndef PM_CL_CHAIN
#define PM_CL_CHAIN 4
#endif
constexpr int32_t kClChain = PM_CL_CHAIN;
// ... or wide: more clusters than this (a level kernel's waves then fill the GPU as well, and
// its nodes run side by side where a cluster's run one after another).  C4 (T2) share
// 27.74 -> 26.88 ms (its bands below height 62 hold 25k-454k clusters), C3 unchanged (its
// widest band: 5.2k clusters); 4096 / 32768: 27.44 / 27.10 ms (r06mc, tools/gpu_r06mc.sh)
#ifndef PM_CL_MAX_CLUSTERS
#define PM_CL_MAX_CLUSTERS 16384
#endif
constexpr int32_t kClMaxClusters = PM_CL_MAX_CLUSTERS;
constexpr int32_t kClMaxLevel = PM_CL_MAX_LEVEL;
#ifndef PM_CL_FSLOTS
#define PM_CL_FSLOTS 8
#endif
constexpr int kClFSlots = PM_CL_FSLOTS;   // the pre-order sweeps' LDS final slots (1 KiB each)

struct ClusterPlan {
    int32_t h0 = 0;                  // first post-order level (subtree form) the sweeps take
    int32_t max_rounds = 0;          // steps of the longest cluster
    std::vector<NodeDesc> items;     // per cluster: its nodes in step order; parent = the node's
                                     // LDS slot, pad0 / pad1 its first two children's slots (-1:
                                     // not in the cluster)
    std::vector<int32_t> wg_off;     // [clusters + 1] item offsets
    std::vector<int32_t> band_wg;    // [bands + 1] cluster offsets
    std::vector<int32_t> band_level; // [bands + 1] first level of each band
    std::vector<int32_t> slot_of;    // [I] a node's slot (children beyond the first two), -1
    std::vector<int32_t> item_of;    // [I] a swept node's (first) item, -1
    int32_t n_items = 0;
    int32_t max_degree = 0;          // the items' largest out-degree (Sankoff sweeps: <= 255)
    int32_t upm_base = 0;            // the items' up slots follow both up orders' (UpArgs::upm)
    // the pre-order over the same clusters (plan_cluster_down; empty: the level kernels): per
    // cluster its nodes in depth-first pre-order; pad0 = the slot of the parent's final, pad1
    // = this node's (-1: none)
    std::vector<NodeDesc> down_items;
    bool down = false;
};

constexpr int32_t kVirtualBit = 1 << 30;
// Subtree form: a virtual child's shape in bits 28-29 of its encoding (0 = one or two leaves,
// 1 = S2 (cherry, leaf), 2 = S3 (cherry, cherry)); the dense index is the low 28 bits.
constexpr int kShapeShift = 28;
constexpr int32_t kDenseMask = (1 << kShapeShift) - 1;

struct HostTree {
    int32_t num_nodes = 0;
    int32_t root = -1;
    std::vector<int32_t> dense_of;        // [N] dense internal index or -(leaf rank + 1)
    std::vector<int32_t> internal_id;     // [I]
    std::vector<int32_t> leaf_id;         // [L]
    std::vector<int32_t> up_level_off;    // [H+1] offsets into up_order (level 0 = height 1)
    std::vector<int32_t> up_class_off;    // [4H+1] within a level, nodes by out-degree class
                                          // (<=3, <=15, <=255, more): Sankoff counter widths
    std::vector<int32_t> down_level_off;  // [D+1] offsets into down_order (level 0 = root)
    std::vector<int32_t> leaf_level_off;  // [D+1] offsets into leaf_down by depth
    std::vector<int32_t> child_off;       // dense CSR (host copy)
    std::vector<int32_t> child_enc;
    std::vector<int32_t> up_level_off_v;    // levels of up_order_v / down_order_v
    std::vector<int32_t> up_class_off_v;    // [4H+1] (level, degree class) buckets of up_order_v
    std::vector<uint8_t> up_leafy_v;        // [H] level's out-degree <= 3 nodes have leaf / virtual children only
    std::vector<int32_t> down_level_off_v;
    int64_t num_virtual = 0;
    bool down_dense_v = false;            // down_order_v[k] == k (dense order = pre-order levels)
    int32_t num_tail = 0, num_tail_v = 0;
    // Sankoff parts: prefix over the up-order descriptors ([I'+1]; nodes of out-degree <= 255
    // have none) of each form, and every descriptor's out-degree
    std::vector<int32_t> part_off, part_off_v, part_off_k, part_off_gs;
    std::vector<int32_t> up_degree[4];   // [0] plain, [1] leaf-parent form, [2] subtree form, [3] its Sankoff groups
    // subtree form: levels without the S2 / S3 nodes, each pre-order level's first dense index
    std::vector<int32_t> up_level_off_k, up_class_off_k, down_level_off_k, down_dense_base_k;
    std::vector<uint8_t> up_leafy_k;
    // subtree form, grouped post-order launches (PM_OPT_UP_GROUP): launch l's nodes by class
    std::vector<int32_t> up_level_off_g, up_class_off_g;
    std::vector<uint8_t> up_leafy_g, up_recomp_g;   // (recomp: some node of the launch recomputes a child)
    // ... and each launch's "plain" nodes at the front of its out-degree <= 3 class: binary, no
    // S2 / S3 child, no recomputed child -- the lean, higher-occupancy kernel (k_fitch_up<.., PLAIN>)
    std::vector<int32_t> up_plain_g, up_plain_gs;
    // ... and Sankoff's (a recomputed child must be binary)
    std::vector<int32_t> up_level_off_gs, up_class_off_gs;
    std::vector<uint8_t> up_leafy_gs, up_recomp_gs;
    bool down_dense_k = false;
    int32_t up_items_k = 0, up_items_g = 0, up_items_gs = 0;   // descriptor counts (up slot storage)
    int64_t num_sshape = 0;
    std::vector<uint8_t> sshape;          // [I] 1: S2, 2: S3 (subtree form), else 0
    int32_t num_tail_k = 0;
    int32_t num_tail_s = 0;               // subtree form: the first num_tail_s tail items are the S2 / S3 nodes
    int32_t sbase = -1;                   // ... dense indices sbase + item
    // offsets of the level tables in DevTree::lvl: [form] = plain, leaf-parent, subtree form,
    // (up only) its Fitch groups, its Sankoff groups
    int64_t lvl_up[5] = {0, 0, 0, 0, 0}, lvl_down[3] = {0, 0, 0}, lvl_base_k = 0;
    // LDS-staged post-order sweeps of the subtree form (items and slots on the device only)
    ClusterPlan cl;
};

// Everything pm_tree_upload sends to the device: the host tables and, under the name of the
// DevTree pointer each fills, the arrays that live on the device only (ht.child_off, ht.child_enc,
// ht.internal_id, ht.leaf_id and ht.cl.items / down_items / wg_off / slot_of go up as well).
struct TreePlan {
    HostTree ht;
    std::vector<int32_t> parent_dense, leaf_parent;
    std::vector<int32_t> up_order, down_order, leaf_down;
    std::vector<int32_t> child_enc_v, up_order_v, down_order_v, vleaf;
    std::vector<int32_t> child_enc_k, vinner;
    std::vector<int32_t> up_order_k, down_order_k;   // (host only: the device reads the subtree form's orders from its descriptors)
    std::vector<NodeDesc> down_desc, up_desc, up_desc_v, down_desc_v;
    std::vector<NodeDesc> up_desc_k, up_desc_g, up_desc_gs, down_desc_k, down_desc_ks;
    std::vector<TailDesc> tail_desc, tail_desc_v, tail_desc_k;
    std::vector<PartDesc> part_desc, part_desc_v, part_desc_k, part_desc_gs;
    std::vector<int32_t> pslot_k, pslot_g, pslot_gs, pslot_kc, pslot_gc, cl_pslot;
    std::vector<int32_t> lvl;
};

// pm_plan.cpp: the caller's CSR tree validated, numbered and planned (every form's levels,
// descriptors, up slots, tails and parts; the sweeps' schedule above the first level of at most
// cluster_max_level nodes).  PM_OK, or the code with its text in `err` (`out` is then not to be
// used).  Logs the phases tree.topology+levels ... tree.parts and the cluster.* counts.
int plan_tree(const pm_tree& t, int32_t cluster_max_level, bool cluster_chain, TreePlan& out, std::string& err);

// pm_cluster.cpp: the band / cluster / round / slot schedule above the first level of at most
// max_level nodes (0: none)
int plan_clusters(const HostTree& ht, const std::vector<int32_t>& up_order_k, const std::vector<int32_t>& child_enc_k,
                  const std::vector<int32_t>& parent_dense, const std::vector<int32_t>& vleaf, int32_t max_level,
                  bool chain_check, ClusterPlan& out);
bool plan_cluster_down(const HostTree& ht, const std::vector<int32_t>& down_order_k, const std::vector<NodeDesc>& down_desc_k,
                       const std::vector<int32_t>& child_enc_k, ClusterPlan& cl);

// host plumbing (pm_hostpar.cpp)
// Phase log (pm_phase_report): drivers append (name, seconds) of their host / device phases.
void phase_add(const std::string& name, double seconds);
struct PhaseClock {
    std::chrono::steady_clock::time_point t;
    PhaseClock();
    double lap(const char* name);   // seconds since construction / the last lap, logged as `name`
};
// One phase of pm_tree_upload: logged as tree.<what>, and with PM_UPLOAD_TIMING set printed on stderr
void tree_phase(PhaseClock& clock, const char* what);
int host_threads();   // host worker threads (PM_HOST_THREADS, else min(16, cores))
void host_parallel_for(int tasks, const std::function<void(int)>& fn);

}  // namespace pm
