// pm_plan.cpp -- the host plan of a tree (plan_tree): the caller's CSR tree validated and
// numbered, the level tables of its five forms (plain, leaf-parent `_v`, subtree `_k`, its Fitch
// groups `_g` and Sankoff groups `_gs`), the LDS sweeps' schedule (pm_cluster.cpp), and every
// descriptor, up slot, tail item and Sankoff part pm_tree_upload sends to the device.
//
// The reference keeps the tree as Node* with children vectors and rebuilds an
// unordered_map<string,int> per column (src/panman.cpp:1409-1417).  Here the topology is
// flattened once: dense internal indices, height levels for the post-order and depth levels for
// the pre-order, children encoded for the kernels.  Host code only (no HIP header): checked
// stand-alone by tests/test_plan_host.py.
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "pm_plan.h"

namespace pm {

namespace {

// The caller's tree as the steps read it (caller node ids throughout).
struct Topology {
    int32_t N = 0, root = -1;
    const int32_t* off = nullptr;
    const int32_t* idx = nullptr;
    std::vector<int32_t> parent, depth, height;
    std::vector<int32_t> bfs, dfs;   // breadth-first and depth-first pre-order from the root
    int32_t degree(int32_t u) const { return off[u + 1] - off[u]; }
};

int32_t degree(const HostTree& ht, int32_t d) { return ht.child_off[d + 1] - ht.child_off[d]; }
bool is_mat(int32_t x) { return x >= 0 && !(x & kVirtualBit); }   // a child with a record of its own
bool is_sub_shaped(int32_t x) { return x >= 0 && (x & kVirtualBit) && ((x >> kShapeShift) & 3); }

// A virtual leaf-parent: a non-root node of one or two children, all leaves.  It is never
// materialised; its parent evaluates it from the leaves in both passes (Fitch and Sankoff).
bool leaf_parent_like(const Topology& tp, int32_t u) {
    if (u == tp.root || tp.degree(u) == 0 || tp.degree(u) > 2) return false;
    for (int32_t e = tp.off[u]; e < tp.off[u + 1]; ++e)
        if (tp.degree(tp.idx[e]) > 0) return false;
    return true;
}

// Subtree form (Fitch, every leaf present): a node whose two children are leaves or
// two-leaf cherries, at least one a cherry, under a parent of out-degree <= 2, is also
// evaluated inline by its parent (shapes S2 = (cherry, leaf), S3 = (cherry, cherry)).
bool cherry2(const Topology& tp, int32_t u) { return tp.degree(u) == 2 && leaf_parent_like(tp, u); }
int sshape_of(const Topology& tp, int32_t u) {
    if (u == tp.root || tp.degree(u) != 2 || tp.parent[u] < 0 || tp.degree(tp.parent[u]) > 2) return 0;
    int cherries = 0;
    for (int32_t e = tp.off[u]; e < tp.off[u + 1]; ++e) {
        const int32_t ch = tp.idx[e];
        if (tp.degree(ch) == 0) continue;
        if (!cherry2(tp, ch)) return 0;
        ++cherries;
    }
    return cherries;   // 1: S2, 2: S3
}

// order = 0 .. count-1 sorted by key (stable), offs = the keys' offsets
template <class Key>
void bucket(int32_t levels, int32_t count, Key key, std::vector<int32_t>& offs, std::vector<int32_t>& order) {
    offs.assign(levels + 1, 0);
    for (int32_t i = 0; i < count; ++i) ++offs[key(i) + 1];
    for (int32_t k = 0; k < levels; ++k) offs[k + 1] += offs[k];
    order.assign(count, 0);
    std::vector<int32_t> cur(offs.begin(), offs.end() - 1);
    for (int32_t i = 0; i < count; ++i) order[cur[key(i)]++] = i;
}

// A levelled order without the nodes flagged in `dropped`: the levels keep their buckets.
void keep_levels(const std::vector<int32_t>& src_order, const std::vector<int32_t>& src_offs, const std::vector<uint8_t>& dropped,
                 std::vector<int32_t>& order, std::vector<int32_t>& offs) {
    order.clear();
    offs.assign(1, 0);
    for (size_t k = 0; k + 1 < src_offs.size(); ++k) {
        for (int32_t i = src_offs[k]; i < src_offs[k + 1]; ++i)
            if (!dropped[src_order[i]]) order.push_back(src_order[i]);
        offs.push_back((int32_t)order.size());
    }
}

// [levels + 1] from the (level, degree class) buckets
std::vector<int32_t> level_offsets(const std::vector<int32_t>& class_off) {
    std::vector<int32_t> level_off((class_off.size() - 1) / kDegreeClasses + 1, 0);
    for (size_t h = 0; h < level_off.size(); ++h) level_off[h] = class_off[h * kDegreeClasses];
    return level_off;
}

// [levels] 1: the level's nodes of out-degree <= 3 have no materialised child
std::vector<uint8_t> leafy_levels(const HostTree& ht, const std::vector<int32_t>& class_off, const std::vector<int32_t>& order,
                                  const std::vector<int32_t>& enc) {
    std::vector<uint8_t> out((class_off.size() - 1) / kDegreeClasses, 0);
    for (size_t l = 0; l < out.size(); ++l) {
        bool leafy = true;
        for (int32_t i = class_off[l * kDegreeClasses]; i < class_off[l * kDegreeClasses + 1] && leafy; ++i)
            for (int32_t e = ht.child_off[order[i]]; e < ht.child_off[order[i] + 1]; ++e) leafy &= !is_mat(enc[e]);
        out[l] = leafy;
    }
    return out;
}

// ---- the steps of plan_tree, in order --------------------------------------------------------

int read_topology(const pm_tree& t, Topology& tp, std::string& err) {
    if (!t.child_offsets || t.num_nodes < 2) return (err = "bad tree", PM_ERR_ARG);
    const int32_t N = tp.N = t.num_nodes;
    const int32_t* off = tp.off = t.child_offsets;
    const int32_t* idx = tp.idx = t.child_index;
    tp.root = t.root;
    if (off[0] != 0 || t.root < 0 || t.root >= N) return (err = "bad tree header", PM_ERR_ARG);
    for (int32_t i = 0; i < N; ++i)
        if (off[i + 1] < off[i]) return (err = "child offsets not monotone", PM_ERR_ARG);
    if (off[N] != N - 1) return (err = "a tree on N nodes has N-1 edges", PM_ERR_ARG);
    tp.parent.assign(N, -2);
    tp.parent[t.root] = -1;
    for (int32_t i = 0; i < N; ++i)
        for (int32_t e = off[i]; e < off[i + 1]; ++e) {
            const int32_t ch = idx[e];
            if (ch < 0 || ch >= N || tp.parent[ch] != -2) return (err = "child index invalid or repeated", PM_ERR_ARG);
            tp.parent[ch] = i;
        }
    if (off[t.root + 1] == off[t.root]) return (err = "root must be internal", PM_ERR_ARG);
    // a child's encoding keeps the dense internal index in its low kShapeShift bits (the
    // subtree shape above them): more internal nodes would mix shape bits into indices
    int64_t internal = 0;
    for (int32_t i = 0; i < N; ++i) internal += off[i + 1] > off[i];
    if (internal > kDenseMask) return (err = "too many internal nodes (limit 2^28 - 1)", PM_ERR_ARG);
    // BFS from the root: depth + connectivity.
    tp.bfs.reserve(N);
    tp.depth.assign(N, -1);
    tp.bfs.push_back(t.root);
    tp.depth[t.root] = 0;
    for (size_t h = 0; h < tp.bfs.size(); ++h) {
        const int32_t u = tp.bfs[h];
        for (int32_t e = off[u]; e < off[u + 1]; ++e) {
            tp.depth[idx[e]] = tp.depth[u] + 1;
            tp.bfs.push_back(idx[e]);
        }
    }
    if ((int32_t)tp.bfs.size() != N) return (err = "tree is not connected", PM_ERR_ARG);
    tp.height.assign(N, 0);
    for (int32_t k = N - 1; k >= 0; --k) {
        const int32_t u = tp.bfs[k];
        int32_t h = 0;
        for (int32_t e = off[u]; e < off[u + 1]; ++e) h = std::max(h, tp.height[idx[e]] + 1);
        tp.height[u] = off[u + 1] > off[u] ? h : 0;
    }
    tp.dfs.reserve(N);
    std::vector<int32_t> stack{t.root};
    while (!stack.empty()) {
        const int32_t u = stack.back();
        stack.pop_back();
        tp.dfs.push_back(u);
        for (int32_t e = off[u + 1] - 1; e >= off[u]; --e) stack.push_back(idx[e]);
    }
    return PM_OK;
}

// Dense internal indices and leaf ranks in DFS pre-order: a subtree's leaf rows and
// records are contiguous, and the nodes of one level (bucketed in dense order below)
// run in tree order, so neighbouring waves read neighbouring rows.
// Internal nodes: the materialised ones (every internal node but the virtual
// leaf-parents) by depth, then the virtual ones; DFS order within a depth.
// A pre-order level of the virtual-leaf-parent form is then a contiguous range of
// dense indices, so its waves know their node -- and its record masks -- without
// reading the level descriptor first (DevTree::down_dense).
void number_nodes(const Topology& tp, TreePlan& p) {
    HostTree& ht = p.ht;
    ht.num_nodes = tp.N;
    ht.root = tp.root;
    ht.dense_of.assign(tp.N, 0);
    std::vector<int32_t> inner;
    for (const int32_t i : tp.dfs) {
        if (tp.degree(i) > 0) {
            inner.push_back(i);
        } else {
            ht.dense_of[i] = -(int32_t)ht.leaf_id.size() - 1;
            ht.leaf_id.push_back(i);
        }
    }
    // stable counting sort by key: DFS order kept within a key
    int32_t maxd = 0;
    for (const int32_t i : inner) maxd = std::max(maxd, tp.depth[i]);
    // key: the materialised nodes by (depth, has an S2 / S3 child) -- a subtree-form
    // pre-order level, and each half of it, is one contiguous range of dense indices --
    // then the S2 / S3 nodes by depth -- the order of the subtree form's tail items, so a
    // tail wave knows its S2 / S3 node, and the masks its parent pushed there, from its
    // item index alone -- then the virtual leaf-parents.  (The leaf-parent form's levels,
    // which include the S2 / S3 nodes, are then two ranges: its pre-order kernels read
    // the node from the descriptor.)
    auto has_sub_child = [&](int32_t u) {
        for (int32_t e = tp.off[u]; e < tp.off[u + 1]; ++e)
            if (sshape_of(tp, tp.idx[e])) return true;
        return false;
    };
    const int32_t D1 = maxd + 1, nk = 4 * D1;
    std::vector<int32_t> key(inner.size()), start(nk + 1, 0);
    for (size_t k = 0; k < inner.size(); ++k) {
        const int32_t u = inner[k];
        key[k] = leaf_parent_like(tp, u) ? 3 * D1 + tp.depth[u] : sshape_of(tp, u) ? 2 * D1 + tp.depth[u]
                                                                 : 2 * tp.depth[u] + (has_sub_child(u) ? 1 : 0);
        ++start[key[k] + 1];
    }
    for (int32_t k = 0; k < nk; ++k) start[k + 1] += start[k];
    ht.internal_id.assign(inner.size(), 0);
    for (size_t k = 0; k < inner.size(); ++k) ht.internal_id[start[key[k]]++] = inner[k];
    for (size_t k = 0; k < ht.internal_id.size(); ++k) ht.dense_of[ht.internal_id[k]] = (int32_t)k;
    // the dense CSR
    const int32_t I = (int32_t)ht.internal_id.size(), L = (int32_t)ht.leaf_id.size();
    ht.child_off.assign(I + 1, 0);
    ht.child_enc.reserve(tp.N - 1);
    p.parent_dense.assign(I, -1);
    p.leaf_parent.assign(L, -1);
    for (int32_t d = 0; d < I; ++d) {
        const int32_t u = ht.internal_id[d];
        for (int32_t e = tp.off[u]; e < tp.off[u + 1]; ++e) {
            const int32_t ch = ht.dense_of[tp.idx[e]];
            ht.child_enc.push_back(ch);
            if (ch >= 0) p.parent_dense[ch] = d;
            else p.leaf_parent[-ch - 1] = d;
        }
        ht.child_off[d + 1] = (int32_t)ht.child_enc.size();
    }
}

// post-order levels: internal nodes by height 1..H, within a height by out-degree class;
// pre-order levels: internal nodes and leaves by depth
void level_orders(const Topology& tp, TreePlan& p) {
    HostTree& ht = p.ht;
    const int32_t I = (int32_t)ht.internal_id.size(), L = (int32_t)ht.leaf_id.size();
    int32_t H = 0, D = 0, DL = 0;
    for (int32_t d = 0; d < I; ++d) {
        H = std::max(H, tp.height[ht.internal_id[d]]);
        D = std::max(D, tp.depth[ht.internal_id[d]]);
    }
    for (int32_t l = 0; l < L; ++l) DL = std::max(DL, tp.depth[ht.leaf_id[l]]);
    bucket(H * kDegreeClasses, I,
           [&](int32_t d) { return (tp.height[ht.internal_id[d]] - 1) * kDegreeClasses + degree_class(degree(ht, d)); },
           ht.up_class_off, p.up_order);
    ht.up_level_off = level_offsets(ht.up_class_off);
    bucket(D + 1, I, [&](int32_t d) { return tp.depth[ht.internal_id[d]]; }, ht.down_level_off, p.down_order);
    bucket(DL + 1, L, [&](int32_t l) { return tp.depth[ht.leaf_id[l]]; }, ht.leaf_level_off, p.leaf_down);
}

// heavy child first: the internal child with the largest subtree (a materialised one
// on ties) leads its parent's child list, so it is the next node down the parent's
// chain in both the plain and the virtual-leaf-parent form (children order is free:
// every pass combines children commutatively and records are sorted on fetch)
void heavy_child_first(const Topology& tp, HostTree& ht) {
    std::vector<int64_t> sub(tp.N, 1);
    for (int32_t k = tp.N - 1; k >= 0; --k) {
        const int32_t u = tp.bfs[k];
        for (int32_t e = tp.off[u]; e < tp.off[u + 1]; ++e) sub[u] += sub[tp.idx[e]];
    }
    for (size_t d = 0; d + 1 < ht.child_off.size(); ++d) {
        int32_t best = -1;
        int64_t best_key = -1;
        for (int32_t e = ht.child_off[d]; e < ht.child_off[d + 1]; ++e) {
            const int32_t x = ht.child_enc[e];
            if (x < 0) continue;
            const int64_t key = sub[ht.internal_id[x]] * 2 + (leaf_parent_like(tp, ht.internal_id[x]) ? 0 : 1);
            if (key > best_key) { best_key = key; best = e; }
        }
        if (best > ht.child_off[d]) std::swap(ht.child_enc[best], ht.child_enc[ht.child_off[d]]);
    }
}

// virtual leaf-parents (Fitch level kernels): tagged in the child encodings, their leaves in
// vleaf, dropped from the levels (which keep their (height, degree class) buckets)
void leaf_parent_form(const Topology& tp, TreePlan& p) {
    HostTree& ht = p.ht;
    const int32_t I = (int32_t)ht.internal_id.size();
    std::vector<uint8_t> virt(I, 0);
    p.child_enc_v = ht.child_enc;
    p.vleaf.assign((size_t)I * 4, -1);
    for (int32_t d = 0; d < I; ++d) {
        if (!leaf_parent_like(tp, ht.internal_id[d])) continue;
        virt[d] = 1;
        ht.num_virtual += 1;
        for (int32_t e = ht.child_off[d], k = 0; e < ht.child_off[d + 1]; ++e, ++k) p.vleaf[(size_t)d * 4 + k] = -ht.child_enc[e] - 1;
    }
    for (auto& x : p.child_enc_v)
        if (x >= 0 && virt[x]) x |= kVirtualBit;
    keep_levels(p.up_order, ht.up_class_off, virt, p.up_order_v, ht.up_class_off_v);
    ht.up_level_off_v = level_offsets(ht.up_class_off_v);
    ht.up_leafy_v = leafy_levels(ht, ht.up_class_off_v, p.up_order_v, p.child_enc_v);
    keep_levels(p.down_order, ht.down_level_off, virt, p.down_order_v, ht.down_level_off_v);
    ht.down_dense_v = true;   // pre-order item k of the virtual form is dense index k
    for (size_t k = 0; k < p.down_order_v.size(); ++k) ht.down_dense_v &= p.down_order_v[k] == (int32_t)k;
}

// subtree form (Fitch, all leaves present): S2 / S3 nodes dropped from the levels as well;
// child encodings carry the shape (kShapeShift), vleaf their leaves (a, b[, c[, d]]) and
// vinner their cherries (x[, y])
void subtree_form(const Topology& tp, TreePlan& p) {
    HostTree& ht = p.ht;
    const int32_t I = (int32_t)ht.internal_id.size();
    p.child_enc_k = p.child_enc_v;
    p.vinner.assign((size_t)I * 2, -1);
    ht.sshape.assign(I, 0);
    for (int32_t d = 0; d < I; ++d) {
        const int sh = sshape_of(tp, ht.internal_id[d]);
        if (!sh) continue;
        ht.sshape[d] = (uint8_t)sh;
        // leaves: the cherries' leaves first, then the lone leaf (S2)
        int32_t nl = 0, ni = 0;
        for (int32_t e = ht.child_off[d]; e < ht.child_off[d + 1]; ++e) {
            const int32_t x = ht.child_enc[e];
            if (x < 0) continue;
            p.vinner[(size_t)d * 2 + ni++] = x;
            for (int32_t f = ht.child_off[x]; f < ht.child_off[x + 1]; ++f) p.vleaf[(size_t)d * 4 + nl++] = -ht.child_enc[f] - 1;
        }
        for (int32_t e = ht.child_off[d]; e < ht.child_off[d + 1]; ++e)
            if (ht.child_enc[e] < 0) p.vleaf[(size_t)d * 4 + nl++] = -ht.child_enc[e] - 1;
        ht.num_sshape += 1;
    }
    for (auto& x : p.child_enc_k)
        if (is_mat(x) && ht.sshape[x]) x = (x | kVirtualBit) | (ht.sshape[x] << kShapeShift);
    keep_levels(p.up_order_v, ht.up_class_off_v, ht.sshape, p.up_order_k, ht.up_class_off_k);
    ht.up_level_off_k = level_offsets(ht.up_class_off_k);
    ht.up_leafy_k = leafy_levels(ht, ht.up_class_off_k, p.up_order_k, p.child_enc_k);
    keep_levels(p.down_order_v, ht.down_level_off_v, ht.sshape, p.down_order_k, ht.down_level_off_k);
    // each subtree-form pre-order level is one dense range (dense key: depth, then S2/S3 last)
    ht.down_dense_base_k.assign(ht.down_level_off_k.size() - 1, -1);
    ht.down_dense_k = true;
    for (size_t l = 0; l + 1 < ht.down_level_off_k.size(); ++l) {
        const int32_t a = ht.down_level_off_k[l], b = ht.down_level_off_k[l + 1];
        if (a == b) continue;
        for (int32_t i = a; i < b; ++i) ht.down_dense_k &= p.down_order_k[i] == p.down_order_k[a] + (i - a);
        ht.down_dense_base_k[l] = p.down_order_k[a];
    }
}

// LDS-staged post-order sweeps of the subtree form (PM_OPT_CLUSTER, pm_cluster.cpp)
void plan_sweeps(TreePlan& p, int32_t max_level, bool chain, PhaseClock& clock) {
    ClusterPlan& cl = p.ht.cl;
    plan_clusters(p.ht, p.up_order_k, p.child_enc_k, p.parent_dense, p.vleaf, max_level, chain, cl);
    for (const NodeDesc& x : cl.items) cl.max_degree = std::max(cl.max_degree, x.e1 - x.e0);   // (the schedule reads it: run_paths)
    tree_phase(clock, "clusters");
    // (counts: the sweeps' first level, bands, workgroups per tile, longest workgroup in rounds)
    phase_add("cluster.first_level", (double)cl.h0);
    phase_add("cluster.bands", cl.band_wg.empty() ? 0.0 : (double)(cl.band_wg.size() - 1));
    phase_add("cluster.workgroups", cl.wg_off.empty() ? 0.0 : (double)(cl.wg_off.size() - 1));
    phase_add("cluster.max_rounds", (double)cl.max_rounds);
}

// the level items of the first `count` nodes of `order` over the form's child encodings
std::vector<NodeDesc> make_desc(const TreePlan& p, const std::vector<int32_t>& order, size_t count, const std::vector<int32_t>& enc) {
    std::vector<NodeDesc> desc(count);
    for (size_t k = 0; k < count; ++k) {
        const int32_t d = order[k];
        NodeDesc& x = desc[k];
        x = NodeDesc{};
        x.node = d;
        x.parent = p.parent_dense[d];
        x.e0 = p.ht.child_off[d];
        x.e1 = p.ht.child_off[d + 1];
        x.c0 = enc[x.e0];
        x.c1 = x.e1 - x.e0 > 1 ? enc[x.e0 + 1] : 0;
        for (int j = 0; j < 4; ++j) {
            x.vl0[j] = x.c0 >= 0 && (x.c0 & kVirtualBit) ? p.vleaf[(size_t)(x.c0 & kDenseMask) * 4 + j] : -1;
            x.vl1[j] = x.e1 - x.e0 > 1 && x.c1 >= 0 && (x.c1 & kVirtualBit) ? p.vleaf[(size_t)(x.c1 & kDenseMask) * 4 + j] : -1;
        }
    }
    return desc;
}

// pre-order descriptors carry the grandparent and great-grandparent (k_down level groups
// recompute the ancestors' finals)
std::vector<NodeDesc> make_down_desc(const TreePlan& p, const std::vector<int32_t>& order, const std::vector<int32_t>& enc) {
    std::vector<NodeDesc> desc = make_desc(p, order, order.size(), enc);
    for (NodeDesc& x : desc) {
        x.pad0 = x.parent >= 0 ? p.parent_dense[x.parent] : -1;
        x.pad1 = x.pad0 >= 0 ? p.parent_dense[x.pad0] : -1;
    }
    return desc;
}

void level_descriptors(TreePlan& p) {
    p.down_desc = make_down_desc(p, p.down_order, p.ht.child_enc);
    p.down_desc_v = make_down_desc(p, p.down_order_v, p.child_enc_v);
    p.up_desc = make_desc(p, p.up_order, p.up_order.size(), p.ht.child_enc);
    p.up_desc_v = make_desc(p, p.up_order_v, p.up_order_v.size(), p.child_enc_v);
    p.up_desc_k = make_desc(p, p.up_order_k, p.up_order_k.size(), p.child_enc_k);
}

// Grouped post-order launches of the subtree form (PM_OPT_UP_GROUP): a node of
// out-degree <= 3 joins the launch of its latest materialised children when each of
// those is of out-degree <= max_rc (Fitch 3; Sankoff 2: a recomputed child's Z0 is the
// AND-else-OR of its children only when it is binary), computed from earlier launches
// only, and among its first two children -- its wave recomputes them in registers
// (k_fitch_up / k_sankoff_up <.., GROUP>, the descriptor's pad0 / pad1 = their descriptor
// indices) -- otherwise the launch after.  Children come before parents in up_order_k
// (height order).  Only nodes of heights with at most kUpGroupNodes nodes join a child's
// launch: big levels fill the chip by themselves and pay for the recomputation (measured
// at N*).
// `levels`: only the subtree form's first `levels` post-order levels (Fitch with the LDS-staged
// sweeps: the levels below them; the sweeps take the rest).  Returns the grouped order.
struct GroupTables {
    std::vector<int32_t>&level_off, &class_off;
    std::vector<uint8_t>&leafy, &recomp;
    std::vector<int32_t>& plain;
};
std::vector<int32_t> make_groups(const TreePlan& p, int32_t max_rc, int32_t levels, GroupTables out, std::vector<NodeDesc>& desc) {
    const HostTree& ht = p.ht;
    const std::vector<int32_t>& enc = p.child_enc_k;
    const int32_t I = (int32_t)ht.internal_id.size();
    levels = std::min<int32_t>(levels, (int32_t)ht.up_level_off_k.size() - 1);
    const size_t count = (size_t)ht.up_level_off_k[levels];   // the nodes of p.up_order_k that group
    std::vector<int32_t> lv(I, -1), inl((size_t)I * 2, -1), hsize(I, 0);
    for (int32_t h = 0; h < levels; ++h)
        for (int32_t i = ht.up_level_off_k[h]; i < ht.up_level_off_k[h + 1]; ++i)
            hsize[p.up_order_k[i]] = ht.up_level_off_k[h + 1] - ht.up_level_off_k[h];
    std::vector<uint8_t> gen(I, 0);
    int32_t G = 0;
    for (size_t i = 0; i < count; ++i) {
        const int32_t d = p.up_order_k[i], e0 = ht.child_off[d], e1 = ht.child_off[d + 1];
        int32_t M = -1;
        for (int32_t e = e0; e < e1; ++e)
            if (is_mat(enc[e])) M = std::max(M, lv[enc[e]]);
        if (M < 0) {
            lv[d] = 0;
        } else {
            bool ok = degree_class(e1 - e0) == 0 && hsize[d] <= kUpGroupNodes;
            int top = 0, g = 0;   // children in launch M, the deepest recomputation below them
            for (int32_t e = e0; e < e1 && ok; ++e) {
                const int32_t x = enc[e];
                if (is_mat(x) && lv[x] == M) {
                    ok = degree(ht, x) <= max_rc && e - e0 < 2 && gen[x] < kUpGroupDepth;
                    ++top;
                    g = std::max(g, (int)gen[x]);
                }
            }
            ok = ok && (g == 0 || top == 1);   // a chain below: one recomputed child only
            lv[d] = ok ? M : M + 1;
            gen[d] = ok ? (uint8_t)(g + 1) : 0;
            if (ok)
                for (int32_t e = e0; e < e0 + 2 && e < e1; ++e)
                    if (is_mat(enc[e]) && lv[enc[e]] == M) inl[(size_t)d * 2 + (e - e0)] = enc[e];
        }
        G = std::max(G, lv[d] + 1);
    }
    // bucket by (launch, degree class), children-first order kept inside a bucket; in the
    // out-degree <= 3 class the plain nodes first (binary, neither of the children an S2 / S3
    // subtree nor recomputed here): one launch of the lean kernel covers them
    out.class_off.assign((size_t)G * kDegreeClasses + 1, 0);
    auto key = [&](int32_t d) { return lv[d] * kDegreeClasses + degree_class(degree(ht, d)); };
    auto plain = [&](int32_t d) {
        if (degree(ht, d) > 2 || inl[(size_t)d * 2] >= 0 || inl[(size_t)d * 2 + 1] >= 0) return false;
        for (int32_t e = ht.child_off[d]; e < ht.child_off[d + 1]; ++e)
            if (is_sub_shaped(enc[e])) return false;
        return true;
    };
    for (size_t i = 0; i < count; ++i) ++out.class_off[key(p.up_order_k[i]) + 1];
    for (size_t k = 0; k + 1 < out.class_off.size(); ++k) out.class_off[k + 1] += out.class_off[k];
    std::vector<int32_t> order(count), cur(out.class_off.begin(), out.class_off.end() - 1), pos(I, -1);
    out.plain.assign(G, 0);
    for (int pass = 0; pass < 2; ++pass)
        for (size_t i = 0; i < count; ++i) {
            const int32_t d = p.up_order_k[i];
            if (plain(d) != (pass == 0)) continue;
            pos[d] = cur[key(d)]++;
            order[pos[d]] = d;
            if (pass == 0) ++out.plain[lv[d]];
        }
    out.level_off = level_offsets(out.class_off);
    out.leafy = leafy_levels(ht, out.class_off, order, enc);
    desc = make_desc(p, order, order.size(), enc);
    out.recomp.assign(G, 0);   // launches where some node recomputes a child (the others run the plain kernel)
    for (size_t k = 0; k < order.size(); ++k) {
        const int32_t d = order[k];
        desc[k].pad0 = inl[(size_t)d * 2] >= 0 ? pos[inl[(size_t)d * 2]] : -1;
        desc[k].pad1 = inl[(size_t)d * 2 + 1] >= 0 ? pos[inl[(size_t)d * 2 + 1]] : -1;
        if (desc[k].pad0 >= 0 || desc[k].pad1 >= 0) out.recomp[lv[d]] = 1;
    }
    return order;
}

// up slots: each descriptor's parent item and child slot (the parent's first / second
// child) in the same array
std::vector<int32_t> make_pslot(const std::vector<NodeDesc>& desc, int32_t I) {
    std::vector<int32_t> pos(I, -1), ps(desc.size(), -1);
    for (size_t k = 0; k < desc.size(); ++k) pos[desc[k].node] = (int32_t)k;
    for (size_t k = 0; k < desc.size(); ++k)
        for (int j = 0; j < 2 && j < desc[k].e1 - desc[k].e0; ++j) {
            const int32_t x = j == 0 ? desc[k].c0 : desc[k].c1;
            if (is_mat(x) && pos[x] >= 0) ps[pos[x]] = (int32_t)k * 2 + j;
        }
    return ps;
}

// with the sweeps: a level item (either up order) whose parent is swept pushes into the
// parent's sweep item's up slot (item cl.upm_base + item); a swept node whose parent is in a
// later band likewise (a parent in its own cluster reads its LDS slot instead)
void redirect_to_sweeps(TreePlan& p) {
    const HostTree& ht = p.ht;
    const ClusterPlan& cl = ht.cl;
    const int32_t I = (int32_t)ht.internal_id.size();
    p.pslot_kc = p.pslot_k;
    p.pslot_gc = p.pslot_g;
    p.cl_pslot.assign(cl.items.size(), -1);
    if (cl.item_of.empty()) return;
    std::vector<int32_t> pos_k(I, -1), pos_g(I, -1);
    for (size_t k = 0; k < p.up_desc_k.size(); ++k) pos_k[p.up_desc_k[k].node] = (int32_t)k;
    for (size_t k = 0; k < p.up_desc_g.size(); ++k) pos_g[p.up_desc_g[k].node] = (int32_t)k;
    for (int32_t par = 0; par < I; ++par) {
        if (cl.item_of[par] < 0) continue;   // swept parents: their first two materialised children
        const int32_t e0 = ht.child_off[par], e1 = ht.child_off[par + 1];
        for (int j = 0; j < 2 && e0 + j < e1; ++j) {
            const int32_t x = p.child_enc_k[e0 + j];
            if (!is_mat(x)) continue;
            const int32_t to = (cl.upm_base + cl.item_of[par]) * 2 + j;
            if (cl.item_of[x] >= 0) {
                p.cl_pslot[cl.item_of[x]] = cl.slot_of[x] >= 0 ? -1 : to;
            } else {
                if (pos_k[x] >= 0) p.pslot_kc[pos_k[x]] = to;
                if (pos_g[x] >= 0) p.pslot_gc[pos_g[x]] = to;
            }
        }
    }
}

// the grouped launches of the subtree form with their up slots
void groups_and_up_slots(TreePlan& p) {
    HostTree& ht = p.ht;
    const int32_t I = (int32_t)ht.internal_id.size();
    const int32_t all_levels = (int32_t)ht.up_level_off_k.size() - 1;
    // (with a sweep plan the grouped Fitch launches stop below its first level: ht.cl.h0)
    make_groups(p, 3, ht.cl.band_wg.size() > 1 ? ht.cl.h0 : all_levels,
                {ht.up_level_off_g, ht.up_class_off_g, ht.up_leafy_g, ht.up_recomp_g, ht.up_plain_g}, p.up_desc_g);
    p.pslot_k = make_pslot(p.up_desc_k, I);
    p.pslot_g = make_pslot(p.up_desc_g, I);
    ht.cl.upm_base = (int32_t)std::max(p.up_desc_k.size(), p.up_desc_g.size());
    redirect_to_sweeps(p);
    ht.up_items_k = (int32_t)p.up_desc_k.size();
    ht.up_items_g = (int32_t)p.up_desc_g.size();
    // Sankoff: binary recomputed children; its part descriptors are the subtree form's (nodes
    // above 255 children never group), so pad0 / pad1 here index the grouped array only
    make_groups(p, 2, all_levels, {ht.up_level_off_gs, ht.up_class_off_gs, ht.up_leafy_gs, ht.up_recomp_gs, ht.up_plain_gs},
                p.up_desc_gs);
    p.pslot_gs = make_pslot(p.up_desc_gs, I);
    ht.up_items_gs = (int32_t)p.up_desc_gs.size();
}

// subtree-form pre-order descriptors list only the children the level kernel handles:
// S2 / S3 children are tail items (k_tail<.., SUB>); a node left with none gets a
// materialised placeholder (c0 = 0, no loads, no records)
void subtree_pre_order(TreePlan& p) {
    p.down_desc_k = make_down_desc(p, p.down_order_k, p.child_enc_k);
    p.down_desc_ks = p.down_desc_k;   // (PM_OPT_SUB_DOWN: S children kept)
    for (NodeDesc& x : p.down_desc_k) {
        const int32_t deg = x.e1 - x.e0;
        if (deg > 2) continue;   // S2 / S3 nodes have parents of out-degree <= 2
        int32_t keep_enc[2], keep_vl[2][4], nk = 0;
        for (int j = 0; j < deg; ++j) {
            const int32_t enc = j == 0 ? x.c0 : x.c1;
            if (is_sub_shaped(enc)) continue;
            keep_enc[nk] = enc;
            for (int q = 0; q < 4; ++q) keep_vl[nk][q] = j == 0 ? x.vl0[q] : x.vl1[q];
            ++nk;
        }
        if (nk == deg) continue;
        x.e0 = 0;
        x.e1 = std::max(nk, 1);
        x.c0 = nk > 0 ? keep_enc[0] : 0;
        x.c1 = nk > 1 ? keep_enc[1] : 0;
        for (int q = 0; q < 4; ++q) {
            x.vl0[q] = nk > 0 ? keep_vl[0][q] : -1;
            x.vl1[q] = nk > 1 ? keep_vl[1][q] : -1;
        }
    }
    // the pre-order over the sweeps' clusters (every level swept only)
    p.ht.cl.down = plan_cluster_down(p.ht, p.down_order_k, p.down_desc_k, p.child_enc_k, p.ht.cl);
    phase_add("cluster.down", p.ht.cl.down ? 1.0 : 0.0);
}

// A form's tail items: the leaf and virtual children beyond a node's first two, by their
// parent's pre-order level (neighbouring waves read neighbouring parents)
std::vector<TailDesc> make_tail(const TreePlan& p, const std::vector<int32_t>& order, const std::vector<int32_t>& offs,
                                const std::vector<int32_t>& enc) {
    const HostTree& ht = p.ht;
    std::vector<TailDesc> tail;
    for (int32_t d : order)
        for (int32_t e = ht.child_off[d] + 2; e < ht.child_off[d + 1]; ++e) {
            const int32_t x = enc[e];
            if (is_mat(x)) continue;   // materialised child: its own wave
            TailDesc t{};
            t.parent = d;
            t.enc = x;
            t.ix = t.iy = -1;
            for (int j = 0; j < 4; ++j) t.vl[j] = x >= 0 ? p.vleaf[(size_t)(x & kDenseMask) * 4 + j] : -1;
            t.id[0] = x < 0 ? ht.leaf_id[-x - 1] : ht.internal_id[x & kDenseMask];
            for (int j = 0; j < 4; ++j) t.id[1 + j] = t.vl[j] >= 0 ? ht.leaf_id[t.vl[j]] : -1;
            tail.push_back(t);
        }
    std::vector<int32_t> lvl_of(ht.internal_id.size(), 0);
    for (size_t l = 0; l + 1 < offs.size(); ++l)
        for (int32_t i = offs[l]; i < offs[l + 1]; ++i) lvl_of[order[i]] = (int32_t)l;
    std::stable_sort(tail.begin(), tail.end(), [&](const TailDesc& x, const TailDesc& y) { return lvl_of[x.parent] < lvl_of[y.parent]; });
    return tail;
}

// subtree form: every S2 / S3 node, in dense order (item k = dense index sbase + k), then
// the leaf-parent form's items (the subtree form's levels are the leaf-parent form's, S2 / S3
// nodes removed)
int tails(TreePlan& p, std::string& err) {
    HostTree& ht = p.ht;
    const int32_t I = (int32_t)ht.internal_id.size();
    p.tail_desc = make_tail(p, p.down_order, ht.down_level_off, ht.child_enc);
    p.tail_desc_v = make_tail(p, p.down_order_v, ht.down_level_off_v, p.child_enc_v);
    ht.num_tail = (int32_t)p.tail_desc.size();
    ht.num_tail_v = (int32_t)p.tail_desc_v.size();
    ht.sbase = -1;
    for (int32_t d = 0; d < I; ++d) {
        if (!ht.sshape[d]) continue;
        if (ht.sbase < 0) ht.sbase = d;
        TailDesc t{};
        t.parent = p.parent_dense[d];
        t.enc = (d | kVirtualBit) | (ht.sshape[d] << kShapeShift);
        for (int j = 0; j < 4; ++j) t.vl[j] = p.vleaf[(size_t)d * 4 + j];
        t.ix = ht.internal_id[p.vinner[(size_t)d * 2]];
        t.iy = p.vinner[(size_t)d * 2 + 1] >= 0 ? ht.internal_id[p.vinner[(size_t)d * 2 + 1]] : -1;
        t.id[0] = ht.internal_id[d];
        for (int j = 0; j < 4; ++j) t.id[1 + j] = t.vl[j] >= 0 ? ht.leaf_id[t.vl[j]] : -1;
        p.tail_desc_k.push_back(t);
    }
    ht.num_tail_s = (int32_t)p.tail_desc_k.size();
    for (int32_t k = 0; k < ht.num_tail_s; ++k)
        if (ht.sbase + k >= I || !ht.sshape[ht.sbase + k]) return (err = "S2 / S3 nodes not one dense range", PM_ERR_STATE);
    p.tail_desc_k.insert(p.tail_desc_k.end(), p.tail_desc_v.begin(), p.tail_desc_v.end());
    ht.num_tail_k = (int32_t)p.tail_desc_k.size();
    return PM_OK;
}

// Sankoff parts: nodes of out-degree > 255, children cut into kPartChildren-wide parts.
// The up descriptors' pad0 = the node's first part (the Fitch level kernels do not read it);
// in the grouped order only above 255 children (grouped nodes have out-degree <= 3: pad0 /
// pad1 stay theirs)
void parts_of(std::vector<NodeDesc>& ud, bool grouped, std::vector<int32_t>& po, std::vector<int32_t>& degree_out,
              std::vector<PartDesc>& parts) {
    po.assign(ud.size() + 1, 0);
    degree_out.assign(ud.size(), 0);
    for (size_t k = 0; k < ud.size(); ++k) {
        const int32_t deg = ud[k].e1 - ud[k].e0;
        degree_out[k] = deg;
        const int32_t np = deg > 255 ? (deg + kPartChildren - 1) / kPartChildren : 0;
        for (int32_t j = 0; j < np; ++j) parts.push_back(PartDesc{(int32_t)k, j, po[k] + j, 0});
        po[k + 1] = po[k] + np;
        if (!grouped || deg > 255) ud[k].pad0 = po[k];
    }
}

void sankoff_parts(TreePlan& p) {
    HostTree& ht = p.ht;
    parts_of(p.up_desc, false, ht.part_off, ht.up_degree[0], p.part_desc);
    parts_of(p.up_desc_v, false, ht.part_off_v, ht.up_degree[1], p.part_desc_v);
    parts_of(p.up_desc_k, false, ht.part_off_k, ht.up_degree[2], p.part_desc_k);
    parts_of(p.up_desc_gs, true, ht.part_off_gs, ht.up_degree[3], p.part_desc_gs);
}

// level tables on the device: every form's buckets back to back, their offsets in lvl_*
void level_table(TreePlan& p) {
    HostTree& ht = p.ht;
    const std::vector<int32_t>* up[5] = {&ht.up_class_off, &ht.up_class_off_v, &ht.up_class_off_k, &ht.up_class_off_g,
                                         &ht.up_class_off_gs};
    const std::vector<int32_t>* dn[3] = {&ht.down_level_off, &ht.down_level_off_v, &ht.down_level_off_k};
    for (int f = 0; f < 5; ++f) {
        ht.lvl_up[f] = (int64_t)p.lvl.size();
        p.lvl.insert(p.lvl.end(), up[f]->begin(), up[f]->end());
        if (f >= 3) continue;
        ht.lvl_down[f] = (int64_t)p.lvl.size();
        p.lvl.insert(p.lvl.end(), dn[f]->begin(), dn[f]->end());
    }
    ht.lvl_base_k = (int64_t)p.lvl.size();
    p.lvl.insert(p.lvl.end(), ht.down_dense_base_k.begin(), ht.down_dense_base_k.end());
}

}  // namespace

int plan_tree(const pm_tree& t, int32_t cluster_max_level, bool cluster_chain, TreePlan& out, std::string& err) {
    PhaseClock clock;
    out = TreePlan{};
    Topology tp;
    if (const int rc = read_topology(t, tp, err)) return rc;
    number_nodes(tp, out);
    level_orders(tp, out);
    tree_phase(clock, "topology+levels");
    heavy_child_first(tp, out.ht);
    tree_phase(clock, "heavy child");
    leaf_parent_form(tp, out);
    tree_phase(clock, "virtual form");
    subtree_form(tp, out);
    tree_phase(clock, "subtree form");
    plan_sweeps(out, cluster_max_level, cluster_chain, clock);
    level_descriptors(out);
    groups_and_up_slots(out);
    subtree_pre_order(out);
    tree_phase(clock, "descriptors");
    if (const int rc = tails(out, err)) return rc;
    sankoff_parts(out);
    level_table(out);
    tree_phase(clock, "parts");
    return PM_OK;
}

}  // namespace pm
