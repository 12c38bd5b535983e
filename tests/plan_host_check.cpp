// plan_host_check.cpp -- the tree planner (panman_amd/csrc/pm_plan.cpp, pm_cluster.cpp) without
// a GPU: hand-written plans of three tiny trees, every argument error, and the plan's invariants
// over the trees given on the command line and the library's two generators, each under four
// sweep settings.  Built and run by tests/test_plan_host.py under ASan / UBSan.
//
//   plan_host_check [--digest] TREE...    TREE: a text file "N root n_off n_idx", the offsets, the indices
//
// --digest: no checks; per (tree, setting) one line "field count fnv1a64" for every array and
// scalar of the TreePlan (two planners that print the same lines built the same plan).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "../panman_amd/csrc/pm_plan.h"

using namespace pm;

namespace {

int g_failed = 0;
std::string g_where;

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            if (++g_failed <= 40) std::fprintf(stderr, "%s: line %d: %s\n", g_where.c_str(), __LINE__, #cond); \
        }                                                                                        \
    } while (0)

static_assert(sizeof(NodeDesc) == 64 && sizeof(TailDesc) == 64 && sizeof(PartDesc) == 16, "no padding bytes");

struct Tree {
    std::string name;
    int32_t n = 0, root = 0;
    std::vector<int32_t> off, idx;
    pm_tree view() const {
        pm_tree t{};
        t.num_nodes = n;
        t.root = root;
        t.child_offsets = off.data();
        t.child_index = idx.data();
        return t;
    }
};

bool read_tree(const char* path, Tree& t) {
    std::ifstream in(path);
    int64_t n_off = 0, n_idx = 0;
    if (!(in >> t.n >> t.root >> n_off >> n_idx)) return false;
    t.off.resize(n_off);
    t.idx.resize(n_idx);
    for (auto& x : t.off) in >> x;
    for (auto& x : t.idx) in >> x;
    const char* slash = std::strrchr(path, '/');
    t.name = slash ? slash + 1 : path;
    return (bool)in;
}

Tree generated(const char* name, bool sars, int64_t leaves) {
    Tree t;
    t.name = name;
    t.off.assign(2 * leaves + 1, 0);
    t.idx.assign(2 * leaves, 0);
    int64_t n = 2 * leaves - 1;
    const int rc = sars ? pm_synth_tree_sars_like(leaves, 7, t.off.data(), t.idx.data(), &t.root, &n)
                        : pm_synth_tree_random_join(leaves, 7, t.off.data(), t.idx.data(), &t.root);
    if (rc != PM_OK) std::exit(3);
    t.n = (int32_t)n;
    t.off.resize(n + 1);
    t.idx.resize(t.off[n]);
    return t;
}

struct Setting {
    int32_t max_level;
    bool chain;
};
const Setting kSettings[4] = {{kClMaxLevel, true}, {1 << 20, false}, {1, false}, {0, false}};

// ---- digest ---------------------------------------------------------------------------------
uint64_t fnv(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
template <class T>
void line(const char* field, const std::vector<T>& v) {
    std::printf("%s %zu %016" PRIx64 "\n", field, v.size(), fnv(v.data(), v.size() * sizeof(T)));
}
void scalar(const char* field, int64_t v) { std::printf("%s 1 %016" PRIx64 "\n", field, fnv(&v, sizeof v)); }

void digest(const TreePlan& p) {
    const HostTree& h = p.ht;
#define V(x) line(#x, x)
#define S(x) scalar(#x, (int64_t)(x))
    S(h.num_nodes); S(h.root); V(h.dense_of); V(h.internal_id); V(h.leaf_id); V(h.up_level_off); V(h.up_class_off);
    V(h.down_level_off); V(h.leaf_level_off); V(h.child_off); V(h.child_enc); V(h.up_level_off_v); V(h.up_class_off_v);
    V(h.up_leafy_v); V(h.down_level_off_v); S(h.num_virtual); S(h.down_dense_v); S(h.num_tail); S(h.num_tail_v);
    V(h.part_off); V(h.part_off_v); V(h.part_off_k); V(h.part_off_gs);
    V(h.up_degree[0]); V(h.up_degree[1]); V(h.up_degree[2]); V(h.up_degree[3]);
    V(h.up_level_off_k); V(h.up_class_off_k); V(h.down_level_off_k); V(h.down_dense_base_k); V(h.up_leafy_k);
    V(h.up_level_off_g); V(h.up_class_off_g); V(h.up_leafy_g); V(h.up_recomp_g); V(h.up_plain_g); V(h.up_plain_gs);
    V(h.up_level_off_gs); V(h.up_class_off_gs); V(h.up_leafy_gs); V(h.up_recomp_gs);
    S(h.down_dense_k); S(h.up_items_k); S(h.up_items_g); S(h.up_items_gs); S(h.num_sshape); V(h.sshape);
    S(h.num_tail_k); S(h.num_tail_s); S(h.sbase);
    for (int f = 0; f < 5; ++f) S(h.lvl_up[f]);
    for (int f = 0; f < 3; ++f) S(h.lvl_down[f]);
    S(h.lvl_base_k);
    S(h.cl.h0); S(h.cl.max_rounds); V(h.cl.items); V(h.cl.wg_off); V(h.cl.band_wg); V(h.cl.band_level);
    V(h.cl.slot_of); V(h.cl.item_of); S(h.cl.n_items); S(h.cl.max_degree); S(h.cl.upm_base); V(h.cl.down_items);
    S(h.cl.down);
    V(p.parent_dense); V(p.leaf_parent); V(p.up_order); V(p.down_order); V(p.leaf_down); V(p.child_enc_v);
    V(p.up_order_v); V(p.down_order_v); V(p.vleaf); V(p.child_enc_k); V(p.vinner); V(p.down_desc); V(p.up_desc);
    V(p.up_desc_v); V(p.down_desc_v); V(p.up_desc_k); V(p.up_desc_g); V(p.up_desc_gs); V(p.down_desc_k);
    V(p.down_desc_ks); V(p.tail_desc); V(p.tail_desc_v); V(p.tail_desc_k); V(p.part_desc); V(p.part_desc_v);
    V(p.part_desc_k); V(p.part_desc_gs); V(p.pslot_k); V(p.pslot_g); V(p.pslot_gs); V(p.pslot_kc); V(p.pslot_gc);
    V(p.cl_pslot); V(p.lvl);
#undef V
#undef S
}

// ---- invariants -----------------------------------------------------------------------------
bool is_mat(int32_t x) { return x >= 0 && !(x & kVirtualBit); }
bool is_virt(int32_t x) { return x >= 0 && (x & kVirtualBit); }
bool is_sub(int32_t x) { return is_virt(x) && ((x >> kShapeShift) & 3); }

bool monotone(const std::vector<int32_t>& v) { return std::is_sorted(v.begin(), v.end()); }

// c0 / c1 / vl* / e0 / e1 of a descriptor against the form's child list
void check_children(const TreePlan& p, const NodeDesc& x, const std::vector<int32_t>& enc) {
    const HostTree& h = p.ht;
    const int32_t I = (int32_t)h.internal_id.size();
    CHECK(x.node >= 0 && x.node < I);
    if (x.node < 0 || x.node >= I) return;
    CHECK(x.e0 == h.child_off[x.node] && x.e1 == h.child_off[x.node + 1]);
    const int32_t deg = x.e1 - x.e0;
    CHECK(x.c0 == enc[x.e0]);
    CHECK(x.c1 == (deg > 1 ? enc[x.e0 + 1] : 0));
    for (int j = 0; j < 4; ++j) {
        CHECK(x.vl0[j] == (is_virt(x.c0) ? p.vleaf[(size_t)(x.c0 & kDenseMask) * 4 + j] : -1));
        CHECK(x.vl1[j] == (deg > 1 && is_virt(x.c1) ? p.vleaf[(size_t)(x.c1 & kDenseMask) * 4 + j] : -1));
    }
}

// One up order: `nodes` = the materialised nodes it must hold, each once, materialised children
// in an earlier level; in a grouped order (`grouped`) a same-launch child is one of the first two
// and named by pad0 / pad1.
void check_up_order(const TreePlan& p, const std::vector<NodeDesc>& desc, const std::vector<int32_t>* order,
                    const std::vector<int32_t>& level_off, const std::vector<int32_t>& class_off,
                    const std::vector<int32_t>& enc, const std::vector<int32_t>& nodes, bool grouped) {
    const HostTree& h = p.ht;
    const int32_t I = (int32_t)h.internal_id.size();
    CHECK(!level_off.empty() && class_off.size() == (level_off.size() - 1) * kDegreeClasses + 1);
    CHECK(monotone(level_off) && monotone(class_off));
    for (size_t l = 0; l < level_off.size(); ++l) CHECK(level_off[l] == class_off[l * kDegreeClasses]);
    CHECK(level_off.back() == (int32_t)desc.size());
    if (order) CHECK(order->size() == desc.size());
    std::vector<int32_t> pos(I, -1), lvl(I, -1);
    for (size_t l = 0; l + 1 < level_off.size(); ++l)
        for (int32_t i = level_off[l]; i < level_off[l + 1] && i < (int32_t)desc.size(); ++i) {
            const int32_t d = desc[i].node;
            if (order) CHECK((*order)[i] == d);
            CHECK(d >= 0 && d < I && pos[d] < 0);   // once
            if (d < 0 || d >= I) continue;
            pos[d] = i;
            lvl[d] = (int32_t)l;
        }
    size_t held = 0;
    for (const int32_t d : nodes) {
        CHECK(pos[d] >= 0);
        held += pos[d] >= 0;
    }
    CHECK(held == desc.size());   // and nothing else
    for (size_t k = 0; k < desc.size(); ++k) {
        const NodeDesc& x = desc[k];
        check_children(p, x, enc);
        CHECK(x.parent == p.parent_dense[x.node]);
        const int32_t deg = x.e1 - x.e0;
        // (class bucket of its level)
        const size_t b = (size_t)lvl[x.node] * kDegreeClasses + degree_class(deg);
        CHECK((int32_t)k >= class_off[b] && (int32_t)k < class_off[b + 1]);
        for (int32_t e = x.e0; e < x.e1; ++e) {
            if (!is_mat(enc[e])) continue;
            const int32_t ch = enc[e];
            CHECK(pos[ch] >= 0 && lvl[ch] <= lvl[x.node]);
            if (lvl[ch] < lvl[x.node]) continue;
            CHECK(grouped && e - x.e0 < 2 && deg <= 3 && (e == x.e0 ? x.pad0 : x.pad1) == pos[ch]);
        }
        if (grouped && deg <= 3)   // a named child is a same-launch one
            for (int j = 0; j < 2; ++j) {
                const int32_t named = j == 0 ? x.pad0 : x.pad1;
                if (named < 0) continue;
                CHECK(j < deg && named < (int32_t)desc.size() && desc[named].node == enc[x.e0 + j] &&
                      lvl[desc[named].node] == lvl[x.node]);
            }
    }
}

// up slots of one order: 2 * (parent item) + j exactly for the parent's j-th child, j < 2
std::vector<int32_t> expected_pslot(const TreePlan& p, const std::vector<NodeDesc>& desc) {
    const HostTree& h = p.ht;
    std::vector<int32_t> pos(h.internal_id.size(), -1), want(desc.size(), -1);
    for (size_t k = 0; k < desc.size(); ++k) pos[desc[k].node] = (int32_t)k;
    for (size_t k = 0; k < desc.size(); ++k) {
        const int32_t d = desc[k].node, par = p.parent_dense[d];
        if (par < 0 || pos[par] < 0) continue;
        for (int j = 0; j < 2 && h.child_off[par] + j < h.child_off[par + 1]; ++j)
            if (p.child_enc_k[h.child_off[par] + j] == d) want[k] = 2 * pos[par] + j;
    }
    return want;
}

// ... with the sweeps: a level item whose parent is swept (and is not swept itself) pushes into
// the parent's sweep item
std::vector<int32_t> expected_pslot_c(const TreePlan& p, const std::vector<NodeDesc>& desc, std::vector<int32_t> want) {
    const HostTree& h = p.ht;
    if (h.cl.item_of.empty()) return want;
    for (size_t k = 0; k < desc.size(); ++k) {
        const int32_t d = desc[k].node, par = p.parent_dense[d];
        if (par < 0 || h.cl.item_of[par] < 0 || h.cl.item_of[d] >= 0) continue;
        for (int j = 0; j < 2 && h.child_off[par] + j < h.child_off[par + 1]; ++j)
            if (p.child_enc_k[h.child_off[par] + j] == d) want[k] = 2 * (h.cl.upm_base + h.cl.item_of[par]) + j;
    }
    return want;
}

// a form's tail: every leaf or virtual child beyond the first two of the nodes of `order`, once
void check_tail(const TreePlan& p, const TailDesc* tail, size_t n, const std::vector<int32_t>& order,
                const std::vector<int32_t>& level_off, const std::vector<int32_t>& enc) {
    const HostTree& h = p.ht;
    std::map<int32_t, int32_t> want;   // enc -> parent (a child has one parent: encodings are unique)
    for (const int32_t d : order)
        for (int32_t e = h.child_off[d] + 2; e < h.child_off[d + 1]; ++e)
            if (!is_mat(enc[e])) want[enc[e]] = d;
    CHECK(want.size() == n);
    std::vector<int32_t> lvl_of(h.internal_id.size(), -1);
    for (size_t l = 0; l + 1 < level_off.size(); ++l)
        for (int32_t i = level_off[l]; i < level_off[l + 1]; ++i) lvl_of[order[i]] = (int32_t)l;
    int32_t last = -1;
    for (size_t k = 0; k < n; ++k) {
        const TailDesc& t = tail[k];
        const auto it = want.find(t.enc);
        CHECK(it != want.end() && it->second == t.parent);
        if (it == want.end()) continue;
        want.erase(it);   // once
        CHECK(lvl_of[t.parent] >= last);   // by the parent's pre-order level
        last = lvl_of[t.parent];
        CHECK(t.ix == -1 && t.iy == -1 && t.pad[0] == 0 && t.pad[1] == 0 && t.pad[2] == 0);
        CHECK(t.id[0] == (t.enc < 0 ? h.leaf_id[-t.enc - 1] : h.internal_id[t.enc & kDenseMask]));
        for (int j = 0; j < 4; ++j) {
            CHECK(t.vl[j] == (t.enc >= 0 ? p.vleaf[(size_t)(t.enc & kDenseMask) * 4 + j] : -1));
            CHECK(t.id[1 + j] == (t.vl[j] >= 0 ? h.leaf_id[t.vl[j]] : -1));
        }
    }
    CHECK(want.empty());
}

void check_parts(const std::vector<NodeDesc>& desc, const std::vector<int32_t>& part_off, const std::vector<PartDesc>& parts,
                 const std::vector<int32_t>& degree, bool pad0_is_part) {
    CHECK(part_off.size() == desc.size() + 1 && degree.size() == desc.size());
    if (part_off.size() != desc.size() + 1 || degree.size() != desc.size()) return;
    CHECK(part_off[0] == 0);
    size_t q = 0;
    for (size_t k = 0; k < desc.size(); ++k) {
        const int32_t deg = desc[k].e1 - desc[k].e0;
        const int32_t np = deg > 255 ? (deg + 254) / 255 : 0;
        CHECK(degree[k] == deg && part_off[k + 1] == part_off[k] + np);
        if (pad0_is_part || deg > 255) CHECK(desc[k].pad0 == part_off[k]);
        if (pad0_is_part) CHECK(desc[k].pad1 == 0);
        for (int32_t j = 0; j < np; ++j, ++q) {
            CHECK(q < parts.size());
            if (q >= parts.size()) return;
            CHECK(parts[q].item == (int32_t)k && parts[q].sub == j && parts[q].global == part_off[k] + j && parts[q].pad == 0);
        }
    }
    CHECK(q == parts.size());
}

void check_slice(const std::vector<int32_t>& lvl, int64_t at, const std::vector<int32_t>& table) {
    CHECK(at >= 0 && at + (int64_t)table.size() <= (int64_t)lvl.size());
    if (at < 0 || at + (int64_t)table.size() > (int64_t)lvl.size()) return;
    CHECK(std::equal(table.begin(), table.end(), lvl.begin() + at));
}

void check_down(const TreePlan& p, const std::vector<NodeDesc>& desc, const std::vector<int32_t>* order,
                const std::vector<int32_t>& level_off, const std::vector<int32_t>& enc, const std::vector<int32_t>& nodes) {
    const HostTree& h = p.ht;
    CHECK(monotone(level_off) && level_off.back() == (int32_t)desc.size() && desc.size() == nodes.size());
    if (order) CHECK(order->size() == desc.size());
    std::vector<int32_t> lvl(h.internal_id.size(), -1);
    for (size_t l = 0; l + 1 < level_off.size(); ++l)
        for (int32_t i = level_off[l]; i < level_off[l + 1]; ++i) {
            CHECK(lvl[desc[i].node] < 0);
            lvl[desc[i].node] = (int32_t)l;
            if (order) CHECK((*order)[i] == desc[i].node);
        }
    for (const int32_t d : nodes) CHECK(lvl[d] >= 0);
    for (const NodeDesc& x : desc) {
        check_children(p, x, enc);
        CHECK(x.parent == p.parent_dense[x.node]);
        const int32_t gp = x.parent >= 0 ? p.parent_dense[x.parent] : -1;
        CHECK(x.pad0 == gp && x.pad1 == (gp >= 0 ? p.parent_dense[gp] : -1));
        for (int32_t e = x.e0; e < x.e1; ++e)
            if (is_mat(enc[e])) CHECK(lvl[enc[e]] == lvl[x.node] + 1);
    }
}

void check_plan(const Tree& t, const TreePlan& p) {
    const HostTree& h = p.ht;
    const int32_t N = t.n, I = (int32_t)h.internal_id.size(), L = (int32_t)h.leaf_id.size();
    // the numbering: inverse permutations
    CHECK(h.num_nodes == N && h.root == t.root && I + L == N && (int32_t)h.dense_of.size() == N);
    for (int32_t d = 0; d < I; ++d) CHECK(h.dense_of[h.internal_id[d]] == d);
    for (int32_t l = 0; l < L; ++l) CHECK(h.dense_of[h.leaf_id[l]] == -l - 1);
    for (int32_t v = 0; v < N; ++v) {
        const bool inner = t.off[v + 1] > t.off[v];
        CHECK(inner == (h.dense_of[v] >= 0));
        CHECK(inner ? h.internal_id[h.dense_of[v]] == v : h.leaf_id[-h.dense_of[v] - 1] == v);
    }
    // the dense CSR: the caller's children (in any order) and the parents
    CHECK((int32_t)h.child_off.size() == I + 1 && monotone(h.child_off) && (int32_t)h.child_enc.size() == N - 1);
    for (int32_t d = 0; d < I; ++d) {
        const int32_t u = h.internal_id[d];
        std::vector<int32_t> want, got(h.child_enc.begin() + h.child_off[d], h.child_enc.begin() + h.child_off[d + 1]);
        for (int32_t e = t.off[u]; e < t.off[u + 1]; ++e) want.push_back(h.dense_of[t.idx[e]]);
        std::sort(want.begin(), want.end());
        std::sort(got.begin(), got.end());
        CHECK(want == got);
        for (int32_t e = h.child_off[d]; e < h.child_off[d + 1]; ++e) {
            const int32_t x = h.child_enc[e];
            CHECK(x >= 0 ? p.parent_dense[x] == d : p.leaf_parent[-x - 1] == d);
        }
    }
    CHECK(p.parent_dense[h.dense_of[t.root]] == -1);
    // the forms: virtual leaf-parents and S2 / S3 nodes from their definitions
    std::vector<uint8_t> virt(I, 0), sshape(I, 0);
    auto degree = [&](int32_t d) { return h.child_off[d + 1] - h.child_off[d]; };
    for (int32_t d = 0; d < I; ++d) {
        if (h.internal_id[d] == t.root || degree(d) > 2) continue;
        bool all = true;
        for (int32_t e = h.child_off[d]; e < h.child_off[d + 1]; ++e) all &= h.child_enc[e] < 0;
        virt[d] = all;
    }
    for (int32_t d = 0; d < I; ++d) {
        const int32_t par = p.parent_dense[d];
        if (par < 0 || degree(d) != 2 || degree(par) > 2) continue;
        int cherries = 0;
        bool ok = true;
        for (int32_t e = h.child_off[d]; e < h.child_off[d + 1]; ++e) {
            const int32_t x = h.child_enc[e];
            if (x < 0) continue;
            ok &= virt[x] && degree(x) == 2;
            ++cherries;
        }
        sshape[d] = ok ? (uint8_t)cherries : 0;
    }
    CHECK(h.sshape == sshape);
    int64_t nv = 0, ns = 0;
    for (int32_t d = 0; d < I; ++d) nv += virt[d], ns += sshape[d] != 0;
    CHECK(h.num_virtual == nv && h.num_sshape == ns);
    CHECK(p.child_enc_v.size() == h.child_enc.size() && p.child_enc_k.size() == h.child_enc.size());
    CHECK(p.vleaf.size() == (size_t)I * 4 && p.vinner.size() == (size_t)I * 2);
    for (size_t e = 0; e < h.child_enc.size(); ++e) {
        const int32_t x = h.child_enc[e];
        CHECK(p.child_enc_v[e] == (x >= 0 && virt[x] ? x | kVirtualBit : x));
        CHECK(p.child_enc_k[e] == (x >= 0 && virt[x]     ? x | kVirtualBit
                                   : x >= 0 && sshape[x] ? x | kVirtualBit | (sshape[x] << kShapeShift)
                                                         : x));
    }
    for (int32_t d = 0; d < I; ++d) {   // vleaf / vinner: a virtual node's leaves; an S node's cherries' leaves, then its own
        std::vector<int32_t> leaves, inner;
        if (virt[d] || sshape[d]) {
            for (int32_t e = h.child_off[d]; e < h.child_off[d + 1]; ++e)
                if (h.child_enc[e] >= 0) {
                    inner.push_back(h.child_enc[e]);
                    for (int32_t f = h.child_off[h.child_enc[e]]; f < h.child_off[h.child_enc[e] + 1]; ++f)
                        leaves.push_back(-h.child_enc[f] - 1);
                }
            for (int32_t e = h.child_off[d]; e < h.child_off[d + 1]; ++e)
                if (h.child_enc[e] < 0) leaves.push_back(-h.child_enc[e] - 1);
        }
        leaves.resize(4, -1);
        inner.resize(2, -1);
        CHECK(std::equal(leaves.begin(), leaves.end(), p.vleaf.begin() + (size_t)d * 4));
        CHECK(std::equal(inner.begin(), inner.end(), p.vinner.begin() + (size_t)d * 2));
    }
    std::vector<int32_t> all_nodes, nodes_v, nodes_k;
    for (int32_t d = 0; d < I; ++d) {
        all_nodes.push_back(d);
        if (!virt[d]) nodes_v.push_back(d);
        if (!virt[d] && !sshape[d]) nodes_k.push_back(d);
    }
    // the five up orders
    check_up_order(p, p.up_desc, &p.up_order, h.up_level_off, h.up_class_off, h.child_enc, all_nodes, false);
    check_up_order(p, p.up_desc_v, &p.up_order_v, h.up_level_off_v, h.up_class_off_v, p.child_enc_v, nodes_v, false);
    check_up_order(p, p.up_desc_k, nullptr, h.up_level_off_k, h.up_class_off_k, p.child_enc_k, nodes_k, false);
    // (the Fitch groups stop below the sweeps' first level)
    const int32_t levels_k = (int32_t)h.up_level_off_k.size() - 1;
    const int32_t levels_g = h.cl.band_wg.size() > 1 ? std::min(h.cl.h0, levels_k) : levels_k;
    std::vector<int32_t> nodes_g;
    for (int32_t i = 0; i < h.up_level_off_k[levels_g]; ++i) nodes_g.push_back(p.up_desc_k[i].node);
    check_up_order(p, p.up_desc_g, nullptr, h.up_level_off_g, h.up_class_off_g, p.child_enc_k, nodes_g, true);
    check_up_order(p, p.up_desc_gs, nullptr, h.up_level_off_gs, h.up_class_off_gs, p.child_enc_k, nodes_k, true);
    CHECK(h.up_items_k == (int32_t)p.up_desc_k.size() && h.up_items_g == (int32_t)p.up_desc_g.size() &&
          h.up_items_gs == (int32_t)p.up_desc_gs.size());
    for (const NodeDesc& x : p.up_desc_gs)   // Sankoff recomputes binary children only
        for (int j = 0; j < 2; ++j) {
            const int32_t named = j == 0 ? x.pad0 : x.pad1;
            if (x.e1 - x.e0 <= 3 && named >= 0) CHECK(p.up_desc_gs[named].e1 - p.up_desc_gs[named].e0 <= 2);
        }
    // the pre-orders
    check_down(p, p.down_desc, &p.down_order, h.down_level_off, h.child_enc, all_nodes);
    check_down(p, p.down_desc_v, &p.down_order_v, h.down_level_off_v, p.child_enc_v, nodes_v);
    check_down(p, p.down_desc_ks, nullptr, h.down_level_off_k, p.child_enc_k, nodes_k);
    CHECK(p.down_desc_k.size() == p.down_desc_ks.size());
    for (size_t k = 0; k < p.down_desc_k.size() && k < p.down_desc_ks.size(); ++k) {
        // trimmed: the S2 / S3 children of a node of out-degree <= 2 are left to the tail
        NodeDesc want = p.down_desc_ks[k];
        const int32_t deg = want.e1 - want.e0;
        const bool s0 = deg > 0 && is_sub(want.c0), s1 = deg > 1 && is_sub(want.c1);
        if (deg <= 2 && (s0 || s1)) {
            NodeDesc w = want;
            const bool keep1 = deg > 1 && !s1;   // the one child that can stay
            const bool keep0 = !s0;
            w.e0 = 0;
            w.e1 = 1;
            w.c0 = keep0 ? want.c0 : keep1 ? want.c1 : 0;
            w.c1 = 0;
            for (int j = 0; j < 4; ++j) {
                w.vl0[j] = keep0 ? want.vl0[j] : keep1 ? want.vl1[j] : -1;
                w.vl1[j] = -1;
            }
            want = w;
        }
        CHECK(std::memcmp(&want, &p.down_desc_k[k], sizeof want) == 0);
    }
    CHECK(h.down_dense_base_k.size() + 1 == h.down_level_off_k.size());
    for (size_t l = 0; l + 1 < h.down_level_off_k.size(); ++l) {
        const int32_t a = h.down_level_off_k[l], b = h.down_level_off_k[l + 1];
        CHECK(h.down_dense_base_k[l] == (a < b ? p.down_desc_ks[a].node : -1));
    }
    // leaves by depth
    CHECK((int32_t)p.leaf_down.size() == L && monotone(h.leaf_level_off) && h.leaf_level_off.back() == L);
    {
        std::vector<int32_t> seen(L, 0);
        for (const int32_t l : p.leaf_down) CHECK(l >= 0 && l < L && !seen[l]++);
    }
    // up slots
    const std::vector<int32_t> want_k = expected_pslot(p, p.up_desc_k), want_g = expected_pslot(p, p.up_desc_g);
    CHECK(p.pslot_k == want_k && p.pslot_g == want_g && p.pslot_gs == expected_pslot(p, p.up_desc_gs));
    CHECK(h.cl.upm_base == (int32_t)std::max(p.up_desc_k.size(), p.up_desc_g.size()));
    CHECK(p.pslot_kc == expected_pslot_c(p, p.up_desc_k, want_k) && p.pslot_gc == expected_pslot_c(p, p.up_desc_g, want_g));
    CHECK(p.cl_pslot.size() == h.cl.items.size());
    {
        std::vector<int32_t> want(h.cl.items.size(), -1);
        for (int32_t d = 0; d < I && !h.cl.item_of.empty(); ++d) {
            const int32_t par = p.parent_dense[d];
            if (h.cl.item_of[d] < 0 || par < 0 || h.cl.item_of[par] < 0 || h.cl.slot_of[d] >= 0) continue;
            for (int j = 0; j < 2 && h.child_off[par] + j < h.child_off[par + 1]; ++j)
                if (p.child_enc_k[h.child_off[par] + j] == d) want[h.cl.item_of[d]] = 2 * (h.cl.upm_base + h.cl.item_of[par]) + j;
        }
        CHECK(p.cl_pslot == want);
    }
    // tails
    CHECK(h.num_tail == (int32_t)p.tail_desc.size() && h.num_tail_v == (int32_t)p.tail_desc_v.size() &&
          h.num_tail_k == (int32_t)p.tail_desc_k.size() && h.num_tail_s == (int32_t)ns &&
          p.tail_desc_k.size() == (size_t)ns + p.tail_desc_v.size());
    check_tail(p, p.tail_desc.data(), p.tail_desc.size(), p.down_order, h.down_level_off, h.child_enc);
    check_tail(p, p.tail_desc_v.data(), p.tail_desc_v.size(), p.down_order_v, h.down_level_off_v, p.child_enc_v);
    if (p.tail_desc_k.size() == (size_t)ns + p.tail_desc_v.size()) {
        if (!p.tail_desc_v.empty())
            CHECK(std::memcmp(p.tail_desc_k.data() + ns, p.tail_desc_v.data(), p.tail_desc_v.size() * sizeof(TailDesc)) == 0);
        CHECK((ns == 0) == (h.sbase < 0));
        for (int32_t k = 0; k < (int32_t)ns; ++k) {
            const TailDesc& s = p.tail_desc_k[k];
            const int32_t d = h.sbase + k;
            CHECK((s.enc & kDenseMask) == d && d < I && sshape[d]);
            if (d >= I || !sshape[d]) continue;
            CHECK(s.enc == (d | kVirtualBit | (sshape[d] << kShapeShift)) && s.parent == p.parent_dense[d]);
            CHECK(s.ix == h.internal_id[p.vinner[(size_t)d * 2]]);
            CHECK(s.iy == (p.vinner[(size_t)d * 2 + 1] >= 0 ? h.internal_id[p.vinner[(size_t)d * 2 + 1]] : -1));
            CHECK(s.id[0] == h.internal_id[d] && s.pad[0] == 0 && s.pad[1] == 0 && s.pad[2] == 0);
            for (int j = 0; j < 4; ++j) {
                CHECK(s.vl[j] == p.vleaf[(size_t)d * 4 + j]);
                CHECK(s.id[1 + j] == (s.vl[j] >= 0 ? h.leaf_id[s.vl[j]] : -1));
            }
        }
    }
    // parts
    check_parts(p.up_desc, h.part_off, p.part_desc, h.up_degree[0], true);
    check_parts(p.up_desc_v, h.part_off_v, p.part_desc_v, h.up_degree[1], true);
    check_parts(p.up_desc_k, h.part_off_k, p.part_desc_k, h.up_degree[2], true);
    check_parts(p.up_desc_gs, h.part_off_gs, p.part_desc_gs, h.up_degree[3], false);
    // the level table
    check_slice(p.lvl, h.lvl_up[0], h.up_class_off);
    check_slice(p.lvl, h.lvl_up[1], h.up_class_off_v);
    check_slice(p.lvl, h.lvl_up[2], h.up_class_off_k);
    check_slice(p.lvl, h.lvl_up[3], h.up_class_off_g);
    check_slice(p.lvl, h.lvl_up[4], h.up_class_off_gs);
    check_slice(p.lvl, h.lvl_down[0], h.down_level_off);
    check_slice(p.lvl, h.lvl_down[1], h.down_level_off_v);
    check_slice(p.lvl, h.lvl_down[2], h.down_level_off_k);
    check_slice(p.lvl, h.lvl_base_k, h.down_dense_base_k);
    // the sweeps
    const ClusterPlan& cl = h.cl;
    CHECK(monotone(cl.wg_off) && cl.n_items == (int32_t)cl.items.size());
    if (!cl.wg_off.empty()) CHECK(cl.wg_off.front() == 0 && cl.wg_off.back() == (int32_t)cl.items.size());
    for (size_t w = 0; w + 1 < cl.wg_off.size(); ++w) CHECK(cl.wg_off[w + 1] - cl.wg_off[w] <= kClMaxSteps);
    for (const int32_t s : cl.slot_of) CHECK(s >= -1 && s < kClSlots);
    for (size_t k = 0; k < cl.items.size(); ++k) {
        const NodeDesc& x = cl.items[k];
        check_children(p, x, p.child_enc_k);
        CHECK(x.parent >= -1 && x.parent < kClSlots && x.pad0 >= -1 && x.pad0 < kClSlots && x.pad1 >= -1 && x.pad1 < kClSlots);
        CHECK(cl.item_of[x.node] == (int32_t)k && cl.slot_of[x.node] == x.parent);
    }
    CHECK(cl.down_items.empty() || cl.down_items.size() == cl.items.size());
    CHECK(cl.down == !cl.down_items.empty());
    for (const NodeDesc& x : cl.down_items)
        CHECK(x.pad0 >= -1 && x.pad0 < kClFSlots && x.pad1 >= -1 && x.pad1 < kClFSlots);
}

// ---- hand-written plans ---------------------------------------------------------------------
constexpr int32_t VB = kVirtualBit, S2 = 1 << kShapeShift, S3 = 2 << kShapeShift;
using IV = std::vector<int32_t>;
using BV = std::vector<uint8_t>;

NodeDesc ND(int32_t node, int32_t parent, int32_t e0, int32_t e1, int32_t c0, int32_t c1, int32_t pad0, int32_t pad1,
            IV vl0 = {-1, -1, -1, -1}, IV vl1 = {-1, -1, -1, -1}) {
    NodeDesc x{};
    x.node = node, x.parent = parent, x.e0 = e0, x.e1 = e1, x.c0 = c0, x.c1 = c1, x.pad0 = pad0, x.pad1 = pad1;
    for (int j = 0; j < 4; ++j) x.vl0[j] = vl0[j], x.vl1[j] = vl1[j];
    return x;
}
TailDesc TD(int32_t parent, int32_t enc, int32_t ix, int32_t iy, IV vl, IV id) {
    TailDesc t{};
    t.parent = parent, t.enc = enc, t.ix = ix, t.iy = iy;
    for (int j = 0; j < 4; ++j) t.vl[j] = vl[j];
    for (int j = 0; j < 5; ++j) t.id[j] = id[j];
    return t;
}
template <class T>
bool same(const std::vector<T>& got, const std::vector<T>& want) {
    return got.size() == want.size() && (got.empty() || std::memcmp(got.data(), want.data(), got.size() * sizeof(T)) == 0);
}
#define EQ(field, ...) CHECK(same(field, __VA_ARGS__))

IV cat(std::initializer_list<IV> parts) {
    IV out;
    for (const IV& v : parts) out.insert(out.end(), v.begin(), v.end());
    return out;
}

TreePlan plan_of(const Tree& t, Setting s) {
    TreePlan p;
    std::string err;
    const pm_tree v = t.view();
    const int rc = plan_tree(v, s.max_level, s.chain, p, err);
    CHECK(rc == PM_OK && err.empty());
    return p;
}

// ((a,b),c): ids a b c = 0 1 2, the cherry 3, the root 4.  Default sweeps.
void hand_cherry() {
    g_where = "hand ((a,b),c)";
    Tree t;
    t.n = 5, t.root = 4, t.off = {0, 0, 0, 0, 2, 4}, t.idx = {0, 1, 3, 2};
    const TreePlan p = plan_of(t, kSettings[0]);
    const HostTree& h = p.ht;
    const IV none4 = {-1, -1, -1, -1}, ab = {0, 1, -1, -1};
    EQ(h.internal_id, IV{4, 3});
    EQ(h.leaf_id, IV{0, 1, 2});
    EQ(h.dense_of, IV{-1, -2, -3, 1, 0});
    EQ(h.child_off, IV{0, 2, 4});
    EQ(h.child_enc, IV{1, -3, -1, -2});
    EQ(p.parent_dense, IV{-1, 0});
    EQ(p.leaf_parent, IV{1, 1, 0});
    EQ(p.up_order, IV{1, 0});
    EQ(h.up_class_off, IV{0, 1, 1, 1, 1, 2, 2, 2, 2});
    EQ(h.up_level_off, IV{0, 1, 2});
    EQ(p.down_order, IV{0, 1});
    EQ(h.down_level_off, IV{0, 1, 2});
    EQ(p.leaf_down, IV{2, 0, 1});
    EQ(h.leaf_level_off, IV{0, 0, 1, 3});
    CHECK(h.num_virtual == 1 && h.num_sshape == 0 && h.sbase == -1);
    EQ(p.child_enc_v, IV{1 | VB, -3, -1, -2});
    EQ(p.child_enc_k, IV{1 | VB, -3, -1, -2});
    EQ(p.vleaf, IV{-1, -1, -1, -1, 0, 1, -1, -1});
    EQ(p.vinner, IV{-1, -1, -1, -1});
    EQ(h.sshape, BV{0, 0});
    EQ(p.up_order_v, IV{0});
    EQ(h.up_class_off_v, IV{0, 0, 0, 0, 0, 1, 1, 1, 1});
    EQ(h.up_level_off_v, IV{0, 0, 1});
    EQ(h.up_leafy_v, BV{1, 1});
    EQ(p.down_order_v, IV{0});
    EQ(h.down_level_off_v, IV{0, 1, 1});
    CHECK(h.down_dense_v && h.down_dense_k);
    EQ(h.up_class_off_k, IV{0, 0, 0, 0, 0, 1, 1, 1, 1});
    EQ(h.up_level_off_k, IV{0, 0, 1});
    EQ(h.up_leafy_k, BV{1, 1});
    EQ(h.down_level_off_k, IV{0, 1, 1});
    EQ(h.down_dense_base_k, IV{0, -1});
    // the sweeps take both levels (one cluster of one node), so the Fitch groups hold nothing
    CHECK(h.cl.h0 == 0 && h.cl.max_rounds == 1 && h.cl.n_items == 1 && h.cl.upm_base == 1 && h.cl.down);
    EQ(h.cl.wg_off, IV{0, 1});
    EQ(h.cl.band_wg, IV{0, 1});
    EQ(h.cl.band_level, IV{0, 2});
    EQ(h.cl.slot_of, IV{-1, -1});
    EQ(h.cl.item_of, IV{0, -1});
    const std::vector<NodeDesc> root_v = {ND(0, -1, 0, 2, 1 | VB, -3, -1, -1, ab)};
    EQ(h.cl.items, root_v);
    EQ(h.cl.down_items, root_v);
    EQ(p.down_desc, std::vector<NodeDesc>{ND(0, -1, 0, 2, 1, -3, -1, -1), ND(1, 0, 2, 4, -1, -2, -1, -1)});
    EQ(p.down_desc_v, root_v);
    EQ(p.down_desc_k, root_v);
    EQ(p.down_desc_ks, root_v);
    EQ(p.up_desc, std::vector<NodeDesc>{ND(1, 0, 2, 4, -1, -2, 0, 0), ND(0, -1, 0, 2, 1, -3, 0, 0)});
    const std::vector<NodeDesc> root_up = {ND(0, -1, 0, 2, 1 | VB, -3, 0, 0, ab)};
    EQ(p.up_desc_v, root_up);
    EQ(p.up_desc_k, root_up);
    EQ(p.up_desc_g, std::vector<NodeDesc>{});
    EQ(p.up_desc_gs, root_v);   // (pad0 = pad1 = -1: no recomputed child)
    EQ(h.up_level_off_g, IV{0});
    EQ(h.up_class_off_g, IV{0});
    CHECK(h.up_leafy_g.empty() && h.up_recomp_g.empty() && h.up_plain_g.empty());
    EQ(h.up_level_off_gs, IV{0, 1});
    EQ(h.up_class_off_gs, IV{0, 1, 1, 1, 1});
    EQ(h.up_leafy_gs, BV{1});
    EQ(h.up_recomp_gs, BV{0});
    EQ(h.up_plain_gs, IV{1});
    CHECK(h.up_items_k == 1 && h.up_items_g == 0 && h.up_items_gs == 1);
    EQ(p.pslot_k, IV{-1});
    EQ(p.pslot_kc, IV{-1});
    EQ(p.pslot_gs, IV{-1});
    EQ(p.cl_pslot, IV{-1});
    CHECK(p.pslot_g.empty() && p.pslot_gc.empty());
    CHECK(p.tail_desc.empty() && p.tail_desc_v.empty() && p.tail_desc_k.empty());   // no tails
    CHECK(h.num_tail == 0 && h.num_tail_v == 0 && h.num_tail_k == 0 && h.num_tail_s == 0);
    EQ(h.part_off, IV{0, 0, 0});
    EQ(h.part_off_v, IV{0, 0});
    EQ(h.part_off_k, IV{0, 0});
    EQ(h.part_off_gs, IV{0, 0});
    EQ(h.up_degree[0], IV{2, 2});
    EQ(h.up_degree[1], IV{2});
    EQ(h.up_degree[2], IV{2});
    EQ(h.up_degree[3], IV{2});
    CHECK(p.part_desc.empty() && p.part_desc_v.empty() && p.part_desc_k.empty() && p.part_desc_gs.empty());
    EQ(p.lvl, cat({h.up_class_off, h.down_level_off, h.up_class_off_v, h.down_level_off_v, h.up_class_off_k,
                   h.down_level_off_k, IV{0}, IV{0, 1, 1, 1, 1}, IV{0, -1}}));
    const int64_t up[5] = {0, 12, 24, 36, 37}, down[3] = {9, 21, 33};
    CHECK(std::equal(up, up + 5, h.lvl_up) && std::equal(down, down + 3, h.lvl_down) && h.lvl_base_k == 42);
    (void)none4;
}

// ((((a,b),c),((d,e),(f,g))),h): leaves a..h = 0..7; (a,b) 8, (d,e) 9, (f,g) 10, the S2 node
// ((a,b),c) 11, the S3 node ((d,e),(f,g)) 12, their parent 13, the root 14.  No sweeps.
void hand_shapes() {
    g_where = "hand ((((a,b),c),((d,e),(f,g))),h)";
    Tree t;
    t.n = 15, t.root = 14;
    t.off = {0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 4, 6, 8, 10, 12, 14};
    t.idx = {0, 1, 3, 4, 5, 6, 8, 2, 9, 10, 11, 12, 13, 7};
    const TreePlan p = plan_of(t, kSettings[3]);
    const HostTree& h = p.ht;
    const IV ab = {0, 1, -1, -1}, de = {3, 4, -1, -1}, fg = {5, 6, -1, -1}, abc = {0, 1, 2, -1}, defg = {3, 4, 5, 6};
    CHECK(h.num_virtual == 3 && h.num_sshape == 2 && h.sbase == 2);
    // root, the S nodes' parent, S2, S3, the cherries
    EQ(h.internal_id, IV{14, 13, 11, 12, 8, 9, 10});
    EQ(h.leaf_id, IV{0, 1, 2, 3, 4, 5, 6, 7});
    EQ(h.child_off, IV{0, 2, 4, 6, 8, 10, 12, 14});
    // (heavy child first: the seven-node S3 subtree leads the five-node S2 one)
    EQ(h.child_enc, IV{1, -8, 3, 2, 4, -3, 5, 6, -1, -2, -4, -5, -6, -7});
    EQ(p.parent_dense, IV{-1, 0, 1, 1, 2, 3, 3});
    EQ(p.leaf_parent, IV{4, 4, 2, 5, 5, 6, 6, 0});
    EQ(p.up_order, IV{4, 5, 6, 2, 3, 1, 0});
    EQ(h.up_class_off, IV{0, 3, 3, 3, 3, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7});
    EQ(h.up_level_off, IV{0, 3, 5, 6, 7});
    EQ(p.down_order, IV{0, 1, 2, 3, 4, 5, 6});
    EQ(h.down_level_off, IV{0, 1, 2, 4, 7});
    EQ(p.leaf_down, IV{7, 2, 0, 1, 3, 4, 5, 6});
    EQ(h.leaf_level_off, IV{0, 0, 1, 1, 2, 8});
    EQ(p.child_enc_v, IV{1, -8, 3, 2, 4 | VB, -3, 5 | VB, 6 | VB, -1, -2, -4, -5, -6, -7});
    EQ(p.child_enc_k, IV{1, -8, 3 | VB | S3, 2 | VB | S2, 4 | VB, -3, 5 | VB, 6 | VB, -1, -2, -4, -5, -6, -7});
    EQ(p.vleaf, cat({IV(8, -1), abc, defg, ab, de, fg}));
    EQ(p.vinner, IV{-1, -1, -1, -1, 4, -1, 5, 6, -1, -1, -1, -1, -1, -1});
    EQ(h.sshape, BV{0, 0, 1, 2, 0, 0, 0});
    EQ(p.up_order_v, IV{2, 3, 1, 0});
    EQ(h.up_class_off_v, IV{0, 0, 0, 0, 0, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4});
    EQ(h.up_level_off_v, IV{0, 0, 2, 3, 4});
    EQ(h.up_leafy_v, BV{1, 1, 0, 0});
    EQ(p.down_order_v, IV{0, 1, 2, 3});
    EQ(h.down_level_off_v, IV{0, 1, 2, 4, 4});
    EQ(h.up_class_off_k, IV{0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2});
    EQ(h.up_level_off_k, IV{0, 0, 0, 1, 2});
    EQ(h.up_leafy_k, BV{1, 1, 1, 0});
    EQ(h.down_level_off_k, IV{0, 1, 2, 2, 2});
    EQ(h.down_dense_base_k, IV{0, 1, -1, -1});
    CHECK(h.down_dense_v && h.down_dense_k);
    CHECK(h.cl.items.empty() && h.cl.wg_off.empty() && h.cl.band_wg.empty() && !h.cl.down && h.cl.upm_base == 2);
    EQ(p.up_desc, std::vector<NodeDesc>{ND(4, 2, 8, 10, -1, -2, 0, 0), ND(5, 3, 10, 12, -4, -5, 0, 0),
                                        ND(6, 3, 12, 14, -6, -7, 0, 0), ND(2, 1, 4, 6, 4, -3, 0, 0),
                                        ND(3, 1, 6, 8, 5, 6, 0, 0), ND(1, 0, 2, 4, 3, 2, 0, 0), ND(0, -1, 0, 2, 1, -8, 0, 0)});
    EQ(p.up_desc_v, std::vector<NodeDesc>{ND(2, 1, 4, 6, 4 | VB, -3, 0, 0, ab), ND(3, 1, 6, 8, 5 | VB, 6 | VB, 0, 0, de, fg),
                                          ND(1, 0, 2, 4, 3, 2, 0, 0), ND(0, -1, 0, 2, 1, -8, 0, 0)});
    EQ(p.up_desc_k, std::vector<NodeDesc>{ND(1, 0, 2, 4, 3 | VB | S3, 2 | VB | S2, 0, 0, defg, abc), ND(0, -1, 0, 2, 1, -8, 0, 0)});
    // the root joins its child's launch and recomputes it (item 0)
    const std::vector<NodeDesc> grouped = {ND(1, 0, 2, 4, 3 | VB | S3, 2 | VB | S2, -1, -1, defg, abc), ND(0, -1, 0, 2, 1, -8, 0, -1)};
    EQ(p.up_desc_g, grouped);
    EQ(p.up_desc_gs, grouped);
    for (int s = 0; s < 2; ++s) {
        EQ(s ? h.up_level_off_gs : h.up_level_off_g, IV{0, 2});
        EQ(s ? h.up_class_off_gs : h.up_class_off_g, IV{0, 2, 2, 2, 2});
        EQ(s ? h.up_leafy_gs : h.up_leafy_g, BV{0});
        EQ(s ? h.up_recomp_gs : h.up_recomp_g, BV{1});
        EQ(s ? h.up_plain_gs : h.up_plain_g, IV{0});
    }
    CHECK(h.up_items_k == 2 && h.up_items_g == 2 && h.up_items_gs == 2);
    for (const IV* ps : {&p.pslot_k, &p.pslot_g, &p.pslot_gs, &p.pslot_kc, &p.pslot_gc}) EQ(*ps, IV{2, -1});
    CHECK(p.cl_pslot.empty());
    EQ(p.down_desc, std::vector<NodeDesc>{ND(0, -1, 0, 2, 1, -8, -1, -1), ND(1, 0, 2, 4, 3, 2, -1, -1), ND(2, 1, 4, 6, 4, -3, 0, -1),
                                          ND(3, 1, 6, 8, 5, 6, 0, -1), ND(4, 2, 8, 10, -1, -2, 1, 0),
                                          ND(5, 3, 10, 12, -4, -5, 1, 0), ND(6, 3, 12, 14, -6, -7, 1, 0)});
    EQ(p.down_desc_v, std::vector<NodeDesc>{ND(0, -1, 0, 2, 1, -8, -1, -1), ND(1, 0, 2, 4, 3, 2, -1, -1),
                                            ND(2, 1, 4, 6, 4 | VB, -3, 0, -1, ab), ND(3, 1, 6, 8, 5 | VB, 6 | VB, 0, -1, de, fg)});
    EQ(p.down_desc_ks, std::vector<NodeDesc>{ND(0, -1, 0, 2, 1, -8, -1, -1), ND(1, 0, 2, 4, 3 | VB | S3, 2 | VB | S2, -1, -1, defg, abc)});
    // the S nodes' parent keeps no child in the pre-order levels: the placeholder
    EQ(p.down_desc_k, std::vector<NodeDesc>{ND(0, -1, 0, 2, 1, -8, -1, -1), ND(1, 0, 0, 1, 0, 0, -1, -1)});
    CHECK(p.tail_desc.empty() && p.tail_desc_v.empty() && h.num_tail == 0 && h.num_tail_v == 0);
    CHECK(h.num_tail_s == 2 && h.num_tail_k == 2);
    EQ(p.tail_desc_k, std::vector<TailDesc>{TD(1, 2 | VB | S2, 8, -1, abc, {11, 0, 1, 2, -1}), TD(1, 3 | VB | S3, 9, 10, defg, {12, 3, 4, 5, 6})});
    EQ(h.part_off, IV(8, 0));
    EQ(h.part_off_v, IV(5, 0));
    EQ(h.part_off_k, IV(3, 0));
    EQ(h.part_off_gs, IV(3, 0));
    EQ(h.up_degree[0], IV(7, 2));
    EQ(h.up_degree[1], IV(4, 2));
    EQ(h.up_degree[2], IV(2, 2));
    EQ(h.up_degree[3], IV(2, 2));
    CHECK(p.part_desc.empty() && p.part_desc_v.empty() && p.part_desc_k.empty() && p.part_desc_gs.empty());
    EQ(p.lvl, cat({h.up_class_off, h.down_level_off, h.up_class_off_v, h.down_level_off_v, h.up_class_off_k,
                   h.down_level_off_k, h.up_class_off_g, h.up_class_off_gs, h.down_dense_base_k}));
    const int64_t up[5] = {0, 22, 44, 66, 71}, down[3] = {17, 39, 61};
    CHECK(std::equal(up, up + 5, h.lvl_up) && std::equal(down, down + 3, h.lvl_down) && h.lvl_base_k == 76);
}

// (l0, l1, l2, (l3,l4), (l5,l6,l7)): leaves 0..7, the cherry 8, the three-leaf node 9, the root 10.
// No sweeps.
void hand_polytomy() {
    g_where = "hand (l0,l1,l2,(l3,l4),(l5,l6,l7))";
    Tree t;
    t.n = 11, t.root = 10;
    t.off = {0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 10};
    t.idx = {3, 4, 5, 6, 7, 0, 1, 2, 8, 9};
    const TreePlan p = plan_of(t, kSettings[3]);
    const HostTree& h = p.ht;
    const IV l34 = {3, 4, -1, -1}, none = {-1, -1, -1, -1};
    EQ(h.internal_id, IV{10, 9, 8});
    EQ(h.leaf_id, IV{0, 1, 2, 3, 4, 5, 6, 7});
    EQ(h.child_off, IV{0, 5, 8, 10});
    // heavy child first: the three-leaf node (dense 1) swapped with l0 at the front
    EQ(h.child_enc, IV{1, -2, -3, 2, -1, -6, -7, -8, -4, -5});
    EQ(p.parent_dense, IV{-1, 0, 0});
    EQ(p.leaf_parent, IV{0, 0, 0, 2, 2, 1, 1, 1});
    // the root (out-degree 5) is of degree class 1
    EQ(p.up_order, IV{1, 2, 0});
    EQ(h.up_class_off, IV{0, 2, 2, 2, 2, 2, 3, 3, 3});
    EQ(h.up_level_off, IV{0, 2, 3});
    EQ(p.down_order, IV{0, 1, 2});
    EQ(h.down_level_off, IV{0, 1, 3});
    EQ(p.leaf_down, IV{0, 1, 2, 3, 4, 5, 6, 7});
    EQ(h.leaf_level_off, IV{0, 0, 3, 8});
    CHECK(h.num_virtual == 1 && h.num_sshape == 0 && h.sbase == -1);
    EQ(p.child_enc_v, IV{1, -2, -3, 2 | VB, -1, -6, -7, -8, -4, -5});
    EQ(p.child_enc_k, p.child_enc_v);
    EQ(p.vleaf, cat({IV(8, -1), l34}));
    EQ(p.vinner, IV(6, -1));
    EQ(h.sshape, BV{0, 0, 0});
    EQ(p.up_order_v, IV{1, 0});
    for (const IV* c : {&h.up_class_off_v, &h.up_class_off_k, &h.up_class_off_g, &h.up_class_off_gs}) EQ(*c, IV{0, 1, 1, 1, 1, 1, 2, 2, 2});
    for (const IV* c : {&h.up_level_off_v, &h.up_level_off_k, &h.up_level_off_g, &h.up_level_off_gs}) EQ(*c, IV{0, 1, 2});
    for (const BV* c : {&h.up_leafy_v, &h.up_leafy_k, &h.up_leafy_g, &h.up_leafy_gs}) EQ(*c, BV{1, 1});
    EQ(h.up_recomp_g, BV{0, 0});
    EQ(h.up_recomp_gs, BV{0, 0});
    EQ(h.up_plain_g, IV{0, 0});   // (three children, five children: neither node is plain)
    EQ(h.up_plain_gs, IV{0, 0});
    EQ(p.down_order_v, IV{0, 1});
    EQ(h.down_level_off_v, IV{0, 1, 2});
    EQ(h.down_level_off_k, IV{0, 1, 2});
    EQ(h.down_dense_base_k, IV{0, 1});
    CHECK(h.down_dense_v && h.down_dense_k && h.cl.items.empty() && !h.cl.down && h.cl.upm_base == 2);
    EQ(p.up_desc, std::vector<NodeDesc>{ND(1, 0, 5, 8, -6, -7, 0, 0), ND(2, 0, 8, 10, -4, -5, 0, 0), ND(0, -1, 0, 5, 1, -2, 0, 0)});
    const std::vector<NodeDesc> up_v = {ND(1, 0, 5, 8, -6, -7, 0, 0), ND(0, -1, 0, 5, 1, -2, 0, 0)};
    EQ(p.up_desc_v, up_v);
    EQ(p.up_desc_k, up_v);
    const std::vector<NodeDesc> levels = {ND(1, 0, 5, 8, -6, -7, -1, -1), ND(0, -1, 0, 5, 1, -2, -1, -1)};
    EQ(p.up_desc_g, levels);   // the root, of out-degree 5, takes the launch after its child's
    EQ(p.up_desc_gs, levels);
    CHECK(h.up_items_k == 2 && h.up_items_g == 2 && h.up_items_gs == 2);
    for (const IV* ps : {&p.pslot_k, &p.pslot_g, &p.pslot_gs, &p.pslot_kc, &p.pslot_gc}) EQ(*ps, IV{2, -1});
    EQ(p.down_desc, std::vector<NodeDesc>{ND(0, -1, 0, 5, 1, -2, -1, -1), ND(1, 0, 5, 8, -6, -7, -1, -1), ND(2, 0, 8, 10, -4, -5, -1, -1)});
    const std::vector<NodeDesc> down_v = {ND(0, -1, 0, 5, 1, -2, -1, -1), ND(1, 0, 5, 8, -6, -7, -1, -1)};
    EQ(p.down_desc_v, down_v);
    EQ(p.down_desc_k, down_v);
    EQ(p.down_desc_ks, down_v);
    // tails: the root's children beyond the first two that are leaves (l2, l0) or, in the leaf-parent
    // form, the cherry as well; and the three-leaf node's third leaf
    CHECK(h.num_tail == 3 && h.num_tail_v == 4 && h.num_tail_k == 4 && h.num_tail_s == 0);
    EQ(p.tail_desc, std::vector<TailDesc>{TD(0, -3, -1, -1, none, {2, -1, -1, -1, -1}), TD(0, -1, -1, -1, none, {0, -1, -1, -1, -1}),
                                          TD(1, -8, -1, -1, none, {7, -1, -1, -1, -1})});
    const std::vector<TailDesc> tail_v = {TD(0, -3, -1, -1, none, {2, -1, -1, -1, -1}), TD(0, 2 | VB, -1, -1, l34, {8, 3, 4, -1, -1}),
                                          TD(0, -1, -1, -1, none, {0, -1, -1, -1, -1}), TD(1, -8, -1, -1, none, {7, -1, -1, -1, -1})};
    EQ(p.tail_desc_v, tail_v);
    EQ(p.tail_desc_k, tail_v);
    EQ(h.part_off, IV(4, 0));
    EQ(h.part_off_v, IV(3, 0));
    EQ(h.part_off_k, IV(3, 0));
    EQ(h.part_off_gs, IV(3, 0));
    EQ(h.up_degree[0], IV{3, 2, 5});
    for (int v = 1; v < 4; ++v) EQ(h.up_degree[v], IV{3, 5});
    CHECK(p.part_desc.empty() && p.part_desc_v.empty() && p.part_desc_k.empty() && p.part_desc_gs.empty());
    EQ(p.lvl, cat({h.up_class_off, h.down_level_off, h.up_class_off_v, h.down_level_off_v, h.up_class_off_k,
                   h.down_level_off_k, h.up_class_off_g, h.up_class_off_gs, h.down_dense_base_k}));
    const int64_t up[5] = {0, 12, 24, 36, 45}, down[3] = {9, 21, 33};
    CHECK(std::equal(up, up + 5, h.lvl_up) && std::equal(down, down + 3, h.lvl_down) && h.lvl_base_k == 54);
}

// ---- argument errors ------------------------------------------------------------------------
void expect_error(const char* what, int32_t n, int32_t root, IV off, IV idx, const char* text) {
    g_where = std::string("error: ") + what;
    pm_tree t{};
    t.num_nodes = n, t.root = root, t.child_offsets = off.data(), t.child_index = idx.data();
    TreePlan p;
    std::string err;
    const int rc = plan_tree(t, kClMaxLevel, true, p, err);
    CHECK(rc == PM_ERR_ARG);
    CHECK(err == text);
}

void errors() {
    expect_error("fewer than 2 nodes", 1, 0, {0, 0}, {0}, "bad tree");
    expect_error("bad header (first offset)", 3, 2, {1, 1, 1, 3}, {0, 1, 0}, "bad tree header");
    expect_error("bad header (root)", 3, 3, {0, 0, 0, 2}, {0, 1}, "bad tree header");
    expect_error("non-monotone offsets", 3, 2, {0, 2, 1, 2}, {0, 1}, "child offsets not monotone");
    expect_error("E != N - 1", 3, 2, {0, 0, 0, 1}, {0}, "a tree on N nodes has N-1 edges");
    expect_error("repeated child", 3, 2, {0, 0, 0, 2}, {0, 0}, "child index invalid or repeated");
    expect_error("child out of range", 3, 2, {0, 0, 0, 2}, {0, 3}, "child index invalid or repeated");
    expect_error("leaf root", 3, 0, {0, 0, 2, 2}, {2, 1}, "root must be internal");
    expect_error("unreachable 2-cycle", 4, 0, {0, 1, 1, 2, 3}, {1, 3, 2}, "tree is not connected");
    {
        g_where = "error: no offsets";
        pm_tree t{};
        t.num_nodes = 3;
        TreePlan p;
        std::string err;
        CHECK(plan_tree(t, 0, false, p, err) == PM_ERR_ARG && err == "bad tree");
    }
}

}  // namespace

int main(int argc, char** argv) {
    bool want_digest = false;
    std::vector<Tree> trees;
    for (int a = 1; a < argc; ++a) {
        if (!std::strcmp(argv[a], "--digest")) {
            want_digest = true;
            continue;
        }
        Tree t;
        if (!read_tree(argv[a], t)) {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        trees.push_back(std::move(t));
    }
    trees.push_back(generated("gen:random_join", false, 20000));
    trees.push_back(generated("gen:sars_like", true, 20000));
    if (!want_digest) {
        hand_cherry();
        hand_shapes();
        hand_polytomy();
        errors();
    }
    int pairs = 0;
    for (const Tree& t : trees)
        for (int s = 0; s < 4; ++s, ++pairs) {
            g_where = t.name + " setting " + std::to_string(s);
            const TreePlan p = plan_of(t, kSettings[s]);
            if (want_digest) {
                std::printf("== %s setting %d\n", t.name.c_str(), s);
                digest(p);
            } else {
                check_plan(t, p);
            }
        }
    if (g_failed) {
        std::fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    if (!want_digest) std::printf("plan_host_check: %zu trees x 4 settings = %d plans ok\n", trees.size(), pairs);
    return 0;
}
