// schedule_host_check.cpp -- the launch schedule of a pm_run (panman_amd/csrc/pm_schedule.cpp over
// the planner) without a GPU: the hand-written step lists of the three tiny trees
// plan_host_check.cpp plans by hand, and the schedule's invariants over the trees given on the
// command line under every configuration, mode, tile count and leaf presence.  Built and run by
// tests/test_schedule_host.py under ASan / UBSan.
//
//   schedule_host_check CONFIGS TREE...
//     CONFIGS: lines "name cluster narrow group_waves group_levels up_group plain_up sub_down tail_pack
//              down_pack subtree virtual", the values as pm_set_option takes them
//     TREE:    a text file "N root n_off n_idx", the offsets, the indices
//
// Prints per (tree, configuration) one line "counts tree|name" followed, for 2 tiles then 1 tile,
// every leaf present then not, modes 0..3, by the timer spans of classes 0, 1, 5 and the run.* phase
// values (-1: the mode logs none), and at the end "kinds" with every step kind it met.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../panman_amd/csrc/pm_schedule.h"

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

struct Tree {
    std::string name;
    int32_t n = 0, root = 0;
    std::vector<int32_t> off, idx;
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
    const size_t dot = t.name.rfind(".tree");
    if (dot != std::string::npos) t.name.resize(dot);
    return (bool)in;
}

TreePlan plan_of(const Tree& t, int64_t cluster) {   // (PM_OPT_CLUSTER as pm_set_option reads it)
    pm_tree v{};
    v.num_nodes = t.n;
    v.root = t.root;
    v.child_offsets = t.off.data();
    v.child_index = t.idx.data();
    TreePlan p;
    std::string err;
    const int rc = plan_tree(v, cluster == 0 ? 0 : cluster == 1 ? kClMaxLevel : (int32_t)cluster, cluster == 1, p, err);
    CHECK(rc == PM_OK && err.empty());
    return p;
}

struct Config {
    std::string name;
    int64_t v[11];
};

RunOpts opts_of(const Config& c, bool all_present, int tiles) {
    RunOpts o;
    o.cluster = c.v[0] != 0;
    o.narrow_max = c.v[1];
    o.group_waves = c.v[2];
    o.group_levels = c.v[3];
    o.up_group = c.v[4];
    o.plain_up = c.v[5] != 0;
    o.plain_min_waves = c.v[5] >= 2 ? c.v[5] : 0;
    o.sub_down = c.v[6];
    o.tail_pack = c.v[7] != 0;
    o.tail_pack_min_waves = c.v[7] >= 2 ? c.v[7] : c.v[7] < 0 ? -1 : 0;
    o.down_pack = c.v[8] != 0;
    o.down_pack_min_waves = c.v[8] >= 2 ? c.v[8] : c.v[8] < 0 ? -1 : 0;
    o.subtree_form = c.v[9];
    o.virtual_leaf_parents = c.v[10];
    o.nt_loads = -1;
    o.leaves_all_present = all_present;
    o.tiles = tiles;
    return o;
}

bool g_seen[(int)StepKind::kCount];

const char* step_name(StepKind k) {
    static const char* const names[] = {"fork", "join", "span", "up_band", "up_mixed", "up_wide", "up_narrow", "up_sweep", "up_parts",
                                        "up_merge", "down_sweep", "down_band", "down_level", "down_group", "down_packed",
                                        "tail", "tail_packed"};
    return k < StepKind::kCount ? names[(int)k] : "?";
}

bool is_up(StepKind k) { return k >= StepKind::kUpBand && k <= StepKind::kUpMerge; }
bool is_level(StepKind k) { return k == StepKind::kDownBand || k == StepKind::kDownLevel || k == StepKind::kDownGroup || k == StepKind::kDownPacked; }

// The invariants of one schedule; returns its counts (spans of classes 0, 1, 5, then the phase values).
std::vector<int64_t> check_schedule(const HostTree& ht, const RunOpts& o, int mode) {
    const Schedule s = schedule_run(ht, o, mode);
    const RunPaths& p = s.paths;
    const RunForm f = run_form(ht, p);
    const int32_t tiles = (int32_t)o.tiles;
    const ClusterPlan& cl = ht.cl;
    const std::vector<int32_t>&co = *f.up_class_off, &down = *f.down_level_off;
    CHECK(s.first_down <= s.steps.size());
    CHECK(p.sankoff == (mode == PM_MODE_SANKOFF || mode == PM_MODE_BLOCK_SANKOFF));
    CHECK(!p.sub || (p.virt && p.ap && !p.block));
    CHECK((!p.clu && !p.cld && !p.grp && !p.sub_down) || p.sub);

    // post-order: the levels below H by steps, the heights from cl.h0 by the sweeps' bands
    const int H = p.clu && (p.sankoff || !p.grp) ? cl.h0 : (int)f.up_level_off->size() - 1;
    std::vector<int> up_cover(H > 0 ? co[(size_t)H * kDegreeClasses] : 0, 0), down_cover(down.size() - 1, 0), tail_cover(f.num_tail, 0);
    int64_t spans[6] = {0, 0, 0, 0, 0, 0};   // by timer class (the library's kClasses)
    int open_cls = -1, fork_h = -1, last_up = 0, last_down = 0, packed = 0, tail_packed = 0;
    std::vector<size_t> up_bands, down_bands;
    bool tail_seen = false;
    const int D = p.cld ? 0 : (int)down.size() - 1;
    auto narrow = [&](int l) { return o.narrow_max > 0 && down[l + 1] - down[l] <= o.narrow_max; };
    for (size_t i = 0; i < s.steps.size(); ++i) {
        const Step& st = s.steps[i];
        const StepKind k = st.kind;
        CHECK(k < StepKind::kCount);
        if (k >= StepKind::kCount) continue;
        g_seen[(int)k] = true;
        CHECK((i < s.first_down) == (is_up(k) || k <= StepKind::kSpan));
        // timer spans: open and close alternate within one class
        if (st.timer_open) {
            CHECK(open_cls < 0);
            open_cls = st.cls;
        }
        if (st.timer_close) {
            CHECK(open_cls == st.cls);
            open_cls = -1;
            CHECK(st.cls == 0 || st.cls == 1 || st.cls == 5);
            ++spans[st.cls];
        }
        CHECK(st.cls == (is_up(k) || k <= StepKind::kSpan ? 0 : k >= StepKind::kTail ? 5 : 1));
        if (k == StepKind::kFork) {   // every fork has its join before the next level
            CHECK(fork_h < 0);
            fork_h = st.h0;
            continue;
        }
        if (k == StepKind::kJoin) {
            CHECK(fork_h == st.h0);
            fork_h = -1;
            continue;
        }
        if (k == StepKind::kSpan) {   // Sankoff's empty span before the parts of a level it does not mix
            CHECK(p.sankoff && st.timer_open && st.timer_close && i + 1 < s.steps.size() && s.steps[i + 1].kind == StepKind::kUpParts);
            continue;
        }
        CHECK(st.count > 0);
        CHECK(!st.side || fork_h >= 0);
        if (fork_h >= 0) CHECK(st.h0 == fork_h && st.h1 == fork_h + 1);
        const uint32_t wave = wave_grid_x(st.count, tiles), block = block_grid_x(st.count, tiles);
        switch (k) {
        case StepKind::kUpSweep:
        case StepKind::kDownSweep: {
            CHECK(k == StepKind::kUpSweep ? p.clu : p.cld);
            size_t bnd = 0;   // the band of these clusters
            while (bnd + 1 < cl.band_wg.size() && !(cl.band_wg[bnd] == st.first && cl.band_wg[bnd + 1] == st.first + st.count)) ++bnd;
            CHECK(bnd + 1 < cl.band_wg.size());
            if (bnd + 1 < cl.band_wg.size()) CHECK(st.h0 == cl.band_level[bnd] && st.h1 == cl.band_level[bnd + 1]);
            CHECK(st.grid_x == (uint32_t)(st.count * tiles));   // one wave per (cluster, tile), on one grid axis
            (k == StepKind::kUpSweep ? up_bands : down_bands).push_back(bnd);
            break;
        }
        case StepKind::kUpBand:
            CHECK(st.h0 < st.h1 - 1 && st.h1 <= H && st.first == st.h0 && st.count == st.h1 - st.h0 && st.grid_x == (uint32_t)tiles);
            for (int32_t j = co[st.h0 * kDegreeClasses]; j < co[st.h1 * kDegreeClasses]; ++j) ++up_cover[j];
            break;
        case StepKind::kUpMixed:
            CHECK(st.count2 > 0 && st.grid_x == wave + (uint32_t)(st.count2 * tiles));   // (blocks on one grid axis)
            CHECK(p.sankoff ? st.variant == 4 || st.variant == 8 : st.variant == 0);
            for (int32_t j = st.first; j < st.first + st.count + st.count2; ++j) ++up_cover.at(j);
            break;
        case StepKind::kUpWide:
        case StepKind::kUpNarrow:
        case StepKind::kUpMerge:
            CHECK(st.grid_x == (k == StepKind::kUpWide ? block : wave));
            if (k == StepKind::kUpNarrow) CHECK(st.first + st.count <= co[st.h0 * kDegreeClasses + 1] && st.first >= co[st.h0 * kDegreeClasses]);
            else CHECK(st.first >= co[st.h0 * kDegreeClasses + 1]);
            if (k == StepKind::kUpMerge) {   // behind its parts, in one span
                CHECK(p.sankoff && i > 0 && s.steps[i - 1].kind == StepKind::kUpParts && !st.timer_open && st.timer_close);
                CHECK(s.steps[i - 1].first == (*f.part_off)[st.first] &&
                      s.steps[i - 1].count == (*f.part_off)[st.first + st.count] - (*f.part_off)[st.first]);
                CHECK(st.variant == 16 || st.variant == 32);
            }
            for (int32_t j = st.first; j < st.first + st.count; ++j) ++up_cover.at(j);
            break;
        case StepKind::kUpParts:
            CHECK(st.grid_x == wave && st.timer_open && !st.timer_close);
            break;
        case StepKind::kDownBand:
        case StepKind::kDownLevel:
        case StepKind::kDownGroup:
        case StepKind::kDownPacked:
            CHECK(st.h0 >= last_down && st.h0 < st.h1 && st.h1 <= D);   // top-down, each level once
            last_down = st.h1;
            for (int l = st.h0; l < st.h1; ++l) ++down_cover[l];
            if (k == StepKind::kDownBand) {
                CHECK(st.h1 - st.h0 >= 2 && st.first == st.h0 && st.count == st.h1 - st.h0 && st.grid_x == (uint32_t)tiles);
                for (int l = st.h0; l < st.h1; ++l) CHECK(narrow(l));
                break;
            }
            CHECK(st.first == down[st.h0] && st.count == down[st.h1] - down[st.h0]);
            CHECK(st.dense_base == f.dense_base(st.h0));
            CHECK((k == StepKind::kDownGroup) == (st.h1 - st.h0 > 1));
            for (int l = st.h0; l < st.h1; ++l) {   // no group starts a band, none holds an empty level
                CHECK(!(narrow(l) && l + 1 < D && narrow(l + 1)));
                CHECK(down[l + 1] > down[l]);
            }
            if (k == StepKind::kDownGroup) {
                CHECK(st.h1 - st.h0 <= std::min<int64_t>(o.group_levels, kGroupLevels) && (int64_t)st.count * tiles <= o.group_waves);
                for (int g = 0; g < 4; ++g) {
                    const int l = std::min(st.h0 + g, st.h1 - 1);
                    CHECK(st.dense_g[g] == f.dense_base(l));
                    if (g > 0) CHECK(st.split[g - 1] == (st.h0 + g < st.h1 ? down[st.h0 + g] - down[st.h0] : st.count));
                }
            }
            if (k == StepKind::kDownPacked) {
                ++packed;
                CHECK(!p.sankoff && !p.block && p.ap && st.dense_base >= 0 && st.h0 > 0 && o.down_pack);
                CHECK(st.grid_x == wave_grid_x((st.count + kDownPack - 1) / kDownPack, tiles));
            } else {
                CHECK(st.grid_x == wave);
            }
            break;
        case StepKind::kTailPacked:   // the S2 / S3 items, before every other tail item
            ++tail_packed;
            CHECK(!tail_seen && !p.sankoff && p.sub && st.first == 0 && st.count == ht.num_tail_s);
            CHECK(st.grid_x == wave_grid_x((st.count + kTailPack - 1) / kTailPack, tiles));
            for (int32_t j = 0; j < st.count; ++j) ++tail_cover.at(j);
            break;
        case StepKind::kTail:
            tail_seen = true;
            CHECK(st.grid_x == wave && st.count2 == (p.sub && st.first == 0 ? ht.num_tail_s : 0));
            for (int32_t j = st.first; j < st.first + st.count; ++j) ++tail_cover.at(j);
            break;
        default:
            break;
        }
        if (is_up(k) && k != StepKind::kUpSweep) {   // heights never decrease along the stream
            CHECK(st.h0 >= last_up && st.h1 <= H);
            last_up = st.h0;
        }
    }
    CHECK(open_cls < 0 && fork_h < 0);
    for (int c : up_cover) CHECK(c == 1);
    // the sweeps: every band that holds a cluster, once, bottom-up (post-order) / top-down (pre-order)
    std::vector<size_t> bands;
    for (size_t b = 0; b + 1 < cl.band_wg.size(); ++b)
        if (cl.band_wg[b + 1] > cl.band_wg[b]) bands.push_back(b);
    CHECK(up_bands == (p.clu ? bands : std::vector<size_t>{}));
    std::reverse(bands.begin(), bands.end());
    CHECK(down_bands == (p.cld ? bands : std::vector<size_t>{}));
    for (int l = 0; l + 1 < (int)down.size(); ++l) CHECK(p.cld ? down_cover[l] == 0 : down[l + 1] > down[l] ? down_cover[l] == 1 : down_cover[l] <= 1);
    // every tail item in exactly one tail step (PM_OPT_SUB_DOWN: the levels did the S2 / S3 items)
    for (int32_t j = 0; j < f.num_tail; ++j) CHECK(tail_cover[j] == (p.sub_down && j < ht.num_tail_s ? 0 : 1));
    CHECK(s.packed_levels == packed && s.tail_pack == (tail_packed == 1) && tail_packed <= 1);
    CHECK(s.down_pack_ranges.size() % 2 == 0 && (int)s.down_pack_ranges.size() >= 2 * packed);
    std::vector<int64_t> out = {spans[0], spans[1], spans[5], p.nt ? 1 : 0};
    if (p.sankoff) out.insert(out.end(), {-1, -1, -1, -1});
    else out.insert(out.end(), {packed > 0 ? kDownPack : 0, packed, s.tail_pack ? kTailPack : 0, s.tail_s_waves});
    return out;
}

// ---- hand-written step lists (default options, every leaf present, one tile) ---------------------
struct Want {
    StepKind kind;
    int variant, cls, h0, h1, first, count, count2;
    uint32_t grid_x;
};

void hand(const char* where, int32_t n, int32_t root, std::vector<int32_t> off, std::vector<int32_t> idx, int mode,
          const std::vector<Want>& want, size_t first_down) {
    g_where = std::string("hand ") + where + (mode == PM_MODE_FITCH ? " fitch" : " sankoff");
    Tree t;
    t.n = n, t.root = root, t.off = std::move(off), t.idx = std::move(idx);
    const TreePlan p = plan_of(t, 1);
    const Config defaults = {"defaults", {1, 16, 32768, 4, 1, 1, 0, 1, 1, 1, 1}};
    const Schedule s = schedule_run(p.ht, opts_of(defaults, true, 1), mode);
    CHECK(s.steps.size() == want.size() && s.first_down == first_down);
    for (size_t i = 0; i < std::min(s.steps.size(), want.size()); ++i) {
        const Step& g = s.steps[i];
        const Want& w = want[i];
        const bool same = g.kind == w.kind && g.variant == w.variant && g.cls == w.cls && g.h0 == w.h0 && g.h1 == w.h1 &&
                          g.first == w.first && g.count == w.count && g.count2 == w.count2 && g.grid_x == w.grid_x && !g.side &&
                          g.timer_open && g.timer_close;   // (no fork in these trees: every launch its own span)
        if (!same)
            std::fprintf(stderr, "%s: step %zu is %s variant %d cls %d levels [%d, %d) items [%d, +%d) count2 %d grid %u\n",
                         g_where.c_str(), i, step_name(g.kind), g.variant, g.cls, g.h0, g.h1, g.first, g.count, g.count2, g.grid_x);
        CHECK(same);
    }
    CHECK(!s.tail_pack && s.packed_levels == 0 && s.down_pack_ranges.empty() && !s.paths.nt);
}

void hand_lists() {
    using K = StepKind;
    // ((a,b),c): the cherry is evaluated inline, so the leaf-parent form holds the root alone (an empty
    // level below it); no S2 / S3 node, so no subtree form and no sweeps.  Two narrow levels: one band
    // per pass, in both modes; no child beyond a second: no tail.
    for (int mode : {PM_MODE_FITCH, PM_MODE_SANKOFF})
        hand("((a,b),c)", 5, 4, {0, 0, 0, 0, 2, 4}, {0, 1, 3, 2}, mode,
             {{K::kUpBand, 0, 0, 0, 2, 0, 2, 0, 1}, {K::kDownBand, 1, 1, 0, 2, 0, 2, 0, 1}}, 1);
    // ((((a,b),c),((d,e),(f,g))),h): the subtree form holds the root and the parent of the S2 and S3
    // nodes, heights 4 and 3; the default plan sweeps them as one cluster (one band over the four
    // heights), post-order and pre-order, in both modes (no node above 255 children); the tail holds
    // the two S nodes (2 waves: below the packing threshold).
    for (int mode : {PM_MODE_FITCH, PM_MODE_SANKOFF})
        hand("((((a,b),c),((d,e),(f,g))),h)", 15, 14, {0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 4, 6, 8, 10, 12, 14},
             {0, 1, 3, 4, 5, 6, 8, 2, 9, 10, 11, 12, 13, 7}, mode,
             {{K::kUpSweep, 0, 0, 0, 4, 0, 1, 0, 1}, {K::kDownSweep, 0, 1, 0, 4, 0, 1, 0, 1}, {K::kTail, 0, 5, 0, 0, 0, 2, 2, 1}}, 1);
    // (l0,l1,l2,(l3,l4),(l5,l6,l7)): the leaf-parent form holds the three-leaf node (height 1, narrow)
    // and the root (height 2, five children: wide).  Fitch walks both levels in one band (1 + 4 * 1
    // node-equivalents <= 16); Sankoff's bands take narrow nodes only, so one launch per level, the
    // root's with 4-bit counters.  The pre-order: two levels of one node, one band.  The tail: the
    // root's children beyond its second (two leaves, the cherry) and the three-leaf node's third.
    const std::vector<int32_t> off = {0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 10}, idx = {3, 4, 5, 6, 7, 0, 1, 2, 8, 9};
    hand("(l0,l1,l2,(l3,l4),(l5,l6,l7))", 11, 10, off, idx, PM_MODE_FITCH,
         {{K::kUpBand, 0, 0, 0, 2, 0, 2, 0, 1}, {K::kDownBand, 1, 1, 0, 2, 0, 2, 0, 1}, {K::kTail, 0, 5, 2, 2, 0, 4, 0, 1}}, 1);
    hand("(l0,l1,l2,(l3,l4),(l5,l6,l7))", 11, 10, off, idx, PM_MODE_SANKOFF,
         {{K::kUpNarrow, kNarrowBase, 0, 0, 1, 0, 1, 0, 1}, {K::kUpWide, 4, 0, 1, 2, 1, 1, 0, 1},
          {K::kDownBand, 1, 1, 0, 2, 0, 2, 0, 1}, {K::kTail, 0, 5, 2, 2, 0, 4, 0, 1}}, 2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: schedule_host_check CONFIGS TREE...\n");
        return 2;
    }
    std::vector<Config> configs;
    {
        std::ifstream in(argv[1]);
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            Config c;
            if (!(ls >> c.name)) continue;
            for (auto& v : c.v) ls >> v;
            if (!ls) return 2;
            configs.push_back(c);
        }
    }
    hand_lists();
    for (int a = 2; a < argc; ++a) {
        Tree t;
        if (!read_tree(argv[a], t)) {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        std::map<int64_t, TreePlan> plans;   // by PM_OPT_CLUSTER
        for (const Config& c : configs) {
            g_where = t.name + "|" + c.name;
            if (!plans.count(c.v[0])) plans[c.v[0]] = plan_of(t, c.v[0]);
            const HostTree& ht = plans[c.v[0]].ht;
            std::printf("counts %s", g_where.c_str());
            for (int tiles : {2, 1})
                for (bool present : {true, false})
                    for (int mode = PM_MODE_FITCH; mode <= PM_MODE_BLOCK_SANKOFF; ++mode)
                        for (int64_t v : check_schedule(ht, opts_of(c, present, tiles), mode)) std::printf(" %lld", (long long)v);
            std::printf("\n");
        }
    }
    std::printf("kinds");
    for (int k = 0; k < (int)StepKind::kCount; ++k)
        if (g_seen[k]) std::printf(" %s", step_name((StepKind)k));
    std::printf("\n");
    if (g_failed) std::fprintf(stderr, "%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
