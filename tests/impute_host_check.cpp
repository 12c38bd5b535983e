// impute_host_check.cpp -- the host plan of pm_impute (panman_amd/csrc/pm_impute_plan.cpp) as a stand-alone
// program: tests/test_impute_host.py builds it with g++ under AddressSanitizer and UBSan and runs it.
//   impute_host_check CASE...   every case file (written by the test from tests/_impute_cases.py) is planned
//                               and its attempts, candidates in walk order and winners compared with the lines
//                               the file carries; then the built-in checks: the path steps and block folds of
//                               the seven-node tree, the winner rule, every argument error.
// Case file: "N root D has_lengths", the child offsets, the child indices, the lengths (if any), "B n" and n
// lines "node block insertion inversion", "M n" and n lines "node block position gap info nucs", "A n" and n
// lines "node candidates... | nuc improvements... | winner-or--1" (node ids).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../panman_amd/csrc/pm_impute_plan.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond << "\n";     \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

struct Mat {   // owns what a pm_panmat points into
    std::vector<int32_t> off, idx;
    std::string names;
    std::vector<float> length;
    std::vector<int64_t> bm_off, nm_off;
    std::vector<int32_t> bm_primary, nm_primary, nm_secondary, nm_pos, nm_gap;
    std::vector<uint8_t> bm_info, bm_inv, nm_info;
    std::vector<uint32_t> nm_nucs;
    std::vector<int32_t> block_primary{0, 1};
    pm_panmat p{};
    Mat() = default;
    Mat(const Mat&) = delete;   // (p points into the object)

    struct B {
        int32_t node, primary, info, inv;
    };
    struct M {
        int32_t node, primary, pos, gap, info;
        uint32_t nucs;
    };
    void build(int32_t n, int32_t root, const std::vector<B>& bs, const std::vector<M>& ms) {
        names.clear();
        for (int32_t v = 0; v < n; ++v) names += "n" + std::to_string(v) + '\0';
        bm_off.assign(1, 0);
        nm_off.assign(1, 0);
        for (int32_t v = 0; v < n; ++v) {
            for (const B& b : bs)
                if (b.node == v) {
                    bm_primary.push_back(b.primary);
                    bm_info.push_back((uint8_t)b.info);
                    bm_inv.push_back((uint8_t)b.inv);
                }
            for (const M& m : ms)
                if (m.node == v) {
                    nm_primary.push_back(m.primary);
                    nm_secondary.push_back(-1);
                    nm_pos.push_back(m.pos);
                    nm_gap.push_back(m.gap);
                    nm_info.push_back((uint8_t)m.info);
                    nm_nucs.push_back(m.nucs);
                }
            bm_off.push_back((int64_t)bm_primary.size());
            nm_off.push_back((int64_t)nm_primary.size());
        }
        // (never null, also when empty)
        bm_primary.push_back(0), bm_info.push_back(0), bm_inv.push_back(0);
        nm_primary.push_back(0), nm_secondary.push_back(-1), nm_pos.push_back(0), nm_gap.push_back(-1), nm_info.push_back(0), nm_nucs.push_back(0);
        p = pm_panmat{};
        p.num_nodes = n;
        p.root = root;
        p.child_offsets = off.data();
        p.child_index = idx.data();
        p.names = names.data();
        p.num_blocks = 2;
        p.block_primary = block_primary.data();
        p.block_mut_offsets = bm_off.data();
        p.block_mut_primary = bm_primary.data();
        p.block_mut_info = bm_info.data();
        p.block_mut_inversion = bm_inv.data();
        p.nuc_mut_offsets = nm_off.data();
        p.nuc_mut_primary = nm_primary.data();
        p.nuc_mut_secondary = nm_secondary.data();
        p.nuc_mut_position = nm_pos.data();
        p.nuc_mut_gap_position = nm_gap.data();
        p.nuc_mut_info = nm_info.data();
        p.nuc_mut_nucs = nm_nucs.data();
        p.branch_length = length.empty() ? nullptr : length.data();
    }
};

std::vector<long long> numbers(const std::string& s) {
    std::vector<long long> v;
    std::istringstream in(s);
    long long x;
    while (in >> x) v.push_back(x);
    return v;
}

void check_case(const std::string& path) {
    std::ifstream in(path);
    if (!in) {
        std::cerr << "cannot read " << path << "\n";
        ++failures;
        return;
    }
    int32_t n, root, distance, has_lengths;
    in >> n >> root >> distance >> has_lengths;
    Mat m;
    m.off.resize((size_t)n + 1);
    for (auto& x : m.off) in >> x;
    m.idx.resize((size_t)n - 1);
    for (auto& x : m.idx) in >> x;
    if (has_lengths) {
        m.length.resize((size_t)n);
        for (auto& x : m.length) in >> x;
    }
    std::string tag;
    size_t count;
    std::vector<Mat::B> bs;
    std::vector<Mat::M> ms;
    in >> tag >> count;
    for (size_t i = 0; i < count; ++i) {
        Mat::B b;
        in >> b.node >> b.primary >> b.info >> b.inv;
        bs.push_back(b);
    }
    in >> tag >> count;
    for (size_t i = 0; i < count; ++i) {
        Mat::M r;
        in >> r.node >> r.primary >> r.pos >> r.gap >> r.info >> r.nucs;
        ms.push_back(r);
    }
    m.build(n, root, bs, ms);
    std::string err;
    pm::ImputePlan plan;
    CHECK(pm::impute_check(&m.p, err) == PM_OK);
    CHECK(pm::impute_plan(&m.p, distance, plan, err) == PM_OK);
    in >> tag >> count;
    std::string line;
    std::getline(in, line);
    if (plan.attempts.size() != count) {
        std::cerr << path << ": " << plan.attempts.size() << " attempts, expected " << count << "\n";
        ++failures;
        return;
    }
    for (size_t a = 0; a < count; ++a) {
        std::getline(in, line);
        const size_t bar1 = line.find('|'), bar2 = line.find('|', bar1 + 1);
        const std::vector<long long> head = numbers(line.substr(0, bar1)), nuc = numbers(line.substr(bar1 + 1, bar2 - bar1 - 1)),
                                     win = numbers(line.substr(bar2 + 1));
        const pm::ImputeAttempt& at = plan.attempts[a];
        bool same = at.node == head[0] && (size_t)(at.pair1 - at.pair0) == head.size() - 1 && nuc.size() == head.size() - 1;
        for (size_t k = 1; same && k < head.size(); ++k) same = plan.pairs[(size_t)at.pair0 + k - 1].candidate == head[k];
        if (!same) {
            std::cerr << path << ": attempt " << a << " (node " << at.node << ") has other candidates than \"" << line << "\"\n";
            ++failures;
            continue;
        }
        std::vector<int64_t> improvement(nuc.begin(), nuc.end());
        const int64_t best = pm::impute_winner(improvement.data(), plan.pairs.data() + at.pair0, at.pair1 - at.pair0);
        const long long winner = best < 0 ? -1 : plan.pairs[(size_t)(at.pair0 + best)].candidate;
        if (winner != win[0]) {
            std::cerr << path << ": attempt " << a << " is won by " << winner << ", expected " << win[0] << "\n";
            ++failures;
        }
    }
}

// ((a,b)p,(c,d)q)r as r0 p1 a2 b3 q4 c5 d6
void seven(Mat& m, const std::vector<Mat::B>& bs, const std::vector<Mat::M>& ms) {
    m.off = {0, 2, 4, 4, 4, 6, 6, 6};
    m.idx = {1, 4, 2, 3, 5, 6};
    m.build(7, 0, bs, ms);
}

constexpr int32_t kNI3 = (3 << 4) | 2;
constexpr uint32_t kNNN = 0xfff000, kACG = 0x124000;

void check_steps_and_blocks() {
    std::string err;
    pm::ImputePlan plan;
    {   // the donor through the grandparent: c and q are left upward, p is entered downward, a's list last
        Mat m;
        seven(m, {}, {{2, 0, 3, 0, kNI3, kNNN}, {5, 0, 3, 0, kNI3, kACG}});
        CHECK(pm::impute_plan(&m.p, 5, plan, err) == PM_OK);
        CHECK(plan.attempts.size() == 1 && plan.pairs.size() == 1 && plan.pairs[0].candidate == 5);
        CHECK(plan.attempts[0].node == 2 && plan.attempts[0].runs_with_n == 1);
        const std::vector<std::pair<int, int>> want = {{5, 1}, {4, 1}, {1, 0}, {2, 0}};
        CHECK(plan.steps.size() == want.size());
        for (size_t i = 0; i < want.size() && i < plan.steps.size(); ++i)
            CHECK(plan.steps[i].node == want[i].first && plan.steps[i].inverted == want[i].second);
        CHECK(plan.run_off[2] == 0 && plan.run_off[3] == 1 && plan.runs[0].length == 3 && plan.runs[0].ns == 3 && plan.runs[1].ns == 0);
    }
    {   // the sibling: one inverted step and the own list; the parent itself as a candidate: the own list alone
        Mat m;
        seven(m, {}, {{1, 0, 3, 0, kNI3, kACG}, {2, 0, 3, 0, kNI3, kNNN}, {3, 0, 3, 0, kNI3, kACG}});
        CHECK(pm::impute_plan(&m.p, 5, plan, err) == PM_OK);
        CHECK(plan.pairs.size() == 2 && plan.pairs[0].candidate == 1 && plan.pairs[1].candidate == 3);
        CHECK(plan.pairs[0].step1 - plan.pairs[0].step0 == 1 && plan.steps[0].node == 2 && !plan.steps[0].inverted);
        CHECK(plan.pairs[1].step1 - plan.pairs[1].step0 == 2 && plan.steps[1].node == 3 && plan.steps[1].inverted);
    }
    {   // block_swap: c's deletion of block 1 inverted is an insertion that a's deletion cancels: 1 - 0
        Mat m;
        seven(m, {{2, 1, 0, 0}, {5, 1, 0, 0}}, {{2, 0, 3, 0, kNI3, kNNN}, {5, 0, 3, 0, kNI3, kACG}});
        CHECK(pm::impute_plan(&m.p, 5, plan, err) == PM_OK);
        CHECK(plan.pairs.size() == 1 && plan.pairs[0].block_improvement == 1);
        std::vector<pm::ImputeBlockMut> blocks;
        CHECK(pm::impute_pair_blocks(&m.p, plan, plan.pairs[0], blocks, err) && blocks.empty());
        // wasBlockInv: the root never inserted block 1 here, its strand is the initial true: !true
        CHECK(plan.was_inv_off[2] == 0 && plan.was_inv_off[3] == 1 && plan.was_inv[0].primary == 1 && plan.was_inv[0].inversion == 0);
    }
    {   // block_ratchet: c's inversion stays on the path: 0 - 1; an inverted insertion becomes a plain deletion
        Mat m;
        seven(m, {{5, 1, 0, 1}, {4, 0, 1, 1}}, {{2, 0, 3, 0, kNI3, kNNN}, {5, 0, 3, 0, kNI3, kACG}});
        CHECK(pm::impute_plan(&m.p, 5, plan, err) == PM_OK);
        CHECK(plan.pairs.size() == 1 && plan.pairs[0].block_improvement == -2);
        std::vector<pm::ImputeBlockMut> blocks;
        CHECK(pm::impute_pair_blocks(&m.p, plan, plan.pairs[0], blocks, err) && blocks.size() == 2);
        if (blocks.size() == 2) {
            CHECK(blocks[0].primary == 0 && blocks[0].info == 0 && blocks[0].inversion == 0);
            CHECK(blocks[1].primary == 1 && blocks[1].info == 0 && blocks[1].inversion == 1);
        }
    }
    {   // the strand drifts: a inverts block 1, which the root inserted forward; the walk never applies that on the
        // way down but undoes it on the way up, so the deletion in a's later sibling b records !false
        Mat m;
        seven(m, {{0, 1, 1, 0}, {2, 1, 0, 1}, {3, 1, 0, 0}}, {});
        CHECK(pm::impute_plan(&m.p, 5, plan, err) == PM_OK);
        CHECK(plan.was_inv.size() == 1 && plan.was_inv_off[3] == 0 && plan.was_inv_off[4] == 1 && plan.was_inv[0].inversion == 1);
    }
    {   // a path on which consolidateBlockMutations throws: c's insertion of block 1, inverted, is a deletion, and
        // p deletes the block again
        Mat m;
        seven(m, {{5, 1, 1, 0}, {1, 1, 0, 0}, {2, 1, 0, 1}}, {{2, 0, 3, 0, kNI3, kNNN}, {5, 0, 3, 0, kNI3, kACG}});
        CHECK(pm::impute_plan(&m.p, 5, plan, err) == PM_ERR_ARG);
        CHECK(err == "Block deletion followed by inversion or deletion doesn't make sense");
    }
}

void check_winner_rule() {
    pm::ImputePair pairs[4] = {};
    {   // a tie: the first keeps the place
        const int64_t nuc[3] = {3, 3, 3};
        CHECK(pm::impute_winner(nuc, pairs, 3) == 0);
    }
    {   // -1 never beats the start, 0 does
        const int64_t nuc[2] = {-1, 0};
        CHECK(pm::impute_winner(nuc, pairs, 1) == -1 && pm::impute_winner(nuc, pairs, 2) == 1);
    }
    {   // the block ratchet: (2, 0), then (3, -1) refused, then (4, 1) taken, then (5, 0) refused
        const int64_t nuc[4] = {2, 3, 4, 5};
        pairs[1].block_improvement = -1;
        pairs[2].block_improvement = 1;
        CHECK(pm::impute_winner(nuc, pairs, 2) == 0 && pm::impute_winner(nuc, pairs, 3) == 2 && pm::impute_winner(nuc, pairs, 4) == 2);
    }
    CHECK(pm::impute_winner(nullptr, pairs, 0) == -1);
}

void check_argument_errors() {
    std::string err;
    CHECK(pm::impute_check(nullptr, err) == PM_ERR_ARG && err == "bad arguments");
    auto code = [&](Mat& m) { return pm::impute_check(&m.p, err); };
    Mat ok;
    seven(ok, {}, {{2, 0, 3, 0, kNI3, kNNN}});
    CHECK(code(ok) == PM_OK);
    {
        Mat m;
        seven(m, {}, {});
        m.p.root = 7;
        CHECK(code(m) == PM_ERR_ARG && err == "bad arguments");
        m.p.root = 0;
        m.p.names = nullptr;
        CHECK(code(m) == PM_ERR_ARG && err == "bad arguments");
    }
    {   // a child twice, the root as a child, a child out of range, decreasing offsets
        Mat m;
        seven(m, {}, {});
        m.idx[1] = 1;
        CHECK(code(m) == PM_ERR_ARG && err == "bad PanMAT topology");
        m.idx[1] = 0;
        CHECK(code(m) == PM_ERR_ARG && err == "bad PanMAT topology");
        m.idx[1] = 7;
        CHECK(code(m) == PM_ERR_ARG && err == "bad PanMAT topology");
        m.idx[1] = 4;
        m.off[2] = 1;
        CHECK(code(m) == PM_ERR_ARG && err == "bad offsets");
    }
    {   // a cycle beside the root: every node a child once, but 2 and 3 hang under each other
        Mat m;
        m.off = {0, 1, 1, 2, 3};
        m.idx = {1, 3, 2};
        m.build(4, 0, {}, {});
        CHECK(code(m) == PM_ERR_ARG && err == "bad PanMAT topology");
    }
    {
        Mat m;
        seven(m, {}, {{2, 0, 3, 0, kNI3, kNNN}});
        m.nm_secondary[0] = 0;
        CHECK(code(m) == PM_ERR_UNSUPPORTED && err == "secondary blocks");
    }
    {
        Mat m;
        seven(m, {}, {{2, 0, 3, 0, (1 << 4) | 6, 0}});
        CHECK(code(m) == PM_ERR_ARG && err == "unknown nucleotide mutation type");
    }
    {
        Mat m;
        seven(m, {}, {{2, 0, 3, -1, (7 << 4) | 0, 0}});
        CHECK(code(m) == PM_ERR_ARG && err == "nucleotide run longer than 6");
    }
    {
        Mat m;
        seven(m, {}, {{2, 0, 3, -1, (2 << 4) | 3, 0}});
        CHECK(code(m) == PM_ERR_ARG && err == "single-base record whose length is not 1");
    }
    {   // a negative block id in a block mutation is the plan's to refuse
        Mat m;
        seven(m, {{2, -1, 0, 0}}, {});
        pm::ImputePlan plan;
        CHECK(code(m) == PM_OK && pm::impute_plan(&m.p, 5, plan, err) == PM_ERR_ARG);
    }
}

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) check_case(argv[i]);
    check_steps_and_blocks();
    check_winner_rule();
    check_argument_errors();
    if (failures) {
        std::cerr << failures << " check(s) failed\n";
        return 1;
    }
    std::cout << "impute_host_check: " << (argc - 1) << " case files and the built-in checks passed\n";
    return 0;
}
