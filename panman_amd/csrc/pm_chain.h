// pm_chain.h -- what the PanGraph and GFA builders share: chain_align (src/chaining.cpp:285-310)
// restated, the chained alignment of a path of block names against the running consensus order.
// Order-dependent steps follow the reference's containers (the score map is the same
// std::unordered_map fed the same insertions, so libstdc++ iterates it in the same order).
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace pm {

// ---- src/chaining.cpp -----------------------------------------------------------------
using Pt = std::pair<int, int>;
inline const Pt kOrigin(-1, -1);

struct HashPair {   // src/chaining.cpp:24-37
    size_t operator()(const Pt& p) const {
        const size_t h1 = std::hash<int>{}(p.first), h2 = std::hash<int>{}(p.second);
        return h1 != h2 ? h1 ^ h2 : h1;
    }
};

struct RangeNode {
    Pt point;
    int left = -1, right = -1;
};

inline int build_range_tree(std::vector<Pt>& pts, int start, int end, std::vector<RangeNode>& nodes) {   // :69-82
    if (start > end) return -1;
    std::sort(pts.begin() + start, pts.begin() + end + 1, [](const Pt& a, const Pt& b) { return a.first < b.first; });
    const int mid = (start + end) / 2;
    const int me = (int)nodes.size();
    nodes.push_back(RangeNode{pts[mid]});
    const int l = build_range_tree(pts, start, mid - 1, nodes);
    const int r = build_range_tree(pts, mid + 1, end, nodes);
    nodes[me].left = l;
    nodes[me].right = r;
    return me;
}

inline void query_range(const std::vector<RangeNode>& nodes, int root, Pt lo, Pt hi, std::vector<Pt>& out) {   // :87-100
    if (root < 0) return;
    const RangeNode& n = nodes[root];
    if (n.point.first >= lo.first && n.point.first <= hi.first && n.point.second >= lo.second &&
        n.point.second <= hi.second)
        out.push_back(n.point);
    if (n.left >= 0 && lo.first <= n.point.first) query_range(nodes, n.left, lo, hi, out);
    if (n.right >= 0 && hi.first >= n.point.first) query_range(nodes, n.right, lo, hi, out);
}

using ScoreMap = std::unordered_map<Pt, std::pair<int, Pt>, HashPair>;

inline void find_chain(const std::vector<RangeNode>& nodes, int root, Pt point, ScoreMap& map, int K) {   // :102-143
    const int match = 50;
    if (point.first == 0 && point.second == 0) {
        map[point] = {match, Pt(-1, -1)};
        return;
    }
    std::vector<Pt> result;
    query_range(nodes, root, Pt(point.first - K > 0 ? point.first - K : 0, point.second - K > 0 ? point.second - K : 0),
                Pt(point.first - 1, point.second - 1), result);
    int best = 10;
    Pt best_node = kOrigin;
    int xb = -1, yb = -1;
    for (auto it = result.rbegin(); it != result.rend(); ++it) {
        const Pt p = *it;
        if (p.first <= xb && p.second <= yb) continue;
        const int cost = -(point.first - p.first + point.second - p.second);
        if (cost + map[p].first + match > best) {
            best = cost + map[p].first + match;
            best_node = p;
        }
        if (xb < p.first) xb = p.first - 1;
        if (yb < p.second) yb = p.second - 1;
    }
    map[point] = {best, best_node};
}

// `Name`: the block names as given (PanGraph) or interned to integers (GFA).
template <class Name>
std::vector<Pt> chaining(const std::vector<Name>& cons, const std::vector<Name>& sample) {   // :146-230
    std::vector<Pt> chain;
    const int K = 4000;
    // every (i, j) with cons[i] == sample[j], through an index of the sample's positions by name
    // instead of the reference's loop over all pairs; the sort below fixes the order either way
    std::unordered_map<Name, std::vector<int>> where;
    for (size_t j = 0; j < sample.size(); ++j) where[sample[j]].push_back((int)j);
    std::vector<Pt> pts;
    for (size_t i = 0; i < cons.size(); ++i) {
        auto it = where.find(cons[i]);
        if (it == where.end()) continue;
        for (int j : it->second) pts.emplace_back((int)i, j);
    }
    std::sort(pts.begin(), pts.end());   // comparePoint: (x, y), points are distinct
    std::vector<RangeNode> nodes;
    nodes.reserve(pts.size());
    const int root = build_range_tree(pts, 0, (int)pts.size() - 1, nodes);
    if (pts.empty()) return chain;
    ScoreMap map;
    for (const Pt& p : pts) map[p] = {-1, kOrigin};
    for (const Pt& p : pts) find_chain(nodes, root, p, map, K);
    int best = -1;
    Pt seed{};
    for (const auto& m : map)
        if (m.second.first > best) {
            best = m.second.first;
            seed = m.first;
        }
    while (true) {
        chain.push_back(seed);
        seed = map[seed].second;
        if (seed == kOrigin) break;
    }
    return chain;
}

template <class Name>
void build_consensus(const std::vector<Pt>& chain, const std::vector<Name>& cons, const std::vector<Name>& sample,
                     const std::vector<size_t>& int_cons, std::vector<size_t>& int_sample, size_t& num_blocks,
                     std::vector<Name>& cons_new, std::vector<size_t>& int_cons_new,
                     std::unordered_map<int, Name>& int_to_string) {   // :233-277
    int pc = -1, ps = -1;
    for (auto it = chain.rbegin(); it != chain.rend(); ++it) {
        const int cc = it->first, sc = it->second;
        for (int j = pc + 1; j < cc; ++j) {
            cons_new.push_back(cons[j]);
            int_cons_new.push_back(int_cons[j]);
        }
        for (int j = ps + 1; j < sc; ++j) {
            cons_new.push_back(sample[j]);
            int_sample.push_back(num_blocks);
            int_to_string[(int)num_blocks] = sample[j];
            int_cons_new.push_back(num_blocks);
            ++num_blocks;
        }
        cons_new.push_back(cons[cc]);
        int_sample.push_back(int_cons[cc]);
        int_cons_new.push_back(int_cons[cc]);
        pc = cc;
        ps = sc;
    }
    for (int j = pc + 1; j < (int)cons.size(); ++j) {
        cons_new.push_back(cons[j]);
        int_cons_new.push_back(int_cons[j]);
    }
    for (int j = ps + 1; j < (int)sample.size(); ++j) {
        cons_new.push_back(sample[j]);
        int_sample.push_back(num_blocks);
        int_to_string[(int)num_blocks] = sample[j];
        int_cons_new.push_back(num_blocks);
        ++num_blocks;
    }
}

}  // namespace pm
