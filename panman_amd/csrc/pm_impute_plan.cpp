// pm_impute_plan.cpp -- the host plan of pm_impute; see pm_impute_plan.h.  No HIP.
#include "pm_impute_plan.h"

#include <algorithm>
#include <map>
#include <unordered_map>

namespace pm {
namespace {

constexpr uint32_t kNI = 2, kSnpI = 4;
constexpr uint32_t kN = 15;

struct RunKey {
    int32_t node, blk, pos, gap, length;
    bool operator==(const RunKey& o) const {
        return node == o.node && blk == o.blk && pos == o.pos && gap == o.gap && length == o.length;
    }
};
struct RunHash {
    size_t operator()(const RunKey& k) const {
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (uint32_t x : {(uint32_t)k.node, (uint32_t)k.blk, (uint32_t)k.pos, (uint32_t)k.gap, (uint32_t)k.length}) {
            h ^= x;
            h *= 0xff51afd7ed558ccdull;
            h ^= h >> 32;
        }
        return (size_t)h;
    }
};

// IndelPosition::mergeIndels (src/panman.hpp:408-421): the head's gap-ness alone picks the comparison.
bool merge_indels(ImputeRun& run, int32_t blk, int32_t pos, int32_t gap, int32_t length) {
    if (run.blk != blk) return false;
    if ((run.gap == -1 && (int64_t)pos - run.pos == run.length) || (run.gap != -1 && (int64_t)gap - run.gap == run.length)) {
        run.length += length;
        return true;
    }
    return false;
}

// allowedDistance - branchLength: int minus float in float, back to int toward zero
int32_t step_distance(int32_t allowed, float length) {
    const float d = (float)allowed - length;
    if (!(d > -2147483000.0f)) return -1;   // (below int's range, and NaN: the walk stops)
    if (d > 2147483000.0f) return 2147483000;
    return (int32_t)d;
}

// consolidateBlockMutations (src/panman.cpp:2324-2372) over the block lists of steps [s0, s1)
bool fold_steps(const pm_panmat* p, const ImputeStep* steps, int64_t n, std::vector<ImputeBlockMut>& out, std::string& err) {
    struct State {
        bool have;
        uint8_t info, inv;
    };
    std::map<int32_t, State> state;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t v = steps[i].node;
        for (int64_t k = p->block_mut_offsets[v]; k < p->block_mut_offsets[v + 1]; ++k) {
            bool ins = p->block_mut_info[k] != 0, inv = p->block_mut_inversion[k] != 0;
            if (steps[i].inverted) {
                // invertMutations: an insertion becomes a deletion; a deletion an insertion whose
                // strand stays false -- convertToInsertion(bool inversion) assigns its parameter to
                // itself (src/panman.hpp:498-501), so the wasBlockInv value it is handed is never
                // stored; an inversion stays
                if (ins) ins = inv = false;
                else if (!inv) ins = true;
            }
            State& s = state[p->block_mut_primary[k]];
            if (!s.have) {
                s = State{true, (uint8_t)ins, (uint8_t)inv};
            } else if (s.info) {
                if (ins) {
                    err = "Block insertion followed by insertion doesn't make sense";
                    return false;
                }
                if (!inv) s.have = false;
                else s.inv = !s.inv;
            } else if (!s.inv) {
                if (!ins) {
                    err = "Block deletion followed by inversion or deletion doesn't make sense";
                    return false;
                }
                s.have = false;
            } else {
                if (ins) {
                    err = "Block inversion followed by insertion doesn't make sense";
                    return false;
                }
                if (!inv) s = State{true, 0, 0};
                else s.have = false;
            }
        }
    }
    out.clear();
    for (const auto& kv : state)
        if (kv.second.have) out.push_back(ImputeBlockMut{kv.first, kv.second.info, kv.second.inv});
    return true;
}

}  // namespace

int impute_check(const pm_panmat* p, std::string& err) {
    const int32_t N = p ? p->num_nodes : 0;
    if (!p || N < 1 || !p->child_offsets || !p->names || !p->nuc_mut_offsets || !p->block_mut_offsets || p->root < 0 ||
        p->root >= N || p->num_blocks < 0 || (p->num_blocks > 0 && !p->block_primary)) {
        err = "bad arguments";
        return PM_ERR_ARG;
    }
    if (p->child_offsets[0] != 0 || p->nuc_mut_offsets[0] < 0 || p->block_mut_offsets[0] < 0) {
        err = "bad offsets";
        return PM_ERR_ARG;
    }
    for (int32_t v = 0; v < N; ++v)
        if (p->child_offsets[v] > p->child_offsets[v + 1] || p->nuc_mut_offsets[v] > p->nuc_mut_offsets[v + 1] ||
            p->block_mut_offsets[v] > p->block_mut_offsets[v + 1]) {
            err = "bad offsets";
            return PM_ERR_ARG;
        }
    if (p->child_offsets[N] != N - 1 || (N > 1 && !p->child_index)) {
        err = "bad PanMAT topology";
        return PM_ERR_ARG;
    }
    std::vector<char> seen((size_t)N, 0);
    for (int32_t e = 0; e < N - 1; ++e) {
        const int32_t ch = p->child_index[e];
        if (ch < 0 || ch >= N || ch == p->root || seen[(size_t)ch]) {
            err = "bad PanMAT topology";
            return PM_ERR_ARG;
        }
        seen[(size_t)ch] = 1;
    }
    {   // every node hangs under the root (N - 1 distinct children alone still allow a cycle beside it)
        std::vector<int32_t> st{p->root};
        int32_t reached = 0;
        while (!st.empty()) {
            const int32_t v = st.back();
            st.pop_back();
            ++reached;
            for (int32_t e = p->child_offsets[v]; e < p->child_offsets[v + 1]; ++e) st.push_back(p->child_index[e]);
        }
        if (reached != N) {
            err = "bad PanMAT topology";
            return PM_ERR_ARG;
        }
    }
    const int64_t muts = p->nuc_mut_offsets[N];
    if (muts > 0 && (!p->nuc_mut_primary || !p->nuc_mut_position || !p->nuc_mut_gap_position || !p->nuc_mut_info || !p->nuc_mut_nucs)) {
        err = "bad arguments";
        return PM_ERR_ARG;
    }
    if (p->block_mut_offsets[N] > 0 && (!p->block_mut_primary || !p->block_mut_info || !p->block_mut_inversion)) {
        err = "bad arguments";
        return PM_ERR_ARG;
    }
    for (int64_t k = p->nuc_mut_offsets[0]; k < muts; ++k) {
        const uint32_t info = p->nuc_mut_info[k], type = info & 7u;
        if (p->nuc_mut_secondary && p->nuc_mut_secondary[k] != -1) {
            err = "secondary blocks";
            return PM_ERR_UNSUPPORTED;
        }
        if (type > 5) {
            err = "unknown nucleotide mutation type";
            return PM_ERR_ARG;
        }
        if ((info >> 4) > 6) {
            err = "nucleotide run longer than 6";
            return PM_ERR_ARG;
        }
        if (type >= 3 && (info >> 4) != 1) {   // (length() is the nibble in src/impute.cpp, 1 in consolidateNucMutations)
            err = "single-base record whose length is not 1";
            return PM_ERR_ARG;
        }
    }
    return PM_OK;
}

bool impute_pair_blocks(const pm_panmat* p, const ImputePlan& plan, const ImputePair& pair, std::vector<ImputeBlockMut>& out,
                        std::string& err) {
    return fold_steps(p, plan.steps.data() + pair.step0, pair.step1 - pair.step0, out, err);
}

int64_t impute_winner(const int64_t* nuc_improvement, const ImputePair* pairs, int64_t n) {
    int64_t best_nuc = -1, best_block = 0, best = -1;
    for (int64_t i = 0; i < n; ++i)
        // (the reference's `&` of two comparisons)
        if (nuc_improvement[i] > best_nuc && pairs[i].block_improvement >= best_block) {
            best_nuc = nuc_improvement[i];
            best_block = pairs[i].block_improvement;
            best = i;
        }
    return best;
}

int impute_plan(const pm_panmat* p, int32_t max_distance, ImputePlan& out, std::string& err) {
    const int32_t N = p->num_nodes, root = p->root;
    out = ImputePlan();
    out.parent.assign((size_t)N, -1);
    for (int32_t v = 0; v < N; ++v)
        for (int32_t e = p->child_offsets[v]; e < p->child_offsets[v + 1]; ++e) out.parent[(size_t)p->child_index[e]] = v;
    const std::vector<int32_t>& parent = out.parent;

    // ---- insertion census (fillNucleotideLookupTables, :147-183), from the lists as they are
    std::unordered_map<RunKey, int32_t, RunHash> held;   // a node's runs by IndelPosition -> N count
    out.run_off.assign(1, 0);
    std::vector<ImputeRun> cur;
    for (int32_t v = 0; v < N; ++v) {
        cur.clear();
        if (v != root)   // (the root's list is never visited: its map stays empty)
            for (int64_t k = p->nuc_mut_offsets[v]; k < p->nuc_mut_offsets[v + 1]; ++k) {
                const uint32_t info = p->nuc_mut_info[k], type = info & 7u;
                if (type != kNI && type != kSnpI) continue;   // (other records do not end a run)
                const int32_t len = (int32_t)(info >> 4);
                int32_t ns = 0;
                for (int32_t i = 0; i < len; ++i) ns += ((p->nuc_mut_nucs[k] >> (4 * (5 - i))) & 15u) == kN;
                const int32_t blk = p->nuc_mut_primary[k], pos = p->nuc_mut_position[k], gap = p->nuc_mut_gap_position[k];
                if (!cur.empty() && merge_indels(cur.back(), blk, pos, gap, len)) cur.back().ns += ns;
                else cur.push_back(ImputeRun{blk, pos, gap, len, ns});
            }
        for (const ImputeRun& r : cur)   // std::inserter into the map: an equal key does not overwrite
            if (held.emplace(RunKey{v, r.blk, r.pos, r.gap, r.length}, r.ns).second) out.runs.push_back(r);
        out.run_off.push_back((int64_t)out.runs.size());
    }

    // ---- block tables (fillBlockLookupTables, :186-203; the strand undo, :130-139)
    {
        int32_t max_id = -1;
        for (int64_t k = 0; k < p->block_mut_offsets[N]; ++k) max_id = std::max(max_id, p->block_mut_primary[k]);
        for (int64_t k = 0; k < p->block_mut_offsets[N]; ++k)
            if (p->block_mut_primary[k] < 0) {
                err = "negative block id in a block mutation";
                return PM_ERR_ARG;
            }
        std::vector<uint8_t> strand((size_t)max_id + 1, 1);
        // getSequenceFromReference(root) (src/panman.cpp:4779-4818): the root's own block mutations
        for (int64_t k = p->block_mut_offsets[root]; k < p->block_mut_offsets[root + 1]; ++k) {
            uint8_t& s = strand[(size_t)p->block_mut_primary[k]];
            if (p->block_mut_info[k]) s = !p->block_mut_inversion[k];
            else if (p->block_mut_inversion[k]) s = !s;
            else s = 1;
        }
        std::vector<std::vector<ImputeBlockMut>> was((size_t)N);
        // the walk never applies an inversion on the way down and undoes every record flagged
        // `inversion` (inverted insertions too) on the way up: the strand drifts for later siblings
        std::vector<std::pair<int32_t, int32_t>> st;   // (node, next child edge)
        for (int32_t e = p->child_offsets[root + 1] - 1; e >= p->child_offsets[root]; --e) st.emplace_back(p->child_index[e], -1);
        while (!st.empty()) {
            const int32_t v = st.back().first;
            if (st.back().second == -1) {
                for (int64_t k = p->block_mut_offsets[v]; k < p->block_mut_offsets[v + 1]; ++k)
                    if (!p->block_mut_info[k] && !p->block_mut_inversion[k]) {
                        const int32_t id = p->block_mut_primary[k];
                        const uint8_t state = !strand[(size_t)id];
                        bool found = false;   // (operator[] of the map: a later deletion of the block overwrites)
                        for (ImputeBlockMut& w : was[(size_t)v])
                            if (w.primary == id) {
                                w.inversion = state;
                                found = true;
                            }
                        if (!found) was[(size_t)v].push_back(ImputeBlockMut{id, 0, state});
                    }
                st.back().second = p->child_offsets[v];
            }
            if (st.back().second < p->child_offsets[v + 1]) {
                const int32_t ch = p->child_index[st.back().second++];
                st.emplace_back(ch, -1);
                continue;
            }
            for (int64_t k = p->block_mut_offsets[v]; k < p->block_mut_offsets[v + 1]; ++k)
                if (p->block_mut_inversion[k]) strand[(size_t)p->block_mut_primary[k]] ^= 1;
            st.pop_back();
        }
        out.was_inv_off.assign(1, 0);
        for (int32_t v = 0; v < N; ++v) {
            out.was_inv.insert(out.was_inv.end(), was[(size_t)v].begin(), was[(size_t)v].end());
            out.was_inv_off.push_back((int64_t)out.was_inv.size());
        }
    }

    // ---- candidates (findNearbyInsertions, :288-337) and their paths
    struct Frame {
        int32_t node, from, dist;
    };
    std::vector<Frame> st;
    std::vector<int32_t> anc_stamp((size_t)N, -1), down;
    std::vector<ImputeRun> with_n;
    std::vector<ImputeBlockMut> folded;
    for (int32_t v = 0; v < N; ++v) {
        with_n.clear();
        for (int64_t r = out.run_off[(size_t)v]; r < out.run_off[(size_t)v + 1]; ++r)
            if (out.runs[(size_t)r].ns > 0) with_n.push_back(out.runs[(size_t)r]);
        if (with_n.empty()) continue;   // (never the root: its map is empty)
        const int32_t a = (int32_t)out.attempts.size(), start = parent[(size_t)v];
        ImputeAttempt at{v, (int32_t)with_n.size(), (int64_t)out.pairs.size(), 0};
        for (int32_t u = start; u >= 0; u = parent[(size_t)u]) anc_stamp[(size_t)u] = a;
        const int64_t own_blocks = p->block_mut_offsets[v + 1] - p->block_mut_offsets[v];
        st.assign(1, Frame{start, v, max_distance});
        while (!st.empty()) {
            const Frame f = st.back();
            st.pop_back();
            if (f.node < 0 || f.dist < 0) continue;
            // the first of the moving node's N-bearing runs (list order; the reference's is its hash
            // map's) that this node holds decides: a candidate unless it is all N here
            for (const ImputeRun& r : with_n) {
                const auto it = held.find(RunKey{f.node, r.blk, r.pos, r.gap, r.length});
                if (it == held.end()) continue;
                if (it->second < r.length) {
                    ImputePair pair{a, f.node, (int64_t)out.steps.size(), 0, 0};
                    int32_t u = f.node;
                    for (; anc_stamp[(size_t)u] != a; u = parent[(size_t)u]) out.steps.push_back(ImputeStep{u, 1});
                    down.clear();
                    for (int32_t w = start; w != u; w = parent[(size_t)w]) down.push_back(w);
                    for (size_t i = down.size(); i-- > 0;) out.steps.push_back(ImputeStep{down[i], 0});
                    out.steps.push_back(ImputeStep{v, 0});
                    pair.step1 = (int64_t)out.steps.size();
                    if (!fold_steps(p, out.steps.data() + pair.step0, pair.step1 - pair.step0, folded, err)) return PM_ERR_ARG;
                    pair.block_improvement = (int32_t)(own_blocks - (int64_t)folded.size());
                    out.pairs.push_back(pair);
                }
                break;
            }
            // the node itself, then its children in order, then its parent: pushed in reverse
            const int32_t up = parent[(size_t)f.node];
            if (up != f.from) st.push_back(Frame{up, f.node, step_distance(f.dist, p->branch_length ? p->branch_length[f.node] : 0.0f)});
            for (int32_t e = p->child_offsets[f.node + 1] - 1; e >= p->child_offsets[f.node]; --e) {
                const int32_t ch = p->child_index[e];
                if (ch != f.from) st.push_back(Frame{ch, f.node, step_distance(f.dist, p->branch_length ? p->branch_length[ch] : 0.0f)});
            }
        }
        at.pair1 = (int64_t)out.pairs.size();
        out.attempts.push_back(at);
    }
    return PM_OK;
}

}  // namespace pm
