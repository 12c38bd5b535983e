// pm_gfa_in.cpp -- PanMAN construction from a GFA + Newick (reference: Tree(ifstream&, ifstream&,
// FILE_TYPE::GFA), src/panman.cpp:728-819; GfaGraph, :6060-6197; chain_align, src/chaining.cpp).
//
// Host: the "S" / "P" records, the block order by chained alignment of the paths (pm_chain.h, the
// segment names interned to integers), the two-pointer walk of every path against that order.
// Device: block Fitch over every block column (PM_MODE_BLOCK_FITCH, also on polytomies, root
// parent state absent, no forced root).  The (paths x blocks) state matrix is almost entirely
// "absent": only the paths' steps travel, as sparse rows (pm_leaves_upload_sparse), in batches of
// columns (PM_OPT_GFA_IN_BATCH_SITES); no dense host matrix is built.
#include <algorithm>
#include <chrono>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "pm_build.h"
#include "pm_chain.h"
#include "pm_dev.h"

namespace pm {
namespace {

struct GfaPath {
    std::vector<int> seg;          // interned segment name per step
    std::vector<uint8_t> forward;  // strand per step
    std::vector<size_t> blocks;    // block id per step (GfaGraph::intSequences)
};

int build(pm_ctx* c, const char* gfa_text, const char* newick_c, PanmanTree& out) {
    // the phases are logged together at the end, and only by a build that succeeds
    auto mark = std::chrono::steady_clock::now();
    auto lap = [&](double& into) {
        into += seconds_since(mark);
        mark = std::chrono::steady_clock::now();
    };
    double t_parse = 0, t_chain = 0, t_upload = 0, t_run = 0, t_assemble = 0;
    // ---- parse (:729-753): "S" and "P" records, a later duplicate wins, anything else ignored
    std::map<std::string, std::string> nodes;
    std::map<std::string, std::vector<std::pair<std::string, bool>>> paths;
    for (const char* p = gfa_text; *p;) {
        const char* e = p;
        while (*e && *e != '\n') ++e;
        const std::string line(p, e);
        p = *e ? e + 1 : e;
        const std::vector<std::string> f = split_quoted(line, '\t');   // stringSplit
        if (f.empty()) continue;
        if (f[0] == "S") {
            if (f.size() < 3) return fail(c, PM_ERR_ARG, "GFA: S line with fewer than 3 fields: " + line.substr(0, 60));
            nodes[f[1]] = f[2];
        } else if (f[0] == "P") {
            if (f.size() < 3) return fail(c, PM_ERR_ARG, "GFA: P line with fewer than 3 fields: " + line.substr(0, 60));
            std::vector<std::pair<std::string, bool>> steps;
            for (const std::string& v : split_quoted(f[2], ',')) {
                if (v.size() < 2) return fail(c, PM_ERR_ARG, "GFA: path " + f[1] + ": empty step");
                steps.emplace_back(v.substr(0, v.size() - 1), v.back() == '+');
            }
            paths[f[1]] = std::move(steps);
        }
    }
    if (paths.empty()) return fail(c, PM_ERR_ARG, "GFA: no P line");
    // segment names -> integers (equal names, equal integers: chaining only compares them)
    std::unordered_map<std::string, int> seg_id;
    std::vector<const std::string*> seg_seq;
    std::vector<std::string> path_name;
    std::vector<GfaPath> gp;
    for (const auto& p : paths) {   // std::map order: ascending names
        GfaPath g;
        for (size_t i = 0; i < p.second.size(); ++i) {
            const std::string& name = p.second[i].first;
            auto it = seg_id.find(name);
            if (it == seg_id.end()) {
                auto n = nodes.find(name);
                if (n == nodes.end())
                    return fail(c, PM_ERR_ARG, "GFA: path " + p.first + ": step " + std::to_string(i) +
                                                   " names the undefined segment " + name);
                it = seg_id.emplace(name, (int)seg_seq.size()).first;
                seg_seq.push_back(&n->second);
            }
            g.seg.push_back(it->second);
            g.forward.push_back(p.second[i].second ? 1 : 0);
        }
        path_name.push_back(p.first);
        gp.push_back(std::move(g));
    }
    Topology t;
    std::string err;
    if (!parse_newick(newick_c, t, err)) return fail(c, PM_ERR_ARG, "Newick: " + err);
    const int32_t N = (int32_t)t.name.size();
    lap(t_parse);

    // ---- block order (GfaGraph::GfaGraph, :6060-6142): the first path seeds the consensus, every
    // later one is chained against it; unmatched steps get fresh ids; ids renumbered at the end
    size_t num_nodes = 0;
    std::unordered_map<int, int> int_to_seg;
    std::vector<int> cons;
    std::vector<size_t> int_cons;
    for (size_t s = 0; s < gp.size(); ++s) {
        if (s == 0) {
            for (int seg : gp[0].seg) {
                cons.push_back(seg);
                int_to_seg[(int)num_nodes] = seg;
                gp[0].blocks.push_back(num_nodes);
                int_cons.push_back(num_nodes);
                ++num_nodes;
            }
        } else {
            std::vector<size_t> int_cons_new;
            std::vector<int> cons_new;
            const std::vector<Pt> chain = chaining(cons, gp[s].seg);
            build_consensus(chain, cons, gp[s].seg, int_cons, gp[s].blocks, num_nodes, cons_new, int_cons_new, int_to_seg);
            cons.swap(cons_new);
            int_cons.swap(int_cons_new);
        }
    }
    const size_t T = int_cons.size();
    std::vector<size_t> order(num_nodes, 0);
    std::vector<int> block_seg(T);
    for (size_t i = 0; i < T; ++i) {
        order[int_cons[i]] = i;
        block_seg[i] = int_to_seg[(int)int_cons[i]];
    }
    for (GfaPath& g : gp)
        for (size_t& b : g.blocks) b = order[b];

    // ---- aligned states (getAlignedSequences / getAlignedStrandSequences, :6144-6193; :784-797):
    // p1 walks the blocks 0..T-1, p2 the path; a step is taken where they meet, and a step whose
    // block lies behind p1 is never met, nor is any step after it.  Rows: the paths a leaf names.
    std::unordered_map<std::string, int32_t> path_of;
    for (size_t s = 0; s < path_name.size(); ++s) path_of[path_name[s]] = (int32_t)s;
    std::vector<int32_t> node_row(N, -1), row_path;
    for (int32_t v = 0; v < N; ++v)
        if (t.kids[v].empty()) {
            auto it = path_of.find(t.name[v]);
            if (it == path_of.end()) continue;
            node_row[v] = (int32_t)row_path.size();
            row_path.push_back(it->second);
        }
    const int32_t R = (int32_t)row_path.size();
    std::vector<std::vector<std::pair<int32_t, uint8_t>>> entries(R);   // (block, 1 forward / 2 reverse), ascending
    for (int32_t r = 0; r < R; ++r) {
        const GfaPath& g = gp[row_path[r]];
        size_t p1 = 0;
        for (size_t p2 = 0; p2 < g.blocks.size() && g.blocks[p2] >= p1 && g.blocks[p2] < T; ++p2) {
            entries[r].emplace_back((int32_t)g.blocks[p2], g.forward[p2] ? 1 : 2);
            p1 = g.blocks[p2] + 1;
        }
    }
    lap(t_chain);

    tree_from_topology(t, out);
    const pm_tree tree = tree_view(out);
    int rc = pm_tree_upload(c, &tree);
    if (rc != PM_OK) return rc;
    lap(t_upload);

    // ---- block Fitch (:798-800), batches of columns
    std::vector<std::vector<BlockRec>> bmuts(N);
    std::vector<size_t> cursor(R, 0);
    std::vector<int64_t> row_off(R + 1, 0);
    std::vector<int32_t> site;
    std::vector<uint8_t> code;
    const int64_t batch = std::max<int64_t>(1, std::min(c->gfa_in_batch_sites, kMaxUploadSites));
    for (int64_t c0 = 0; c0 < (int64_t)T; c0 += batch) {
        const int64_t S = std::min<int64_t>(batch, (int64_t)T - c0);
        site.clear();
        code.clear();
        for (int32_t r = 0; r < R; ++r) {
            size_t& k = cursor[r];
            for (; k < entries[r].size() && entries[r][k].first < c0 + S; ++k) {
                site.push_back((int32_t)(entries[r][k].first - c0));
                code.push_back(entries[r][k].second);
            }
            row_off[r + 1] = (int64_t)site.size();
        }
        const std::vector<uint8_t> cons_p((size_t)(S + 1) / 2, 0);   // root parent state: absent
        if ((rc = pm_leaves_upload_sparse(c, S, R, row_off.data(), site.data(), code.data(), 0, node_row.data())) != PM_OK) return rc;
        lap(t_upload);
        std::vector<pm_mut> recs;
        if ((rc = run_columns(c, PM_MODE_BLOCK_FITCH, cons_p, nullptr, recs)) != PM_OK) return rc;
        for (const pm_mut& m : recs)
            bmuts[m.node].emplace_back((int32_t)(c0 + (m.site_info >> 8)), (uint8_t)(m.site_info & 0xFF));
        lap(t_run);
    }

    // ---- the PanMAT: blocks Block(i, sequence) (:777-779); no gaps, no nucleotide mutations
    out.block_seq_off.assign(1, 0);
    out.gap_off.assign(1, 0);
    for (size_t i = 0; i < T; ++i) {
        const std::vector<uint32_t> w = encode_block(*seg_seq[block_seg[i]]);
        out.block_primary.push_back((int32_t)i);
        out.block_seq.insert(out.block_seq.end(), w.begin(), w.end());
        out.block_seq_off.push_back((int64_t)out.block_seq.size());
    }
    for (int32_t v = 0; v < N; ++v) {
        std::sort(bmuts[v].begin(), bmuts[v].end());   // ascending block id (the reference's order is TBB-scheduled)
        append_block_muts(out, v, bmuts[v]);
    }
    lap(t_assemble);
    phase_add("gfain.parse", t_parse);
    phase_add("gfain.chain", t_chain);
    phase_add("gfain.upload", t_upload);
    phase_add("gfain.run", t_run);
    phase_add("gfain.assemble", t_assemble);
    return PM_OK;
}

}  // namespace
}  // namespace pm

extern "C" int pm_gfa_build(pm_ctx* c, const char* gfa_text, const char* newick, pm_panman** out) {
    if (!c || !gfa_text || !newick || !out) return PM_ERR_ARG;
    return pm::build_handle(c, "gfa build", out, [&](pm::PanmanTree& tree) { return pm::build(c, gfa_text, newick, tree); });
}
