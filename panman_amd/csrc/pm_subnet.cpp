// pm_subnet.cpp -- Tree::subtreeExtractParallel + compressTreeParallel (src/subnet.cpp:3-135) with the
// nucleotide consolidation of every merged chain on the GPU (pm_subnet.hip).
//
//   1. host, O(nodes): the requested nodes and their ancestors are kept; a kept node with exactly one
//      kept child merges with it (mergeNodes, src/panman.cpp:2033-2055), so every maximal unary chain
//      becomes one new node named after the chain's bottom, its branch lengths summed top down.  The new
//      nodes are numbered in pre-order, children in their original order.
//   2. host: a merged node's block mutations, folded per block id (consolidateBlockMutations,
//      src/panman.cpp:2324-2372).  They are few and the fold is a 3 x 3 table; output by block id.
//   3. device: a merged node's nucleotide records, the chain's lists top first, in batches of whole new
//      nodes (PM_OPT_SUBNET_BATCH_ENTRIES): expand, sort, fold, group, pack.
//   4. host: the packed records spliced between the verbatim lists of the nodes that merged with nothing
//      (the reference consolidates only on a merge).
#include <algorithm>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "pm_build.h"
#include "pm_dev.h"

namespace pm {
namespace {

struct NewTree {
    int32_t nodes = 0;
    std::vector<int32_t> chain_off{0}, chain;   // per new node its original nodes, top first
    std::vector<int32_t> parent;
};

}  // namespace

int rank_tables(pm_ctx* c, const pm_panmat* p, RankTables& t) {
    int32_t max_id = -1;
    for (int32_t b = 0; b < p->num_blocks; ++b) {
        if (p->block_primary[b] < 0) return fail(c, PM_ERR_UNSUPPORTED, "duplicate or negative primary block id");
        max_id = std::max(max_id, p->block_primary[b]);
    }
    const int32_t B = max_id + 1;
    t.blk_len.assign(B, -1);
    t.pos_off.assign(B, 0);
    t.block_base.assign(B, 0);
    int64_t cells = 0;
    for (int32_t b = 0; b < p->num_blocks; ++b) {
        const int32_t id = p->block_primary[b];
        if (t.blk_len[id] >= 0) return fail(c, PM_ERR_UNSUPPORTED, "duplicate or negative primary block id");
        int32_t n = 0;
        bool end = false;
        for (int64_t w = p->block_seq_offsets[b]; w < p->block_seq_offsets[b + 1] && !end; ++w)
            for (int k = 0; k < 8; ++k) {
                if (((p->block_seq[w] >> (4 * (7 - k))) & 15) == 0) { end = true; break; }
                ++n;
            }
        t.blk_len[id] = n;
        cells += n + 2;
    }
    for (int32_t id = 0; id < B; ++id) {   // ids ascending: primaryBlockId order
        t.pos_off[id] = id ? t.pos_off[id - 1] + (t.blk_len[id - 1] < 0 ? 0 : t.blk_len[id - 1] + 2) : 0;
    }
    // gap slots per position (a later entry of a position replaces an earlier one, as in the replay)
    std::vector<uint32_t> slots((size_t)cells, 0);
    for (int32_t g = 0; g < p->num_gaps; ++g) {
        const int32_t id = p->gap_primary[g];
        if (id < 0 || id >= B || t.blk_len[id] < 0) return fail(c, PM_ERR_UNSUPPORTED, "gap list for a missing block");
        for (int64_t k = p->gap_offsets[g]; k < p->gap_offsets[g + 1]; ++k) {
            if (p->gap_position[k] > (uint32_t)t.blk_len[id]) return fail(c, PM_ERR_ARG, "gap position beyond the block");
            slots[(size_t)(t.pos_off[id] + p->gap_position[k])] = p->gap_length[k];
        }
    }
    t.pos_base.assign((size_t)cells, 0);
    uint64_t total = 0;
    for (int32_t id = 0; id < B; ++id) {
        if (t.blk_len[id] < 0) continue;
        if (total >= ((uint64_t)1 << 32)) break;
        t.block_base[id] = (uint32_t)total;
        uint64_t at = 0;
        for (int32_t j = 0; j <= t.blk_len[id]; ++j) {
            t.pos_base[(size_t)(t.pos_off[id] + j)] = (uint32_t)at;
            at += 1 + (uint64_t)slots[(size_t)(t.pos_off[id] + j)];
            if (at >= ((uint64_t)1 << 32)) break;
        }
        t.pos_base[(size_t)(t.pos_off[id] + t.blk_len[id] + 1)] = (uint32_t)at;
        total += at;
    }
    if (total >= ((uint64_t)1 << 32)) return fail(c, PM_ERR_UNSUPPORTED, "2^32 or more (position, gap slot) coordinates");
    return PM_OK;
}

const char* coordinate_error(int32_t code) {
    switch (code) {
        case kSubnetBadBlock: return "mutation on a missing block";
        case kSubnetBadPos: return "mutation beyond the block";
        case kSubnetBadGap: return "gap-slot mutation outside the slot range";
        default: return "the sort did not keep equal keys in entry order";
    }
}

namespace {

// consolidateBlockMutations over a chain's lists; false with the reference's message in `err`.
bool fold_blocks(const pm_panmat* p, const int32_t* chain, size_t links, PanmanTree& out, std::string& err) {
    struct State {
        bool have;
        uint8_t info, inv;
    };
    std::map<int32_t, State> state;
    for (size_t l = 0; l < links; ++l)
        for (int64_t k = p->block_mut_offsets[chain[l]]; k < p->block_mut_offsets[chain[l] + 1]; ++k) {
            State& s = state[p->block_mut_primary[k]];
            const bool ins = p->block_mut_info[k] != 0, inv = p->block_mut_inversion[k] != 0;
            if (!s.have) {
                s = State{true, (uint8_t)ins, (uint8_t)inv};
            } else if (s.info) {   // an insertion
                if (ins) {
                    err = "Block insertion followed by insertion doesn't make sense";
                    return false;
                }
                if (!inv) s.have = false;   // a deletion cancels it
                else s.inv = !s.inv;        // an inversion flips the inserted strand
            } else if (!s.inv) {   // a deletion
                if (!ins) {
                    err = "Block deletion followed by inversion or deletion doesn't make sense";
                    return false;
                }
                s.have = false;
            } else {               // an inversion
                if (ins) {
                    err = "Block inversion followed by insertion doesn't make sense";
                    return false;
                }
                if (!inv) s = State{true, 0, 0};
                else s.have = false;
            }
        }
    for (const auto& kv : state)
        if (kv.second.have) {
            out.bm_primary.push_back(kv.first);
            out.bm_info.push_back(kv.second.info);
            out.bm_inv.push_back(kv.second.inv);
        }
    return true;
}

struct Packed {   // the device's records of the merged nodes, in new-node order
    std::vector<int32_t> primary, pos, gap;
    std::vector<uint8_t> info;
    std::vector<uint32_t> nucs;
    std::vector<int32_t> node_count;
};

struct Times {
    double upload = 0, expand = 0, sort = 0, fold = 0, group = 0, download = 0;
};

template <class T>
hipError_t append(pm_ctx* c, const Dev<T>& d, int64_t n, std::vector<T>& v) {
    const size_t at = v.size();
    v.resize(at + (size_t)n);
    return n ? hipMemcpyAsync(v.data() + at, d.p, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

// One batch: the records [r0, r1) of the host arrays `rec`, `n` bases in all.
struct Records {
    std::vector<int32_t> node, primary, pos, gap;
    std::vector<uint8_t> info;
    std::vector<uint32_t> nucs;
};

int run_batch(pm_ctx* c, const Records& rec, int64_t r0, int64_t r1, int64_t n, SubnetArgs a, int end_bit, int32_t* d_count,
              Packed& out, Times& t) {
    const hipStream_t s = c->stream;
    const int64_t R = r1 - r0;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](double& into) {
        into += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
    };
    Dev<int32_t> d_node, d_primary, d_pos, d_gap;
    Dev<uint8_t> d_info;
    Dev<uint32_t> d_nucs;
    Dev<int64_t> d_off;
    hipError_t e = d_node.put(rec.node.data() + r0, R, s);
    if (e == hipSuccess) e = d_primary.put(rec.primary.data() + r0, R, s);
    if (e == hipSuccess) e = d_pos.put(rec.pos.data() + r0, R, s);
    if (e == hipSuccess) e = d_gap.put(rec.gap.data() + r0, R, s);
    if (e == hipSuccess) e = d_info.put(rec.info.data() + r0, R, s);
    if (e == hipSuccess) e = d_nucs.put(rec.nucs.data() + r0, R, s);
    if (e == hipSuccess) e = d_off.alloc(R + 1, false, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet upload");
    lap(t.upload);

    a.records = R;
    a.rec_node = d_node.p;
    a.rec_primary = d_primary.p;
    a.rec_pos = d_pos.p;
    a.rec_gap = d_gap.p;
    a.rec_info = d_info.p;
    a.rec_nucs = d_nucs.p;
    a.rec_off = d_off.p;
    int32_t bad = 0;
    int64_t total = 0;
    e = launch_subnet_count(c, a);
    if (e == hipSuccess) e = exclusive_scan(c, d_off.p, d_off.p, R + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, a.error, sizeof bad, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, d_off.p + R, sizeof total, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet count");
    if (bad) return fail(c, PM_ERR_ARG, coordinate_error(bad));
    if (total != n) return fail(c, PM_ERR_STATE, "subnet: the device counted other bases than the host");
    Dev<uint64_t> key, val, key_alt, val_alt;
    Dev<int32_t> eb, ep, eg;
    if ((e = key.alloc(n, false, s)) != hipSuccess || (e = val.alloc(n, false, s)) != hipSuccess ||
        (e = key_alt.alloc(n, false, s)) != hipSuccess || (e = val_alt.alloc(n, false, s)) != hipSuccess ||
        (e = eb.alloc(n, false, s)) != hipSuccess || (e = ep.alloc(n, false, s)) != hipSuccess ||
        (e = eg.alloc(n, false, s)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "subnet entries (lower PM_OPT_SUBNET_BATCH_ENTRIES)");
    const SubnetEntries ent{n, key.p, val.p, eb.p, ep.p, eg.p};
    e = launch_subnet_expand(c, a, ent);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet expand");
    lap(t.expand);

    uint64_t *skey = nullptr, *sval = nullptr;
    if ((e = subnet_sort(c, ent, key_alt.p, val_alt.p, end_bit, &skey, &sval)) != hipSuccess) return hip_fail(c, e, "subnet sort");
    lap(t.sort);

    Dev<int64_t> alive;
    Dev<uint8_t> tc;
    int64_t m = 0;
    if ((e = alive.alloc(n + 1, false, s)) != hipSuccess || (e = tc.alloc(n, false, s)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "subnet fold (lower PM_OPT_SUBNET_BATCH_ENTRIES)");
    e = launch_subnet_fold(c, skey, sval, n, alive.p, tc.p, a.error);
    if (e == hipSuccess) e = exclusive_scan(c, alive.p, alive.p, n + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, a.error, sizeof bad, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&m, alive.p + n, sizeof m, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet fold");
    if (bad) return fail(c, PM_ERR_STATE, coordinate_error(bad));
    lap(t.fold);
    if (m == 0) return PM_OK;   // every coordinate cancelled

    Dev<int32_t> ln, lb, lp, lg;
    Dev<uint8_t> ltc;
    Dev<int64_t> head, start;
    if ((e = ln.alloc(m, false, s)) != hipSuccess || (e = lb.alloc(m, false, s)) != hipSuccess ||
        (e = lp.alloc(m, false, s)) != hipSuccess || (e = lg.alloc(m, false, s)) != hipSuccess ||
        (e = ltc.alloc(m, false, s)) != hipSuccess || (e = head.alloc(m, false, s)) != hipSuccess ||
        (e = start.alloc(m + 1, false, s)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "subnet survivors (lower PM_OPT_SUBNET_BATCH_ENTRIES)");
    const SubnetLive live{m, ln.p, lb.p, lp.p, lg.p, ltc.p, head.p, start.p};
    int64_t recs = 0;
    e = launch_subnet_compact(c, skey, sval, n, alive.p, tc.p, ent, live);
    if (e == hipSuccess) e = subnet_runs(c, live);
    if (e == hipSuccess) e = exclusive_scan(c, start.p, start.p, m + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(&recs, start.p + m, sizeof recs, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet runs");
    Dev<int32_t> op, oo, og;
    Dev<uint8_t> oi;
    Dev<uint32_t> on;
    if ((e = op.alloc(recs, false, s)) != hipSuccess || (e = oo.alloc(recs, false, s)) != hipSuccess ||
        (e = og.alloc(recs, false, s)) != hipSuccess || (e = oi.alloc(recs, false, s)) != hipSuccess ||
        (e = on.alloc(recs, false, s)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "subnet records");
    e = launch_subnet_pack(c, live, SubnetOut{op.p, oo.p, og.p, oi.p, on.p, d_count});
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet pack");
    lap(t.group);

    e = append(c, op, recs, out.primary);
    if (e == hipSuccess) e = append(c, oo, recs, out.pos);
    if (e == hipSuccess) e = append(c, og, recs, out.gap);
    if (e == hipSuccess) e = append(c, oi, recs, out.info);
    if (e == hipSuccess) e = append(c, on, recs, out.nucs);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "subnet download");
    lap(t.download);
    return PM_OK;
}

int subnet(pm_ctx* c, const pm_panmat* p, const char* const* ids, int64_t num_ids, PanmanTree& out) {
    PhaseClock clock;
    const int32_t N = p->num_nodes;
    if (N < 1 || !p->names || !p->child_offsets || p->root < 0 || p->root >= N) return fail(c, PM_ERR_ARG, "bad PanMAT topology");
    if (num_ids <= 0) return fail(c, PM_ERR_ARG, "no node identifiers given");
    std::vector<std::string> name(N);
    std::unordered_map<std::string, int32_t> by_name;
    const char* nm = p->names;
    for (int32_t i = 0; i < N; ++i) {
        name[i] = nm;
        nm += name[i].size() + 1;
        by_name.emplace(name[i], i);
    }
    std::vector<int32_t> parent(N, -1);
    for (int32_t i = 0; i < N; ++i)
        for (int32_t e = p->child_offsets[i]; e < p->child_offsets[i + 1]; ++e) {
            const int32_t ch = p->child_index[e];
            if (ch < 0 || ch >= N || ch == p->root || parent[ch] != -1) return fail(c, PM_ERR_ARG, "bad PanMAT topology");
            parent[ch] = i;
        }
    // 1. tick the requested nodes and their ancestors (src/subnet.cpp:101-135)
    std::vector<char> kept(N, 0);
    for (int64_t k = 0; k < num_ids; ++k) {
        const auto it = ids[k] ? by_name.find(ids[k]) : by_name.end();
        if (it == by_name.end()) return fail(c, PM_ERR_ARG, "Some of the specified node identifiers don't exist!!!");
        for (int32_t v = it->second; v >= 0 && !kept[v]; v = parent[v]) kept[v] = 1;
    }
    if (!kept[p->root]) return fail(c, PM_ERR_ARG, "node unreachable from the root");
    // the chains (src/subnet.cpp:3-53), new nodes in pre-order
    NewTree t;
    std::vector<std::pair<int32_t, int32_t>> st{{p->root, -1}};   // (chain top, new parent)
    std::vector<int32_t> kids;
    while (!st.empty()) {
        int32_t v = st.back().first;
        t.parent.push_back(st.back().second);
        st.pop_back();
        for (;;) {
            t.chain.push_back(v);
            kids.clear();
            for (int32_t e = p->child_offsets[v]; e < p->child_offsets[v + 1]; ++e)
                if (kept[p->child_index[e]]) kids.push_back(p->child_index[e]);
            if (kids.size() != 1) break;
            v = kids[0];
        }
        t.chain_off.push_back((int32_t)t.chain.size());
        for (size_t j = kids.size(); j-- > 0;) st.emplace_back(kids[j], t.nodes);
        ++t.nodes;
    }
    const int32_t M = t.nodes;
    Topology topo;
    topo.root = 0;
    topo.kids.resize(M);
    for (int32_t v = 1; v < M; ++v) topo.kids[t.parent[v]].push_back(v);   // (ascending: the original order)
    for (int32_t v = 0; v < M; ++v) {
        const int32_t* ch = t.chain.data() + t.chain_off[v];
        const int32_t links = t.chain_off[v + 1] - t.chain_off[v];
        topo.name.push_back(name[ch[links - 1]]);
        if (p->branch_length) {
            float len = p->branch_length[ch[0]];
            for (int32_t l = 1; l < links; ++l) len += p->branch_length[ch[l]];   // par->branchLength += chi->branchLength
            topo.length.push_back(len);
        }
    }
    tree_from_topology(topo, out);
    for (int32_t v = 0; v < M; ++v) {
        // kept by the surviving name; the reference also keeps the entries of dropped names, which nothing reads
        const int32_t bottom = t.chain[t.chain_off[v + 1] - 1];
        if (p->circular_offset) out.circular[v] = p->circular_offset[bottom];
        if (p->rotation_index) out.rotation[v] = p->rotation_index[bottom];
        if (p->sequence_inverted) out.inverted[v] = p->sequence_inverted[bottom];
    }

    // 2. block mutations, and the merged chains' nucleotide records in chain order
    Records rec;
    std::vector<int64_t> node_rec{0}, node_bases{0};   // per merged node: prefix of its records and bases
    std::vector<int32_t> merged;
    for (int32_t v = 0; v < M; ++v) {
        const int32_t* ch = t.chain.data() + t.chain_off[v];
        const int32_t links = t.chain_off[v + 1] - t.chain_off[v];
        if (links == 1) {
            for (int64_t k = p->block_mut_offsets[ch[0]]; k < p->block_mut_offsets[ch[0] + 1]; ++k) {
                out.bm_primary.push_back(p->block_mut_primary[k]);
                out.bm_info.push_back(p->block_mut_info[k]);
                out.bm_inv.push_back(p->block_mut_inversion[k]);
            }
        } else {
            std::string err;
            if (!fold_blocks(p, ch, (size_t)links, out, err)) return fail(c, PM_ERR_ARG, err);
            int64_t bases = 0;
            for (int32_t l = 0; l < links; ++l)
                for (int64_t k = p->nuc_mut_offsets[ch[l]]; k < p->nuc_mut_offsets[ch[l] + 1]; ++k) {
                    const uint32_t info = p->nuc_mut_info[k], type = info & 7u;
                    if (p->nuc_mut_secondary && p->nuc_mut_secondary[k] != -1) return fail(c, PM_ERR_UNSUPPORTED, "secondary blocks");
                    if (type > 5) return fail(c, PM_ERR_ARG, "unknown nucleotide mutation type");
                    if (type < 3 && (info >> 4) > 6) return fail(c, PM_ERR_UNSUPPORTED, "nucleotide run longer than 6");
                    bases += type >= 3 ? 1 : (int64_t)(info >> 4);
                    rec.node.push_back(v);
                    rec.primary.push_back(p->nuc_mut_primary[k]);
                    rec.pos.push_back(p->nuc_mut_position[k]);
                    rec.gap.push_back(p->nuc_mut_gap_position[k]);
                    rec.info.push_back((uint8_t)info);
                    rec.nucs.push_back(p->nuc_mut_nucs[k]);
                }
            merged.push_back(v);
            node_rec.push_back((int64_t)rec.node.size());
            node_bases.push_back(node_bases.back() + bases);
        }
        out.bm_off[v + 1] = (int64_t)out.bm_primary.size();
    }
    clock.lap("subnet.host_tree");

    // 3. the device pipeline over the merged nodes' records
    Packed packed;
    if (node_bases.back() > 0) {
        RankTables tab;
        int rc = rank_tables(c, p, tab);
        if (rc != PM_OK) return rc;
        const hipStream_t s = c->stream;
        Times times;
        const auto u0 = std::chrono::steady_clock::now();
        Dev<int32_t> d_len, d_error, d_count;
        Dev<uint32_t> d_base, d_pos_base;
        Dev<int64_t> d_pos_off;
        hipError_t e = d_len.put(tab.blk_len, s);
        if (e == hipSuccess) e = d_base.put(tab.block_base, s);
        if (e == hipSuccess) e = d_pos_base.put(tab.pos_base, s);
        if (e == hipSuccess) e = d_pos_off.put(tab.pos_off, s);
        if (e == hipSuccess) e = d_error.alloc(1, true, s);
        if (e == hipSuccess) e = d_count.alloc(M, true, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(c, e, "subnet tables");
        times.upload += seconds_since(u0);
        SubnetArgs a{};
        a.blocks = (int32_t)tab.blk_len.size();
        a.blk_len = d_len.p;
        a.block_base = d_base.p;
        a.pos_off = d_pos_off.p;
        a.pos_base = d_pos_base.p;
        a.error = d_error.p;
        int end_bit = 33;   // the key's bits that can be set: 32 of the rank, then the new node's
        while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < M) ++end_bit;
        // batches of whole new nodes; a node above the batch size gets a batch of its own
        const size_t K = merged.size();
        for (size_t k0 = 0; k0 < K;) {
            size_t k1 = k0 + 1;
            while (k1 < K && node_bases[k1 + 1] - node_bases[k0] <= c->subnet_batch_entries) ++k1;
            const int64_t n = node_bases[k1] - node_bases[k0];
            if (n >= (int64_t)0x7fffffff) return fail(c, PM_ERR_UNSUPPORTED, "2^31 or more bases on one merged chain");
            if (n > 0 && (rc = run_batch(c, rec, node_rec[k0], node_rec[k1], n, a, end_bit, d_count.p, packed, times)) != PM_OK)
                return rc;
            k0 = k1;
        }
        const auto d0 = std::chrono::steady_clock::now();
        e = d_count.get(packed.node_count, (size_t)M, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(c, e, "subnet download");
        times.download += seconds_since(d0);
        phase_add("subnet.upload", times.upload);
        phase_add("subnet.expand", times.expand);
        phase_add("subnet.sort", times.sort);
        phase_add("subnet.fold", times.fold);
        phase_add("subnet.group", times.group);
        phase_add("subnet.download", times.download);
    }

    // 4. the new tree's arrays
    copy_blocks(*p, out);
    int64_t at = 0;   // cursor in the packed records (new-node order, as the batches ran)
    for (int32_t v = 0; v < M; ++v) {
        if (t.chain_off[v + 1] - t.chain_off[v] == 1) {
            const int32_t o = t.chain[t.chain_off[v]];
            const int64_t k0 = p->nuc_mut_offsets[o], k1 = p->nuc_mut_offsets[o + 1];
            out.nm_primary.insert(out.nm_primary.end(), p->nuc_mut_primary + k0, p->nuc_mut_primary + k1);
            if (p->nuc_mut_secondary) out.nm_secondary.insert(out.nm_secondary.end(), p->nuc_mut_secondary + k0, p->nuc_mut_secondary + k1);
            else out.nm_secondary.insert(out.nm_secondary.end(), (size_t)(k1 - k0), -1);
            out.nm_pos.insert(out.nm_pos.end(), p->nuc_mut_position + k0, p->nuc_mut_position + k1);
            out.nm_gap.insert(out.nm_gap.end(), p->nuc_mut_gap_position + k0, p->nuc_mut_gap_position + k1);
            out.nm_info.insert(out.nm_info.end(), p->nuc_mut_info + k0, p->nuc_mut_info + k1);
            out.nm_nucs.insert(out.nm_nucs.end(), p->nuc_mut_nucs + k0, p->nuc_mut_nucs + k1);
        } else if (!packed.node_count.empty()) {
            const int64_t n = packed.node_count[v];
            out.nm_primary.insert(out.nm_primary.end(), packed.primary.begin() + at, packed.primary.begin() + at + n);
            out.nm_secondary.insert(out.nm_secondary.end(), (size_t)n, -1);
            out.nm_pos.insert(out.nm_pos.end(), packed.pos.begin() + at, packed.pos.begin() + at + n);
            out.nm_gap.insert(out.nm_gap.end(), packed.gap.begin() + at, packed.gap.begin() + at + n);
            out.nm_info.insert(out.nm_info.end(), packed.info.begin() + at, packed.info.begin() + at + n);
            out.nm_nucs.insert(out.nm_nucs.end(), packed.nucs.begin() + at, packed.nucs.begin() + at + n);
            at += n;
        }
        out.nm_off[v + 1] = (int64_t)out.nm_primary.size();
    }
    if (at != (int64_t)packed.primary.size()) return fail(c, PM_ERR_STATE, "subnet: record counts per node do not add up");
    clock.lap("subnet.assemble");
    return PM_OK;
}

}  // namespace
}  // namespace pm

extern "C" int pm_subnet(pm_ctx* c, const pm_panmat* p, const char* const* ids, int64_t num_ids, pm_panman** out) {
    if (!c || !p || !out || (!ids && num_ids > 0)) return PM_ERR_ARG;
    return pm::build_handle(c, "subnet", out, [&](pm::PanmanTree& tree) { return pm::subnet(c, p, ids, num_ids, tree); });
}
