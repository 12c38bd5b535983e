// pm_impute.cpp -- host driver of the N imputation (Tree::imputeNs, src/impute.cpp:4-79 up to the
// plan of moves; the --impute command, src/panmanUtils.cpp:328-354).
//
//   1. host: the derived PanMAT of pm_every_node.h with every block inserted forward at the root and
//      the root's nucleotide mutations on blocks the root does not hold taken out; one replay.  Row v
//      is then the walk's curSequence after node v's list (src/impute.cpp:151-163 never looks at the
//      blocks below the root), so originalNucs[v] is read in the row of v's parent.
//   2. device: the substitution pass over every record but the root's (count, scan, pack); the cells
//      of every list sorted to refuse one written twice; the originals under the imputed records.
//   3. host (pm_impute_plan.cpp): census, candidate walk, path steps, block folds.
//   4. device: every (node, candidate) pair's path lists laid out back to back, then pm_subnet's
//      expand / sort / fold, and the folded length per pair; in batches of whole pairs
//      (PM_OPT_IMPUTE_BATCH_ENTRIES).
//   5. host: the winner rule; device: the winners' folds again, regrouped into records and put
//      through the substitution pass (imputeAllSubstitutionsWithNs).
//   6. host: the plan text and the tree with the imputed lists.  The moves are not applied.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pm_build.h"
#include "pm_dev.h"
#include "pm_every_node.h"
#include "pm_impute_plan.h"
#include "pm_replay.h"

namespace pm {
namespace {

struct HostRecs {
    std::vector<int32_t> primary, pos, gap;
    std::vector<uint8_t> info;
    std::vector<uint32_t> nucs;
};

struct DevRecs {
    Dev<int32_t> node, primary, pos, gap;
    Dev<uint8_t> info;
    Dev<uint32_t> nucs;
    hipError_t alloc(int64_t n, hipStream_t s) {
        hipError_t e = node.alloc((size_t)n, false, s);
        if (e == hipSuccess) e = primary.alloc((size_t)n, false, s);
        if (e == hipSuccess) e = pos.alloc((size_t)n, false, s);
        if (e == hipSuccess) e = gap.alloc((size_t)n, false, s);
        if (e == hipSuccess) e = info.alloc((size_t)n, false, s);
        if (e == hipSuccess) e = nucs.alloc((size_t)n, false, s);
        return e;
    }
    ImputeRecs in(int64_t n) const { return ImputeRecs{n, node.p, primary.p, pos.p, gap.p, info.p, nucs.p}; }
    ImputeRecsOut out() const { return ImputeRecsOut{node.p, primary.p, pos.p, gap.p, info.p, nucs.p}; }
    hipError_t get(HostRecs& h, int64_t n, hipStream_t s) const {
        hipError_t e = primary.get(h.primary, (size_t)n, s);
        if (e == hipSuccess) e = pos.get(h.pos, (size_t)n, s);
        if (e == hipSuccess) e = gap.get(h.gap, (size_t)n, s);
        if (e == hipSuccess) e = info.get(h.info, (size_t)n, s);
        if (e == hipSuccess) e = nucs.get(h.nucs, (size_t)n, s);
        return e;
    }
};

// The substitution pass over `in`: the records at `out` (allocated here), their number, the scanned
// offsets on the host (in.n + 1) and the bases dropped.
int rewrite(pm_ctx* c, const ImputeRecs& in, int64_t keep0, int64_t keep1, DevRecs& out, int64_t& records, std::vector<int64_t>& off,
            int64_t& imputed) {
    const hipStream_t s = c->stream;
    Dev<int64_t> d_off;
    Dev<unsigned long long> d_imputed;
    unsigned long long dropped = 0;
    hipError_t e = d_off.alloc((size_t)in.n + 1, false, s);
    if (e == hipSuccess) e = d_imputed.alloc(1, true, s);
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, "impute offsets");
    e = launch_impute_count(c, in, keep0, keep1, d_off.p, d_imputed.p);
    if (e == hipSuccess) e = exclusive_scan(c, d_off.p, d_off.p, in.n + 1);
    if (e == hipSuccess) e = d_off.get(off, (size_t)in.n + 1, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&dropped, d_imputed.p, sizeof dropped, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute count");
    records = off[(size_t)in.n];
    imputed = (int64_t)dropped;
    if (out.alloc(records, s) != hipSuccess) return fail(c, PM_ERR_OOM, "impute records");
    ImputeRecsOut o = out.out();
    if (!in.node) o.node = nullptr;
    e = launch_impute_pack(c, in, keep0, keep1, d_off.p, o);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute pack");
    return PM_OK;
}

// What the pair batches share.
struct PairWork {
    const ImputePlan* plan;
    const std::vector<int64_t>* im_off;     // [nodes + 1] the imputed lists' records
    const std::vector<int64_t>* im_bases;   // [nodes] their bases
    ImputeRecs imputed;
    const uint32_t* orig;
    SubnetArgs tables;
};

struct PairLists {   // the winners' new nucleotide lists, pair by pair
    HostRecs recs;
    std::vector<int64_t> off{0};
};

// One batch of whole pairs `which[k0 .. k1)`: their folded lengths into sum[k0 ..), or (lists) their new lists.
int run_pairs(pm_ctx* c, const PairWork& w, const std::vector<int64_t>& which, size_t k0, size_t k1, int64_t bases, int64_t* sum,
              PairLists* lists) {
    const hipStream_t s = c->stream;
    const int64_t P = (int64_t)(k1 - k0);
    std::vector<int64_t> dst_off{0}, src0;
    std::vector<uint8_t> inverted;
    std::vector<int32_t> pair;
    for (size_t k = k0; k < k1; ++k) {
        const ImputePair& pr = w.plan->pairs[(size_t)which[k]];
        for (int64_t t = pr.step0; t < pr.step1; ++t) {
            const ImputeStep& st = w.plan->steps[(size_t)t];
            src0.push_back((*w.im_off)[(size_t)st.node]);
            inverted.push_back(st.inverted);
            pair.push_back((int32_t)(k - k0));
            dst_off.push_back(dst_off.back() + (*w.im_off)[(size_t)st.node + 1] - (*w.im_off)[(size_t)st.node]);
        }
        if (lists) lists->off.push_back(lists->off.back());   // (raised below)
    }
    for (size_t k = k0; k < k1 && sum; ++k) sum[k] = 0;
    const int64_t R = dst_off.back();
    if (R == 0 || bases == 0) return PM_OK;
    Dev<int64_t> d_dst_off, d_src0, d_off;
    Dev<uint8_t> d_inverted;
    Dev<int32_t> d_pair;
    DevRecs dst;
    hipError_t e = d_dst_off.put(dst_off, s);
    if (e == hipSuccess) e = d_src0.put(src0, s);
    if (e == hipSuccess) e = d_inverted.put(inverted, s);
    if (e == hipSuccess) e = d_pair.put(pair, s);
    if (e == hipSuccess) e = dst.alloc(R, s);
    if (e == hipSuccess) e = d_off.alloc((size_t)R + 1, false, s);
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, "impute path records (lower PM_OPT_IMPUTE_BATCH_ENTRIES)");
    const ImputeSteps steps{(int64_t)src0.size(), R, d_dst_off.p, d_src0.p, d_inverted.p, d_pair.p};
    SubnetArgs a = w.tables;
    a.records = R;
    a.rec_node = dst.node.p;
    a.rec_primary = dst.primary.p;
    a.rec_pos = dst.pos.p;
    a.rec_gap = dst.gap.p;
    a.rec_info = dst.info.p;
    a.rec_nucs = dst.nucs.p;
    a.rec_off = d_off.p;
    int32_t bad = 0;
    int64_t n = 0;
    e = launch_impute_steps(c, steps, w.imputed, w.orig, dst.out());
    if (e == hipSuccess) e = launch_subnet_count(c, a);
    if (e == hipSuccess) e = exclusive_scan(c, d_off.p, d_off.p, R + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, a.error, sizeof bad, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&n, d_off.p + R, sizeof n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute paths");
    if (bad) return fail(c, PM_ERR_ARG, coordinate_error(bad));
    if (n != bases) return fail(c, PM_ERR_STATE, "impute: the device counted other bases than the host");
    Dev<uint64_t> key, val, key_alt, val_alt;
    Dev<int32_t> eb, ep, eg;
    if (key.alloc((size_t)n, false, s) != hipSuccess || val.alloc((size_t)n, false, s) != hipSuccess ||
        key_alt.alloc((size_t)n, false, s) != hipSuccess || val_alt.alloc((size_t)n, false, s) != hipSuccess ||
        eb.alloc((size_t)n, false, s) != hipSuccess || ep.alloc((size_t)n, false, s) != hipSuccess || eg.alloc((size_t)n, false, s) != hipSuccess)
        return fail(c, PM_ERR_OOM, "impute entries (lower PM_OPT_IMPUTE_BATCH_ENTRIES)");
    const SubnetEntries ent{n, key.p, val.p, eb.p, ep.p, eg.p};
    int end_bit = 33;   // the key's bits that can be set: 32 of the rank, then the batch's pair index
    while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < P) ++end_bit;
    uint64_t *skey = nullptr, *sval = nullptr;
    e = launch_subnet_expand(c, a, ent);
    if (e == hipSuccess) e = subnet_sort(c, ent, key_alt.p, val_alt.p, end_bit, &skey, &sval);
    if (e != hipSuccess) return hip_fail(c, e, "impute sort");
    Dev<int64_t> alive;
    Dev<uint8_t> tc;
    int64_t m = 0;
    if (alive.alloc((size_t)n + 1, false, s) != hipSuccess || tc.alloc((size_t)n, false, s) != hipSuccess)
        return fail(c, PM_ERR_OOM, "impute fold (lower PM_OPT_IMPUTE_BATCH_ENTRIES)");
    e = launch_subnet_fold(c, skey, sval, n, alive.p, tc.p, a.error);
    if (e == hipSuccess) e = exclusive_scan(c, alive.p, alive.p, n + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, a.error, sizeof bad, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&m, alive.p + n, sizeof m, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute fold");
    if (bad) return fail(c, PM_ERR_STATE, coordinate_error(bad));
    if (m == 0) return PM_OK;   // every coordinate cancelled

    Dev<int32_t> ln, lb, lp, lg;
    Dev<uint8_t> ltc;
    Dev<int64_t> head, start;
    if (ln.alloc((size_t)m, false, s) != hipSuccess || lb.alloc((size_t)m, false, s) != hipSuccess || lp.alloc((size_t)m, false, s) != hipSuccess ||
        lg.alloc((size_t)m, false, s) != hipSuccess || ltc.alloc((size_t)m, false, s) != hipSuccess ||
        head.alloc((size_t)m, false, s) != hipSuccess || start.alloc((size_t)m + 1, false, s) != hipSuccess)
        return fail(c, PM_ERR_OOM, "impute survivors (lower PM_OPT_IMPUTE_BATCH_ENTRIES)");
    const SubnetLive live{m, ln.p, lb.p, lp.p, lg.p, ltc.p, head.p, start.p};
    e = launch_subnet_compact(c, skey, sval, n, alive.p, tc.p, ent, live);
    if (!lists) {
        Dev<unsigned long long> d_sum;
        std::vector<unsigned long long> got;
        if (e == hipSuccess && d_sum.alloc((size_t)P, true, s) != hipSuccess) return fail(c, PM_ERR_OOM, "impute sums");
        if (e == hipSuccess) e = launch_impute_pair_sum(c, live, d_sum.p);
        if (e == hipSuccess) e = d_sum.get(got, (size_t)P, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(c, e, "impute sums");
        for (int64_t k = 0; k < P; ++k) sum[k0 + (size_t)k] = (int64_t)got[(size_t)k];
        return PM_OK;
    }
    // the winners: regroup (the greedy cut at 6), then the substitution pass over the new records
    int64_t recs = 0;
    if (e == hipSuccess) e = subnet_runs(c, live);
    if (e == hipSuccess) e = exclusive_scan(c, start.p, start.p, m + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(&recs, start.p + m, sizeof recs, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute runs");
    DevRecs packed, out;
    Dev<int32_t> d_count;
    std::vector<int32_t> count;
    if (packed.alloc(recs, s) != hipSuccess || d_count.alloc((size_t)P, true, s) != hipSuccess) return fail(c, PM_ERR_OOM, "impute records");
    e = launch_subnet_pack(c, live, SubnetOut{packed.primary.p, packed.pos.p, packed.gap.p, packed.info.p, packed.nucs.p, d_count.p});
    if (e == hipSuccess) e = d_count.get(count, (size_t)P, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute pack");
    ImputeRecs in = packed.in(recs);
    in.node = nullptr;
    std::vector<int64_t> off;
    int64_t kept = 0, dropped = 0;
    int rc = rewrite(c, in, 0, 0, out, kept, off, dropped);
    if (rc != PM_OK) return rc;
    HostRecs got;
    e = out.get(got, kept, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute download");
    lists->recs.primary.insert(lists->recs.primary.end(), got.primary.begin(), got.primary.end());
    lists->recs.pos.insert(lists->recs.pos.end(), got.pos.begin(), got.pos.end());
    lists->recs.gap.insert(lists->recs.gap.end(), got.gap.begin(), got.gap.end());
    lists->recs.info.insert(lists->recs.info.end(), got.info.begin(), got.info.end());
    lists->recs.nucs.insert(lists->recs.nucs.end(), got.nucs.begin(), got.nucs.end());
    // the packed records are in (pair, coordinate) order: pair k's are count[k] records after the earlier pairs'
    const size_t first = lists->off.size() - (size_t)P;
    const int64_t base = lists->off[first - 1];
    int64_t before = 0;
    for (int64_t k = 0; k < P; ++k) {
        before += count[(size_t)k];
        lists->off[first + (size_t)k] = base + off[(size_t)before];
    }
    if (before != recs) return fail(c, PM_ERR_STATE, "impute: record counts per pair do not add up");
    return PM_OK;
}

// `which` in batches of whole pairs of at most PM_OPT_IMPUTE_BATCH_ENTRIES bases; a larger pair runs alone.
int run_all_pairs(pm_ctx* c, const PairWork& w, const std::vector<int64_t>& which, std::vector<int64_t>* sum, PairLists* lists) {
    std::vector<int64_t> bases(which.size() + 1, 0);
    for (size_t k = 0; k < which.size(); ++k) {
        const ImputePair& pr = w.plan->pairs[(size_t)which[k]];
        int64_t b = 0;
        for (int64_t t = pr.step0; t < pr.step1; ++t) b += (*w.im_bases)[(size_t)w.plan->steps[(size_t)t].node];
        bases[k + 1] = bases[k] + b;
    }
    if (sum) sum->assign(which.size(), 0);
    for (size_t k0 = 0; k0 < which.size();) {
        size_t k1 = k0 + 1;
        while (k1 < which.size() && bases[k1 + 1] - bases[k0] <= c->impute_batch_entries) ++k1;
        const int64_t n = bases[k1] - bases[k0];
        if (n >= (int64_t)0x7fffffff) return fail(c, PM_ERR_UNSUPPORTED, "2^31 or more bases on one path");
        const int rc = run_pairs(c, w, which, k0, k1, n, sum ? sum->data() : nullptr, lists);
        if (rc != PM_OK) return rc;
        k0 = k1;
    }
    return PM_OK;
}

void append_line(std::string& text, const std::string& name, const char* rest) {
    text += name;
    text += rest;
}

int impute(pm_ctx* c, const pm_panmat* p, int32_t max_distance, PanmanTree& out, std::string& text, pm_impute_stats& stats) {
    PhaseClock clock;
    std::string err;
    int rc = impute_check(p, err);
    if (rc != PM_OK) return fail(c, rc, err);
    const int32_t N = p->num_nodes, root = p->root;
    const int64_t muts = p->nuc_mut_offsets[N];
    if (p->nuc_mut_offsets[0] != 0) return fail(c, PM_ERR_ARG, "bad offsets");
    if (muts > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "2^31 - 64 nucleotide mutations and more");
    bool any_n = false;
    for (int32_t v = 0; v < N; ++v)
        for (int64_t k = p->nuc_mut_offsets[v]; k < p->nuc_mut_offsets[v + 1]; ++k) {
            const uint32_t info = p->nuc_mut_info[k], type = info & 7u;
            if (type == PM_MUT_ND || type == 5u) {
                // the walk writes getNucleotideFromCode(code) for every record type; the replayed rows hold '-'
                if (p->nuc_mut_nucs[k] >> (24 - 4 * (info >> 4))) return fail(c, PM_ERR_UNSUPPORTED, "a deletion that carries codes");
                continue;
            }
            for (uint32_t i = 0; i < (info >> 4) && v != root; ++i) any_n = any_n || ((p->nuc_mut_nucs[k] >> (4 * (5 - i))) & 15u) == 15u;
        }

    // ---- 1. the rows: the root's nucleotide mutations count only on the blocks it holds
    std::vector<uint8_t> held;
    for (int64_t k = p->block_mut_offsets[root]; k < p->block_mut_offsets[root + 1]; ++k) {
        const int32_t id = p->block_mut_primary[k];
        if (id < 0) return fail(c, PM_ERR_ARG, "negative block id in a block mutation");
        if ((size_t)id >= held.size()) held.resize((size_t)id + 1, 0);
        if (p->block_mut_info[k]) held[(size_t)id] = 1;
        else if (!p->block_mut_inversion[k]) held[(size_t)id] = 0;
    }
    pm_panmat q = *p;
    HostRecs fr;
    std::vector<int32_t> fsecondary;
    std::vector<int64_t> foff;
    const int64_t r0 = p->nuc_mut_offsets[root], r1 = p->nuc_mut_offsets[root + 1];
    int64_t dropped = 0;
    for (int64_t k = r0; k < r1; ++k) {
        const int32_t id = p->nuc_mut_primary[k];
        dropped += !(id >= 0 && (size_t)id < held.size() && held[(size_t)id]);
    }
    if (dropped) {
        for (int64_t k = 0; k < muts; ++k) {
            const int32_t id = p->nuc_mut_primary[k];
            if (k >= r0 && k < r1 && !(id >= 0 && (size_t)id < held.size() && held[(size_t)id])) continue;
            fr.primary.push_back(id);
            fsecondary.push_back(-1);
            fr.pos.push_back(p->nuc_mut_position[k]);
            fr.gap.push_back(p->nuc_mut_gap_position[k]);
            fr.info.push_back(p->nuc_mut_info[k]);
            fr.nucs.push_back(p->nuc_mut_nucs[k]);
        }
        foff.assign(p->nuc_mut_offsets, p->nuc_mut_offsets + N + 1);
        for (int32_t v = 0; v <= N; ++v)
            if (foff[(size_t)v] >= r1) foff[(size_t)v] -= dropped;
        q.nuc_mut_offsets = foff.data();
        q.nuc_mut_primary = fr.primary.data();
        q.nuc_mut_secondary = fsecondary.data();
        q.nuc_mut_position = fr.pos.data();
        q.nuc_mut_gap_position = fr.gap.data();
        q.nuc_mut_info = fr.info.data();
        q.nuc_mut_nucs = fr.nucs.data();
    }
    const EveryNodeATip every(&q, true);
    clock.lap("impute.every_node_host");
    if ((rc = fasta_replay(c, &every.q)) != PM_OK) return rc;   // (refuses a mutation whose cell does not exist: PM_ERR_ARG)
    clock = PhaseClock();
    const ReplayState& r = *c->replay;

    // ---- the tree that comes back: everything but the nucleotide lists is the input's
    Topology topo;
    topo.root = root;
    topo.name.assign(r.names.begin(), r.names.begin() + N);
    topo.kids.resize((size_t)N);
    for (int32_t v = 0; v < N; ++v) topo.kids[(size_t)v].assign(p->child_index + p->child_offsets[v], p->child_index + p->child_offsets[v + 1]);
    if (p->branch_length) topo.length.assign(p->branch_length, p->branch_length + N);
    tree_from_topology(topo, out);
    copy_blocks(*p, out);
    if (p->circular_offset) out.circular.assign(p->circular_offset, p->circular_offset + N);
    if (p->rotation_index) out.rotation.assign(p->rotation_index, p->rotation_index + N);
    if (p->sequence_inverted) out.inverted.assign(p->sequence_inverted, p->sequence_inverted + N);
    const int64_t bm0 = p->block_mut_offsets[0], bm1 = p->block_mut_offsets[N];
    out.bm_primary.assign(p->block_mut_primary + bm0, p->block_mut_primary + bm1);
    out.bm_info.assign(p->block_mut_info + bm0, p->block_mut_info + bm1);
    out.bm_inv.assign(p->block_mut_inversion + bm0, p->block_mut_inversion + bm1);
    for (int32_t v = 0; v <= N; ++v) out.bm_off[(size_t)v] = p->block_mut_offsets[v] - bm0;
    stats = pm_impute_stats{0, 0, 0, 0};
    text.clear();
    if (!any_n) {   // nothing to impute and no insertion run holds an N: no launch after the replay
        out.nm_primary.assign(p->nuc_mut_primary, p->nuc_mut_primary + muts);
        out.nm_secondary.assign((size_t)muts, -1);
        out.nm_pos.assign(p->nuc_mut_position, p->nuc_mut_position + muts);
        out.nm_gap.assign(p->nuc_mut_gap_position, p->nuc_mut_gap_position + muts);
        out.nm_info.assign(p->nuc_mut_info, p->nuc_mut_info + muts);
        out.nm_nucs.assign(p->nuc_mut_nucs, p->nuc_mut_nucs + muts);
        out.nm_off.assign(p->nuc_mut_offsets, p->nuc_mut_offsets + N + 1);
        clock.lap("impute.assemble");
        return PM_OK;
    }

    // ---- 2. the substitution pass, the cells written twice, the originals
    const hipStream_t s = c->stream;
    std::vector<int32_t> mut_node((size_t)muts);
    std::vector<int64_t> node_bases((size_t)N + 1, 0);
    for (int32_t v = 0; v < N; ++v) {
        int64_t b = 0;
        for (int64_t k = p->nuc_mut_offsets[v]; k < p->nuc_mut_offsets[v + 1]; ++k) {
            mut_node[(size_t)k] = v;
            b += p->nuc_mut_info[k] >> 4;
        }
        node_bases[(size_t)v + 1] = node_bases[(size_t)v] + (v == root ? 0 : b);
    }
    RankTables tab;
    if ((rc = rank_tables(c, p, tab)) != PM_OK) return rc;
    DevRecs d_in, d_im;
    Dev<int32_t> d_len, d_error;
    Dev<uint32_t> d_base, d_pos_base;
    Dev<int64_t> d_pos_off;
    hipError_t e = d_in.node.put(mut_node, s);
    if (e == hipSuccess) e = d_in.primary.put(p->nuc_mut_primary, (size_t)muts, s);
    if (e == hipSuccess) e = d_in.pos.put(p->nuc_mut_position, (size_t)muts, s);
    if (e == hipSuccess) e = d_in.gap.put(p->nuc_mut_gap_position, (size_t)muts, s);
    if (e == hipSuccess) e = d_in.info.put(p->nuc_mut_info, (size_t)muts, s);
    if (e == hipSuccess) e = d_in.nucs.put(p->nuc_mut_nucs, (size_t)muts, s);
    if (e == hipSuccess) e = d_len.put(tab.blk_len, s);
    if (e == hipSuccess) e = d_base.put(tab.block_base, s);
    if (e == hipSuccess) e = d_pos_base.put(tab.pos_base, s);
    if (e == hipSuccess) e = d_pos_off.put(tab.pos_off, s);
    if (e == hipSuccess) e = d_error.alloc(1, true, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, PM_ERR_OOM, "impute tables");
    clock.lap("impute.upload");
    SubnetArgs tables{};
    tables.blocks = (int32_t)tab.blk_len.size();
    tables.blk_len = d_len.p;
    tables.block_base = d_base.p;
    tables.pos_off = d_pos_off.p;
    tables.pos_base = d_pos_base.p;
    tables.error = d_error.p;

    int64_t im_records = 0;
    std::vector<int64_t> off;
    if ((rc = rewrite(c, d_in.in(muts), r0, r1, d_im, im_records, off, stats.imputed_bases)) != PM_OK) return rc;
    HostRecs im;
    e = d_im.get(im, im_records, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(c, e, "impute download");
    std::vector<int64_t> im_off((size_t)N + 1), im_bases((size_t)N, 0);
    for (int32_t v = 0; v <= N; ++v) im_off[(size_t)v] = off[(size_t)p->nuc_mut_offsets[v]];
    for (int32_t v = 0; v < N; ++v)
        for (int64_t k = im_off[(size_t)v]; k < im_off[(size_t)v + 1]; ++k) im_bases[(size_t)v] += im.info[(size_t)k] >> 4;
    clock.lap("impute.substitutions");

    // a cell written twice in one list: the cells of whole nodes sorted by (node, rank), batch by batch
    {
        int end_bit = 33;
        while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < N) ++end_bit;
        for (int32_t v0 = 0; v0 < N;) {
            if (v0 == root) {   // (its list is never walked)
                ++v0;
                continue;
            }
            int32_t v1 = v0 + 1;
            while (v1 < N && v1 != root && node_bases[(size_t)v1 + 1] - node_bases[(size_t)v0] <= c->impute_batch_entries) ++v1;
            const int64_t k0 = p->nuc_mut_offsets[v0], R = p->nuc_mut_offsets[v1] - k0, n = node_bases[(size_t)v1] - node_bases[(size_t)v0];
            v0 = v1;
            if (n == 0) continue;
            if (n >= (int64_t)0x7fffffff) return fail(c, PM_ERR_UNSUPPORTED, "2^31 or more bases in one list");
            Dev<int64_t> d_off;
            Dev<uint64_t> key, val, key_alt, val_alt;
            Dev<int32_t> eb, ep, eg;
            if (d_off.alloc((size_t)R + 1, false, s) != hipSuccess || key.alloc((size_t)n, false, s) != hipSuccess ||
                val.alloc((size_t)n, false, s) != hipSuccess || key_alt.alloc((size_t)n, false, s) != hipSuccess ||
                val_alt.alloc((size_t)n, false, s) != hipSuccess || eb.alloc((size_t)n, false, s) != hipSuccess ||
                ep.alloc((size_t)n, false, s) != hipSuccess || eg.alloc((size_t)n, false, s) != hipSuccess)
                return fail(c, PM_ERR_OOM, "impute cells (lower PM_OPT_IMPUTE_BATCH_ENTRIES)");
            SubnetArgs a = tables;
            a.records = R;
            a.rec_node = d_in.node.p + k0;
            a.rec_primary = d_in.primary.p + k0;
            a.rec_pos = d_in.pos.p + k0;
            a.rec_gap = d_in.gap.p + k0;
            a.rec_info = d_in.info.p + k0;
            a.rec_nucs = d_in.nucs.p + k0;
            a.rec_off = d_off.p;
            int32_t bad = 0;
            int64_t total = 0;
            e = launch_subnet_count(c, a);
            if (e == hipSuccess) e = exclusive_scan(c, d_off.p, d_off.p, R + 1);
            if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_error.p, sizeof bad, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(&total, d_off.p + R, sizeof total, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return hip_fail(c, e, "impute cells");
            if (bad) return fail(c, PM_ERR_ARG, coordinate_error(bad));
            if (total != n) return fail(c, PM_ERR_STATE, "impute: the device counted other bases than the host");
            const SubnetEntries ent{n, key.p, val.p, eb.p, ep.p, eg.p};
            uint64_t *skey = nullptr, *sval = nullptr;
            e = launch_subnet_expand(c, a, ent);
            if (e == hipSuccess) e = subnet_sort(c, ent, key_alt.p, val_alt.p, end_bit, &skey, &sval);
            if (e == hipSuccess) e = launch_impute_twice(c, skey, n, d_error.p);
            if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_error.p, sizeof bad, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return hip_fail(c, e, "impute cells");
            if (bad) return fail(c, PM_ERR_UNSUPPORTED, "a cell written twice in one list");
        }
    }
    clock.lap("impute.cells");

    // the originals under the imputed records, read in the parents' rows
    const std::vector<int32_t> row_of = every.rows_of_nodes(r, N);
    std::vector<int32_t> par_row((size_t)N);
    for (int32_t v = 0; v < N; ++v) par_row[(size_t)v] = v == root ? -1 : row_of[(size_t)r.parent[(size_t)v]];
    std::vector<int64_t> pos_off;
    std::vector<int32_t> main_col, gap_col;
    cell_columns(r, pos_off, main_col, gap_col);
    Dev<int32_t> d_par_row, d_main_col, d_gap_col;
    Dev<int64_t> d_cell_off;
    Dev<uint32_t> d_orig;
    if (d_par_row.put(par_row, s) != hipSuccess || d_main_col.put(main_col, s) != hipSuccess || d_gap_col.put(gap_col, s) != hipSuccess ||
        d_cell_off.put(pos_off, s) != hipSuccess || d_orig.alloc((size_t)im_records, false, s) != hipSuccess)
        return fail(c, PM_ERR_OOM, "impute originals");
    {
        const ImputeRows rows{r.d_rows, r.dev.row_stride, r.columns, r.max_id + 1, d_cell_off.p, d_main_col.p, d_gap_col.p, d_par_row.p, d_error.p};
        int32_t bad = 0;
        e = launch_impute_originals(c, d_im.in(im_records), rows, d_orig.p);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_error.p, sizeof bad, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(c, e, "impute originals");
        if (bad) return fail(c, PM_ERR_ARG, "a mutation's cell does not exist");
    }
    clock.lap("impute.originals");

    // ---- 3. the host plan
    ImputePlan plan;
    if ((rc = impute_plan(p, max_distance, plan, err)) != PM_OK) return fail(c, rc, err);
    clock.lap("impute.plan_host");

    // ---- 4. every pair's folded length; 5. the winners and their lists
    const PairWork work{&plan, &im_off, &im_bases, d_im.in(im_records), d_orig.p, tables};
    std::vector<int64_t> all(plan.pairs.size()), sum, winners;
    for (size_t i = 0; i < all.size(); ++i) all[i] = (int64_t)i;
    if ((rc = run_all_pairs(c, work, all, &sum, nullptr)) != PM_OK) return rc;
    clock.lap("impute.score");
    std::vector<int64_t> improvement(plan.pairs.size()), won(plan.attempts.size(), -1);
    for (size_t i = 0; i < plan.pairs.size(); ++i)
        improvement[i] = im_bases[(size_t)plan.attempts[(size_t)plan.pairs[i].attempt].node] - sum[i];
    for (size_t a = 0; a < plan.attempts.size(); ++a) {
        const ImputeAttempt& at = plan.attempts[a];
        const int64_t best = impute_winner(improvement.data() + at.pair0, plan.pairs.data() + at.pair0, at.pair1 - at.pair0);
        if (best >= 0) {
            won[a] = at.pair0 + best;
            winners.push_back(won[a]);
        }
    }
    PairLists lists;
    if ((rc = run_all_pairs(c, work, winners, nullptr, &lists)) != PM_OK) return rc;
    clock.lap("impute.winners");

    // ---- 6. the plan text and the tree
    stats.insertion_nodes = (int64_t)plan.attempts.size();
    stats.moves_found = (int64_t)winners.size();
    stats.pairs = (int64_t)plan.pairs.size();
    std::vector<ImputeBlockMut> blocks;
    char line[160];
    size_t w = 0;
    for (size_t a = 0; a < plan.attempts.size(); ++a) {
        const ImputeAttempt& at = plan.attempts[a];
        const std::string& name = r.names[(size_t)at.node];
        std::snprintf(line, sizeof line, "\t%d\t%lld\t", at.runs_with_n, (long long)(at.pair1 - at.pair0));
        append_line(text, name, line);
        if (won[a] < 0) {
            text += ".\t-1\t0\n";
            continue;
        }
        const ImputePair& pr = plan.pairs[(size_t)won[a]];
        std::snprintf(line, sizeof line, "\t%lld\t%d\n", (long long)improvement[(size_t)won[a]], pr.block_improvement);
        text += r.names[(size_t)pr.candidate];
        text += line;
        if (!impute_pair_blocks(p, plan, pr, blocks, err)) return fail(c, PM_ERR_ARG, err);
        for (const ImputeBlockMut& b : blocks) {
            std::snprintf(line, sizeof line, "\tB\t%d\t%d\t%d\n", b.primary, (int)b.info, (int)b.inversion);
            append_line(text, name, line);
        }
        for (int64_t k = lists.off[w]; k < lists.off[w + 1]; ++k) {
            std::snprintf(line, sizeof line, "\tN\t%d\t%d\t%d\t%d\t%06x\n", lists.recs.primary[(size_t)k], lists.recs.pos[(size_t)k],
                          lists.recs.gap[(size_t)k], (int)lists.recs.info[(size_t)k], (unsigned)lists.recs.nucs[(size_t)k]);
            append_line(text, name, line);
        }
        ++w;
    }
    out.nm_primary = std::move(im.primary);
    out.nm_secondary.assign((size_t)im_records, -1);
    out.nm_pos = std::move(im.pos);
    out.nm_gap = std::move(im.gap);
    out.nm_info = std::move(im.info);
    out.nm_nucs = std::move(im.nucs);
    out.nm_off = im_off;
    clock.lap("impute.assemble");
    phase_add("impute.pairs", (double)plan.pairs.size());        // (a count)
    phase_add("impute.attempts", (double)plan.attempts.size());  // (a count)
    return PM_OK;
}

}  // namespace
}  // namespace pm

extern "C" int pm_impute(pm_ctx* c, const pm_panmat* p, int32_t max_distance, pm_panman** out, char** plan, int64_t* plan_length,
                         pm_impute_stats* stats) {
    if (!c) return PM_ERR_ARG;
    if (!p || !out || !plan) return pm::fail(c, PM_ERR_ARG, "bad arguments");
    *plan = nullptr;
    if (plan_length) *plan_length = 0;
    std::string text;
    pm_impute_stats st{0, 0, 0, 0};
    const int rc = pm::build_handle(c, "impute", out, [&](pm::PanmanTree& tree) { return pm::impute(c, p, max_distance, tree, text, st); });
    if (rc != PM_OK) return rc;
    char* buf = static_cast<char*>(std::malloc(text.size() + 1));
    if (!buf) {
        pm_panman_free(*out);
        *out = nullptr;
        return pm::fail(c, PM_ERR_OOM, "impute host buffers");
    }
    std::memcpy(buf, text.data(), text.size());
    buf[text.size()] = '\0';
    *plan = buf;
    if (plan_length) *plan_length = (int64_t)text.size();
    if (stats) *stats = st;
    return PM_OK;
}
