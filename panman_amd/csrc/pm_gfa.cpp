// pm_gfa.cpp -- host driver of GFA extraction (Tree::convertToGFA, src/gfa.cpp:3-500; the
// command at src/panmanUtils.cpp:699-732).
//
// The reference walks every tip's path, chops every held block of every tip into 32-column
// chunks and keeps the chunks in one std::map under a mutex.  Here all tips are replayed at
// once (fasta_replay) and the kernels of pm_gfa.hip build the chunk keys from the canonical
// rows, find the distinct ones exactly (radix sort over the whole key, neighbours compared in
// full) and number them in the defined schedule's insertion order.  The chain compaction,
// duplicate removal and renumbering (gfa.cpp:311-472) are restated on the host over the integer
// ids -- they are std::map / std::set walks whose result depends on the iteration order.  "H",
// "S" and "L" are built on the host, where they are small; the "P" lines, one id and a sign per
// chunk of every tip, are counted, scanned and written on the device in batches of whole lines
// and streamed through the pinned download slots.  A PanMAT without a nucleotide mutation takes
// the reference's other branch (gfa.cpp:13-118): whole blocks as segments, presence from a host
// walk, the "P" lines through the same kernels.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "pm_dev.h"
#include "pm_replay.h"

namespace pm {
namespace {

const char kNuc[] = "-ACMGRSVTWYHKDBN";

// ---- gfa.cpp:311-472 over integer ids -----------------------------------------------------------
// A node is (id, strand); a tip is compared by the rank of its name's bytes.
using Node = std::pair<int64_t, bool>;
using Arc = std::pair<int32_t, Node>;   // (tip's name rank, neighbour)
using Graph = std::map<Node, std::vector<Arc>>;

struct Compacted {
    std::vector<int32_t> printed;   // [2 * nodes]: the printed id of (id, strand), -1 when dropped
    std::string text;               // "H", "S" and "L" lines
};

Compacted compact(const std::vector<std::string>& node_text, const std::vector<uint8_t>& node_forward,
                  const std::vector<int32_t>& tip_off, const std::vector<int32_t>& step_id,
                  const std::vector<uint8_t>& step_forward, const std::vector<int32_t>& name_rank) {
    const int64_t nodes = (int64_t)node_text.size();
    const int32_t tips = (int32_t)name_rank.size();
    std::map<Node, std::string> finals;   // finalNodes, keyed (id, creator strand)
    for (int64_t id = 0; id < nodes; ++id) finals[Node(id, node_forward[(size_t)id] != 0)] = node_text[(size_t)id];
    Graph G, GT;
    for (int32_t t = 0; t < tips; ++t)
        for (int32_t s = tip_off[t] + 1; s < tip_off[t + 1]; ++s) {
            const Node from(step_id[s - 1], step_forward[s - 1] != 0), to(step_id[s], step_forward[s] != 0);
            G[from].push_back(Arc(name_rank[t], to));
            GT[to].push_back(Arc(name_rank[t], from));
        }
    for (auto& u : G) std::sort(u.second.begin(), u.second.end());
    for (auto& u : GT) std::sort(u.second.begin(), u.second.end());
    // the merge loop (:343-409): operator[] inserts into G and GT while G is walked, as there
    for (auto& u : G) {
        if (finals.find(u.first) == finals.end()) continue;
        while (true) {
            if (u.second.size() != GT[u.first].size() || u.second.empty()) break;
            bool check = true;
            for (size_t j = 0; j < u.second.size(); ++j) {
                if (u.second[j].first != GT[u.first][j].first) {
                    check = false;
                    break;
                } else if (j > 0 && u.second[j].second != u.second[j - 1].second) {
                    check = false;
                    break;
                }
            }
            if (!check) break;
            const Node dest = u.second[0].second;
            if (u.second.size() != GT[dest].size()) break;
            if (u.first.second != dest.second) break;
            for (size_t j = 0; j < u.second.size(); ++j)
                if (u.second[j].first != GT[dest][j].first && GT[dest][j].second != u.first) {   // (the && of :379)
                    check = false;
                    break;
                }
            if (G[dest].size() != GT[dest].size()) break;
            for (size_t j = 0; j < GT[dest].size(); ++j)
                if (G[dest][j].first != GT[dest][j].first) {
                    check = false;
                    break;
                }
            if (!check) break;
            if (u.first.second) {
                const std::string tail = finals[dest];   // (inserts an empty text for a missing dest, erased below)
                finals[u.first] += tail;
            } else {
                const std::string head = finals[dest];
                finals[u.first] = head + finals[u.first];
            }
            finals.erase(dest);
            u.second.clear();
            const std::vector<Arc> next = G[dest];   // (dest == u.first: the cleared list)
            u.second = next;
        }
    }
    // duplicates (:411-424): the last node in finals order with a text wins
    std::map<std::string, int64_t> text_id;
    int64_t ctr = 1;
    for (const auto& u : finals) text_id[u.second] = ctr++;
    std::unordered_map<int64_t, int64_t> old_new;
    for (const auto& u : finals) old_new[u.first.first] = text_id[u.second];
    std::set<std::pair<Node, Node>> edges;
    for (const auto& u : G) {
        if (finals.find(u.first) == finals.end()) continue;
        for (const Arc& arc : u.second) {
            if (finals.find(arc.second) == finals.end()) continue;
            edges.insert({Node(old_new[u.first.first], u.first.second), Node(old_new[arc.second.first], arc.second.second)});
        }
    }
    std::unordered_map<int64_t, int64_t> sequential;   // (:464-472) from 1 in finals order
    int64_t current = 1;
    for (const auto& u : finals) {
        const int64_t nn = old_new[u.first.first];
        if (sequential.find(nn) == sequential.end()) sequential[nn] = current++;
    }
    Compacted out;
    out.printed.assign((size_t)(2 * nodes), -1);   // the path filter (:442-454): steps outside finals are dropped
    for (const auto& u : finals)
        if (u.first.first < nodes) out.printed[(size_t)(2 * u.first.first + (u.first.second ? 1 : 0))] = (int32_t)sequential[old_new[u.first.first]];
    out.text = "H\tVN:Z:1.1\n";
    std::unordered_map<int64_t, bool> done;
    for (const auto& u : finals) {
        const int64_t nn = old_new[u.first.first];
        if (done[nn]) continue;
        done[nn] = true;
        out.text += "S\t" + std::to_string(sequential[nn]) + "\t" + u.second + "\n";
    }
    for (const auto& e : edges)
        out.text += "L\t" + std::to_string(sequential[e.first.first]) + "\t" + (e.first.second ? "+" : "-") + "\t" +
                    std::to_string(sequential[e.second.first]) + "\t" + (e.second.second ? "+" : "-") + "\t0M\n";
    return out;
}

// ---- the "P" lines of the steps on the device, in batches of whole lines ------------------------
struct Paths {
    int64_t steps = 0;
    Dev<int32_t> id, tip, tip_off, printed;
    Dev<uint8_t> forward;
    std::vector<int32_t> tip_off_host;
};

int write_paths(pm_ctx* c, const ReplayState& r, const Paths& ph, const Sink& sink, int64_t& written) {
    const int32_t L = (int32_t)r.leaves.size();
    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    std::vector<int64_t> name_off;
    std::vector<char> names;
    tip_names(r, name_off, names);
    Dev<int64_t> d_name_off, d_step_len, d_step_off, d_line_len, d_line_off;
    Dev<char> d_names;
    if (d_name_off.put(name_off, st) != hipSuccess || d_names.put(names, st) != hipSuccess ||
        d_step_len.alloc((size_t)ph.steps + 1, false, st) != hipSuccess ||
        d_step_off.alloc((size_t)ph.steps + 1, false, st) != hipSuccess || d_line_len.alloc((size_t)L, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "GFA path tables");
    GfaText t{};
    t.steps = ph.steps;
    t.tips = L;
    t.id = ph.id.p;
    t.forward = ph.forward.p;
    t.tip = ph.tip.p;
    t.tip_off = ph.tip_off.p;
    t.printed = ph.printed.p;
    t.step_len = d_step_len.p;
    t.step_off = d_step_off.p;
    t.name_off = d_name_off.p;
    t.names = d_names.p;
    t.line_len = d_line_len.p;
    auto t0 = std::chrono::steady_clock::now();
    std::vector<int64_t> len;
    if ((e = launch_gfa_step_len(c, t)) != hipSuccess || (e = exclusive_scan(c, d_step_len.p, d_step_off.p, ph.steps + 1)) != hipSuccess ||
        (e = launch_gfa_line_len(c, t)) != hipSuccess || (e = d_line_len.get(len, (size_t)L, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "GFA line lengths");
    // batches of whole lines: tips under the byte limit (at least one line)
    const std::vector<Batch> batches = cut_batches(len, c->gfa_batch_bytes);
    int64_t most = 0;
    for (const Batch& b : batches) most = std::max(most, b.i1 - b.i0);
    if (d_line_off.alloc((size_t)most, false, st) != hipSuccess) return fail(c, PM_ERR_OOM, "GFA line offsets");
    double t_text = seconds_since(t0), t_down = 0.0;
    for (const Batch& b : batches) {
        t0 = std::chrono::steady_clock::now();
        if (grow_device(&c->text_buf, &c->text_cap, (size_t)std::max<int64_t>(b.bytes, 1)) != hipSuccess)
            return fail(c, PM_ERR_OOM, "GFA text");
        if ((e = exclusive_scan(c, d_line_len.p + b.i0, d_line_off.p, b.i1 - b.i0)) != hipSuccess ||
            (e = launch_gfa_write(c, t, (int32_t)b.i0, (int32_t)b.i1, d_line_off.p, static_cast<char*>(c->text_buf),
                                  (int64_t)ph.tip_off_host[(size_t)b.i1] - ph.tip_off_host[(size_t)b.i0])) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "GFA text kernel");
        t_text += seconds_since(t0);
        const int rc = stream_text(c, "GFA", b.bytes, sink, written, t_down);
        if (rc != PM_OK) return rc;
    }
    phase_add("gfa.text", t_text);
    phase_add("gfa.download_write", t_down);
    return PM_OK;
}

// ---- branch A (gfa.cpp:13-118): whole blocks ------------------------------------------------------
int whole_blocks(pm_ctx* c, const pm_panmat* p, const ReplayState& r, std::string& head, Paths& ph) {
    const int32_t L = (int32_t)r.leaves.size(), B = p->num_blocks;
    // segments keyed by primary id (the last block of an id wins), numbered from 0 in id order
    std::map<int32_t, std::string> segment;
    for (int32_t b = 0; b < B; ++b) {
        std::string s;
        for (int64_t w = p->block_seq_offsets[b]; w < p->block_seq_offsets[b + 1]; ++w)
            for (int k = 0; k < 8; ++k) {   // (:20-29: a code 0 ends the word, not the block)
                const int code = (int)((p->block_seq[w] >> (4 * (7 - k))) & 15);
                if (code == 0) break;
                s += kNuc[code];
            }
        segment[p->block_primary[b]] = s;
    }
    std::map<int32_t, int32_t> rank;
    for (const auto& sgm : segment) {
        const int32_t k = (int32_t)rank.size();
        rank[sgm.first] = k;
    }
    auto printed_id = [&](int32_t block) {   // nodeIds[...]: an id that is no block's reads as 0
        const auto it = rank.find(block);
        return it == rank.end() ? 0 : it->second;
    };
    // presence by its own rule (:60-80): an insertion sets, anything else clears
    std::vector<int32_t> step_id, step_tip, tip_off(L + 1, 0);
    std::set<std::pair<int32_t, int32_t>> links;
    std::vector<uint8_t> present((size_t)B + 1);
    std::vector<int32_t> path;
    for (int32_t li = 0; li < L; ++li) {
        std::fill(present.begin(), present.end(), 0);
        path.clear();
        for (int32_t n = r.leaves[li]; n >= 0; n = r.parent[n]) path.push_back(n);
        for (size_t i = path.size(); i-- > 0;)
            for (int64_t k = p->block_mut_offsets[path[i]]; k < p->block_mut_offsets[path[i] + 1]; ++k)
                present[(size_t)p->block_mut_primary[k]] = p->block_mut_info[k] ? 1 : 0;   // (ids checked by the caller)
        int32_t before = -1;
        for (int32_t i = 0; i <= B; ++i) {
            if (!present[(size_t)i]) continue;
            if (step_id.size() >= (size_t)0x7fffffff) return fail(c, PM_ERR_UNSUPPORTED, "GFA paths of 2^31 steps and more");
            step_id.push_back(printed_id(i));
            step_tip.push_back(li);
            if (before >= 0) links.insert({before, i});
            before = i;
        }
        tip_off[li + 1] = (int32_t)step_id.size();
    }
    for (const auto& sgm : segment) head += "S\t" + std::to_string(rank[sgm.first]) + "\t" + sgm.second + "\n";
    for (const auto& l : links)
        head += "L\t" + std::to_string(printed_id(l.first)) + "\t+\t" + std::to_string(printed_id(l.second)) + "\t+\t0M\n";
    std::vector<int32_t> printed(2 * rank.size(), -1);
    for (size_t k = 0; k < rank.size(); ++k) printed[2 * k + 1] = (int32_t)k;
    ph.steps = (int64_t)step_id.size();
    hipStream_t st = c->stream;
    if (ph.id.put(step_id, st) != hipSuccess || ph.tip.put(step_tip, st) != hipSuccess || ph.tip_off.put(tip_off, st) != hipSuccess ||
        ph.printed.put(printed, st) != hipSuccess || ph.forward.put(std::vector<uint8_t>(step_id.size(), 1), st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)   // (the vectors are released on return)
        return fail(c, PM_ERR_OOM, "GFA block paths");
    ph.tip_off_host = std::move(tip_off);
    return PM_OK;
}

// ---- branch B (gfa.cpp:119-499): 32-column chunks of the replayed rows ------------------------------
int chunk_graph(pm_ctx* c, const ReplayState& r, PhaseClock& clock, std::string& head, Paths& ph) {
    const int32_t L = (int32_t)r.leaves.size();
    const int32_t M = r.max_id + 1;
    if (r.columns >= (int64_t)1 << 31) return fail(c, PM_ERR_UNSUPPORTED, "GFA rows of 2^31 columns and more");
    // ---- host tables: held / strand per (tip, block); per block its chunks and their start codes
    const std::vector<uint8_t> held = held_table(r);
    std::vector<int32_t> chunk_off(M + 1, 0), chunk_blk;
    for (int32_t id = 0; id < M; ++id) {
        const int64_t n = r.is_block[id] ? gfa_chunks(r.width[id]) : 0;
        if (chunk_off[id] + n > (int64_t)0x7fffffff) return fail(c, PM_ERR_UNSUPPORTED, "GFA paths of 2^31 steps and more");
        chunk_off[id + 1] = (int32_t)(chunk_off[id] + n);
        chunk_blk.insert(chunk_blk.end(), (size_t)n, id);
    }
    const int32_t CT = chunk_off[M];
    const int64_t items = (int64_t)L * CT;
    if (items >= (int64_t)1 << 31) return fail(c, PM_ERR_UNSUPPORTED, "GFA paths of 2^31 steps and more");
    // The start tuple of a chunk is (first, position, gap slot) of one column; (position, gap
    // slot) is the column itself.  first = block on the forward strand; on the reverse strand
    // -block - 1 for a main character and -block for a gap slot: separate from every forward
    // first except -0 = 0, block 0's gap slots (:253), which therefore share the forward code.
    std::vector<uint32_t> start_code((size_t)2 * CT);
    for (int32_t id = 0; id < M; ++id) {
        const int64_t lo = r.col_start[id], hi = lo + r.width[id];
        for (int32_t k = chunk_off[id]; k < chunk_off[id + 1]; ++k) {
            const int64_t ck = k - chunk_off[id];
            start_code[(size_t)k] = (uint32_t)(lo + kGfaNode * ck);
            const int64_t low = std::max(lo, hi - kGfaNode * (ck + 1));   // the last visited column
            const bool main_char = std::binary_search(r.main_col[id].begin(), r.main_col[id].end(), low);
            start_code[(size_t)CT + k] = (uint32_t)low | (id == 0 && !main_char ? 0u : kGfaReverseStart);
        }
    }
    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    Dev<uint8_t> d_held;
    Dev<int32_t> d_chunk_off, d_chunk_blk;
    Dev<uint32_t> d_start;
    Dev<uint64_t> d_key;
    Dev<int64_t> d_flag, d_scan;
    if (d_held.put(held, st) != hipSuccess || d_chunk_off.put(chunk_off, st) != hipSuccess ||
        d_chunk_blk.put(chunk_blk, st) != hipSuccess || d_start.put(start_code, st) != hipSuccess ||
        d_key.alloc((size_t)(3 * items), false, st) != hipSuccess || d_flag.alloc((size_t)items, false, st) != hipSuccess ||
        d_scan.alloc((size_t)items, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "GFA chunk tables");
    GfaArgs a{};
    a.rows = r.d_rows;
    a.row_stride = r.dev.row_stride;
    a.tips = L;
    a.blocks = M;
    a.blk_lo = r.d_blk_lo;
    a.blk_hi = r.d_blk_hi;
    a.held = d_held.p;
    a.chunks = CT;
    a.chunk_off = d_chunk_off.p;
    a.chunk_blk = d_chunk_blk.p;
    a.start_code = d_start.p;
    a.items = items;
    a.key = d_key.p;
    a.flag = d_flag.p;
    int64_t last[2] = {0, 0};   // the scan and the flag of the last item
    if ((e = launch_gfa_chunk(c, a)) != hipSuccess || (e = exclusive_scan(c, d_flag.p, d_scan.p, items)) != hipSuccess ||
        (items && ((e = hipMemcpyAsync(&last[0], d_scan.p + items - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st)) != hipSuccess ||
                   (e = hipMemcpyAsync(&last[1], d_flag.p + items - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st)) != hipSuccess)) ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "GFA chunks");
    const int64_t S = last[0] + last[1];
    clock.lap("gfa.chunk");

    // ---- the steps, the exact unique over their keys, the ids in insertion order ---------------------
    Dev<uint64_t> d_skey, d_nkey, d_scratch;
    Dev<uint32_t> d_perm;
    Dev<int32_t> d_run_first;
    Dev<uint8_t> d_nforward;
    Dev<int64_t> d_head, d_creator, d_hscan, d_cscan;
    if (d_skey.alloc((size_t)(3 * S), false, st) != hipSuccess || ph.tip.alloc((size_t)S, false, st) != hipSuccess ||
        ph.forward.alloc((size_t)S, false, st) != hipSuccess || ph.tip_off.alloc((size_t)L + 1, true, st) != hipSuccess ||
        ph.id.alloc((size_t)S, false, st) != hipSuccess || d_perm.alloc((size_t)S, false, st) != hipSuccess ||
        d_scratch.alloc((size_t)(4 * S), false, st) != hipSuccess || d_head.alloc((size_t)S, false, st) != hipSuccess ||
        d_creator.alloc((size_t)S, true, st) != hipSuccess || d_hscan.alloc((size_t)S, false, st) != hipSuccess ||
        d_cscan.alloc((size_t)S, false, st) != hipSuccess || d_run_first.alloc((size_t)S, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "GFA steps");
    GfaSteps s{};
    s.steps = S;
    s.key = d_skey.p;
    s.tip = ph.tip.p;
    s.forward = ph.forward.p;
    s.tip_off = ph.tip_off.p;
    s.id = ph.id.p;
    int64_t tail[2] = {0, 0};
    if ((e = launch_gfa_compact(c, a, d_scan.p, s)) != hipSuccess || (e = gfa_sort(c, s, d_perm.p, d_scratch.p)) != hipSuccess ||
        (e = launch_gfa_heads(c, s, d_perm.p, d_head.p, d_creator.p)) != hipSuccess ||
        (e = exclusive_scan(c, d_head.p, d_hscan.p, S)) != hipSuccess || (e = exclusive_scan(c, d_creator.p, d_cscan.p, S)) != hipSuccess ||
        (e = launch_gfa_runs(c, s, d_perm.p, d_head.p, d_hscan.p, d_run_first.p)) != hipSuccess ||
        (S && ((e = hipMemcpyAsync(&tail[0], d_cscan.p + S - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st)) != hipSuccess ||
               (e = hipMemcpyAsync(&tail[1], d_creator.p + S - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st)) != hipSuccess)) ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "GFA unique");
    d_key.reset();
    d_flag.reset();
    d_scan.reset();
    d_scratch.reset();
    const int64_t U = tail[0] + tail[1];
    if (d_nkey.alloc((size_t)(3 * U), false, st) != hipSuccess || d_nforward.alloc((size_t)U, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "GFA nodes");
    GfaNodes nd{};
    nd.key = d_nkey.p;
    nd.forward = d_nforward.p;
    nd.nodes = U;
    std::vector<uint64_t> nkey;
    std::vector<uint8_t> nforward, step_forward;
    std::vector<int32_t> step_id;
    if ((e = launch_gfa_ids(c, s, d_perm.p, d_head.p, d_hscan.p, d_run_first.p, d_cscan.p, nd)) != hipSuccess ||
        (e = d_nkey.get(nkey, (size_t)(3 * U), st)) != hipSuccess || (e = d_nforward.get(nforward, (size_t)U, st)) != hipSuccess ||
        (e = ph.id.get(step_id, (size_t)S, st)) != hipSuccess || (e = ph.forward.get(step_forward, (size_t)S, st)) != hipSuccess ||
        (e = ph.tip_off.get(ph.tip_off_host, (size_t)L + 1, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "GFA ids");
    ph.steps = S;
    clock.lap("gfa.unique");
    phase_add("gfa.items", (double)items);   // (counts)
    phase_add("gfa.steps", (double)S);
    phase_add("gfa.nodes", (double)U);

    // ---- the literal compaction on the host ----------------------------------------------------------
    std::vector<std::string> node_text((size_t)U);
    for (int64_t id = 0; id < U; ++id) {
        const uint32_t len = (uint32_t)(nkey[(size_t)id] & 0xffffffffu);
        std::string& tx = node_text[(size_t)id];
        tx.resize(len);
        for (uint32_t k = 0; k < len; ++k) {
            const uint64_t w = nkey[(size_t)((k < 16 ? 1 : 2) * U + id)];
            tx[k] = kNuc[(w >> (60 - 4 * (k & 15u))) & 15u];
        }
    }
    // tips compare by their name bytes wherever the reference compares names: equal names, equal rank
    std::vector<int32_t> by_name(L), name_rank(L);
    for (int32_t li = 0; li < L; ++li) by_name[li] = li;
    std::sort(by_name.begin(), by_name.end(), [&](int32_t x, int32_t y) { return r.names[r.leaves[x]] < r.names[r.leaves[y]]; });
    for (int32_t k = 0; k < L; ++k)
        name_rank[by_name[k]] = k > 0 && r.names[r.leaves[by_name[k]]] == r.names[r.leaves[by_name[k - 1]]] ? name_rank[by_name[k - 1]] : k;
    Compacted cp = compact(node_text, nforward, ph.tip_off_host, step_id, step_forward, name_rank);
    head = std::move(cp.text);
    if (ph.printed.put(cp.printed, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "GFA printed ids");
    clock.lap("gfa.compact_host");
    return PM_OK;
}

int gfa_steps(pm_ctx* c, const pm_panmat* p, const Sink& sink, int64_t* length) {
    if (!c) return PM_ERR_ARG;
    if (!p || p->num_nodes < 1 || !p->child_offsets || !p->names) return fail(c, PM_ERR_ARG, "bad arguments");
    (void)hipSetDevice(c->device);
    const int64_t nuc = p->nuc_mut_offsets ? p->nuc_mut_offsets[p->num_nodes] : 0;
    if (has_secondary_mutation(p)) return fail(c, PM_ERR_UNSUPPORTED, "secondary blocks");
    const bool blocks_only = nuc == 0;   // (:6-13) no node has a nucleotide mutation
    if (blocks_only && p->block_mut_offsets)   // blockExistsGlobal has blocks.size() + 1 entries (:34)
        for (int64_t k = 0; k < p->block_mut_offsets[p->num_nodes]; ++k)
            if (p->block_mut_primary[k] < 0 || p->block_mut_primary[k] > p->num_blocks)
                return fail(c, PM_ERR_ARG, "GFA of whole blocks: block id beyond the block list");
    PhaseClock clock;
    const int rc = fasta_replay(c, p);
    if (rc != PM_OK) return rc;
    clock.lap("gfa.replay");
    const ReplayState& r = *c->replay;
    if (r.leaves.empty()) return fail(c, PM_ERR_ARG, "GFA needs a tip");
    std::string head;
    Paths ph;
    const int built = blocks_only ? whole_blocks(c, p, r, head, ph) : chunk_graph(c, r, clock, head, ph);
    if (built != PM_OK) return built;
    int64_t written = 0;
    if (!head.empty() && !sink(head.data(), head.size())) return write_failed(c, "GFA");
    written += (int64_t)head.size();
    const int wrc = write_paths(c, r, ph, sink, written);
    if (wrc != PM_OK) return wrc;
    phase_add("gfa.text_bytes", (double)written);   // (a count)
    if (length) *length = written;
    return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_gfa_fd(pm_ctx* c, const pm_panmat* p, int fd, int64_t* length) {
    if (!c) return PM_ERR_ARG;
    if (fd < 0) return fail(c, PM_ERR_ARG, "bad file descriptor");
    return guarded(c, "GFA", [&]() { return gfa_steps(c, p, fd_sink(fd), length); });
}

int pm_gfa(pm_ctx* c, const pm_panmat* p, char** text, int64_t* length) {
    if (!c) return PM_ERR_ARG;
    if (!text || !length) return fail(c, PM_ERR_ARG, "bad arguments");
    return collect_text(c, "GFA", text, [&](const Sink& sink) { return gfa_steps(c, p, sink, length); });
}

}  // extern "C"
