// pm_mutations.cpp -- host driver of mutation printing (Tree::printMutationsNew(std::ostream&),
// src/panman.cpp:3699-4057; the --printMutations command, src/panmanUtils.cpp:1008-1071).
//
// The reference replays every node's whole sequence on one thread into maps keyed by (node, block,
// position, slot).  Here the rows of every node come from one replay of the derived PanMAT of
// pm_every_node.h; the kernels of pm_mutations.hip then count the root's coordinates over the
// columns, expand every node's own mutation list into one entry per base, look the parent's
// characters up in the parent's row and write the three lines of every node.  The host keeps the
// (node, block) held / strand table as getSequenceFromReference leaves it (src/panman.cpp:
// 4779-4818), refuses what the reference leaves undefined, cuts the nodes into batches
// (PM_OPT_MUTATIONS_BATCH_BYTES) and streams each batch's lines through the pinned download slots.
#include <algorithm>
#include <string>
#include <vector>

#include "pm_dev.h"
#include "pm_every_node.h"
#include "pm_replay.h"

namespace pm {
namespace {

// [nodes][max_id + 1] kMafHeld | kMafForward after all block mutations of the node's path, in path
// order; false: a block mutation's id is negative.
bool node_block_table(const pm_panmat* p, int32_t M, std::vector<uint8_t>& held) {
    const int32_t N = p->num_nodes;
    held.assign((size_t)N * M, 0);
    std::vector<int32_t> order{p->root};   // parents before children
    order.reserve((size_t)N);
    for (size_t at = 0; at < order.size(); ++at)
        for (int32_t e = p->child_offsets[order[at]]; e < p->child_offsets[order[at] + 1]; ++e) order.push_back(p->child_index[e]);
    std::vector<int32_t> parent((size_t)N, -1);
    for (int32_t v = 0; v < N; ++v)
        for (int32_t e = p->child_offsets[v]; e < p->child_offsets[v + 1]; ++e) parent[(size_t)p->child_index[e]] = v;
    for (const int32_t v : order) {
        uint8_t* h = held.data() + (size_t)v * M;
        if (v == p->root) std::fill(h, h + M, (uint8_t)kMafForward);
        else std::copy(held.data() + (size_t)parent[(size_t)v] * M, held.data() + (size_t)parent[(size_t)v] * M + M, h);
        for (int64_t k = p->block_mut_offsets[v]; k < p->block_mut_offsets[v + 1]; ++k) {
            const int32_t id = p->block_mut_primary[k];
            if (id < 0) return false;
            if (id >= M) continue;   // (no block: the replay has checked the id against blocks + 1)
            if (p->block_mut_info[k]) h[id] = (uint8_t)(kMafHeld | (p->block_mut_inversion[k] ? 0 : kMafForward));
            else if (p->block_mut_inversion[k]) h[id] ^= (uint8_t)kMafForward;
            else h[id] = (uint8_t)kMafForward;
        }
    }
    return true;
}

int mutations_steps(pm_ctx* c, const pm_panmat* p, const Sink& sink, int64_t* length, int64_t* odd_substitutions) {
    if (!c) return PM_ERR_ARG;
    if (!p || p->num_nodes < 1 || !p->child_offsets || !p->names || !p->block_mut_offsets || !p->nuc_mut_offsets ||
        p->root < 0 || p->root >= p->num_nodes)
        return fail(c, PM_ERR_ARG, "bad arguments");
    (void)hipSetDevice(c->device);
    if (has_secondary_mutation(p)) return fail(c, PM_ERR_UNSUPPORTED, "secondary blocks");
    if (length) *length = 0;
    if (odd_substitutions) *odd_substitutions = 0;
    const int32_t N = p->num_nodes;
    for (int32_t v = 0; v < N; ++v)
        if (p->child_offsets[v] > p->child_offsets[v + 1] || p->nuc_mut_offsets[v] > p->nuc_mut_offsets[v + 1])
            return fail(c, PM_ERR_ARG, "bad offsets");

    PhaseClock clock;
    const EveryNodeATip every(p);
    clock.lap("mutations.every_node_host");
    int rc = fasta_replay(c, &every.q);   // (refuses a mutation whose cell does not exist: PM_ERR_ARG)
    if (rc != PM_OK) return rc;
    clock = PhaseClock();
    const ReplayState& r = *c->replay;
    const int32_t M = r.max_id + 1;
    if (r.columns > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "mutation rows of 2^31 - 64 columns and more");
    const int64_t muts = p->nuc_mut_offsets[N];
    if (muts > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "2^31 nucleotide mutations and more");

    // ---- host tables: held / strand per (node, block), the unsupported check, positions' columns
    std::vector<uint8_t> held;
    if (!node_block_table(p, M, held)) return fail(c, PM_ERR_ARG, "block mutation id out of range");
    for (int32_t v = 0; v < N; ++v)
        for (int32_t id = 0; id < M; ++id)
            if (r.is_block[id] && held[(size_t)v * M + id] == 0)
                return fail(c, PM_ERR_UNSUPPORTED, "a node ends its path with a block it does not hold flagged reverse");
    const std::vector<int32_t> row_of = every.rows_of_nodes(r, N);
    std::vector<int64_t> pos_off;
    std::vector<int32_t> main_col, gap_col;
    cell_columns(r, pos_off, main_col, gap_col);
    std::vector<uint8_t> col_held((size_t)r.columns, 0);
    host_parallel_for(M, [&](int id) {
        if (!r.is_block[id]) return;
        if (held[(size_t)p->root * M + id] & kMafHeld)
            std::fill(col_held.begin() + r.col_start[id], col_held.begin() + r.col_start[id] + r.width[id], (uint8_t)1);
    });
    std::vector<char> names;
    std::vector<int64_t> name_at;
    node_names(r, N, name_at, names);
    // the node of every mutation and every node's elements (the root's list prints nothing)
    std::vector<int32_t> mut_node((size_t)muts);
    std::vector<int64_t> node_entries((size_t)N, 0);
    host_parallel_for((N + 15) / 16, [&](int task) {
        for (int32_t v = task * 16; v < std::min(N, task * 16 + 16); ++v)
            for (int64_t k = p->nuc_mut_offsets[v]; k < p->nuc_mut_offsets[v + 1]; ++k) {
                mut_node[(size_t)k] = v;
                const uint32_t info = p->nuc_mut_info[k], type = info & 7u;
                if (v != p->root) node_entries[(size_t)v] += type < 3u ? (int64_t)(info >> 4) : type == 3u ? 1 : 0;
            }
    });

    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    const int64_t chunks = (r.columns + kMutChunk - 1) / kMutChunk;
    Dev<uint8_t> d_held, d_col_held, d_info;
    Dev<int32_t> d_row_of, d_main_col, d_gap_col, d_before, d_mut_node, d_primary, d_position, d_gap, d_error;
    Dev<uint32_t> d_nucs;
    Dev<int64_t> d_pos_off, d_chunk, d_name_at, d_node_mut;
    Dev<unsigned long long> d_odd;
    Dev<char> d_names;
    if ((e = d_held.put(held, st)) != hipSuccess || (e = d_col_held.put(col_held, st)) != hipSuccess ||
        (e = d_row_of.put(row_of, st)) != hipSuccess || (e = d_main_col.put(main_col, st)) != hipSuccess ||
        (e = d_gap_col.put(gap_col, st)) != hipSuccess || (e = d_pos_off.put(pos_off, st)) != hipSuccess ||
        (e = d_chunk.alloc((size_t)chunks, false, st)) != hipSuccess || (e = d_before.alloc((size_t)r.columns + 1, false, st)) != hipSuccess ||
        (e = d_mut_node.put(mut_node, st)) != hipSuccess || (e = d_primary.put(p->nuc_mut_primary, (size_t)muts, st)) != hipSuccess ||
        (e = d_position.put(p->nuc_mut_position, (size_t)muts, st)) != hipSuccess ||
        (e = d_gap.put(p->nuc_mut_gap_position, (size_t)muts, st)) != hipSuccess ||
        (e = d_info.put(p->nuc_mut_info, (size_t)muts, st)) != hipSuccess || (e = d_nucs.put(p->nuc_mut_nucs, (size_t)muts, st)) != hipSuccess ||
        (e = d_node_mut.put(p->nuc_mut_offsets, (size_t)N + 1, st)) != hipSuccess || (e = d_name_at.put(name_at, st)) != hipSuccess ||
        (e = d_names.put(names, st)) != hipSuccess || (e = d_odd.alloc(1, true, st)) != hipSuccess ||
        (e = d_error.alloc(1, true, st)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "mutation tables");
    MutArgs a{};
    a.rows = r.d_rows;
    a.row_stride = r.dev.row_stride;
    a.columns = r.columns;
    a.nodes = N;
    a.blocks = M;
    a.root = p->root;
    a.row_of = d_row_of.p;
    a.parent = r.d_parent;   // (the derived PanMAT's: the nodes of `p` keep their ids and parents)
    a.held = d_held.p;
    a.blk_lo = r.d_blk_lo;
    a.blk_hi = r.d_blk_hi;
    a.pos_off = d_pos_off.p;
    a.main_col = d_main_col.p;
    a.gap_col = d_gap_col.p;
    a.col_held = d_col_held.p;
    a.chunk = d_chunk.p;
    a.before = d_before.p;
    a.mut_node = d_mut_node.p;
    a.mut_primary = d_primary.p;
    a.mut_position = d_position.p;
    a.mut_gap = d_gap.p;
    a.mut_info = d_info.p;
    a.mut_nucs = d_nucs.p;
    a.odd = d_odd.p;
    a.error = d_error.p;
    clock.lap("mutations.tables_host");

    // ---- the root map: once per call
    if ((e = launch_mut_root_map(c, a)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "mutation root map");
    clock.lap("mutations.root_map");

    // ---- batches of nodes in id order: the entry records, the scan arrays and the largest text
    std::vector<int64_t> bound((size_t)N);
    for (int32_t v = 0; v < N; ++v)   // a record and " > g" old, ten digits, new per entry; three heads and names
        bound[(size_t)v] = node_entries[(size_t)v] * (int64_t)(sizeof(MutEntry) + 16) +
                           (p->nuc_mut_offsets[v + 1] - p->nuc_mut_offsets[v]) * 8 + 3 * (name_at[(size_t)v + 1] - name_at[(size_t)v] + 17) + 24;
    // (a launch takes three workgroups a node)
    const std::vector<Batch> batches = cut_batches(bound, c->mutations_batch_bytes, [](int64_t) { return (int64_t)3; }, (int64_t)0x7fffffff);
    int64_t most_nodes = 0, most_muts = 0, most_entries = 0;
    std::vector<int64_t> batch_entries;
    for (const Batch& b : batches) {
        int64_t n = 0;
        for (int64_t v = b.i0; v < b.i1; ++v) n += node_entries[(size_t)v];
        batch_entries.push_back(n);
        most_nodes = std::max(most_nodes, b.i1 - b.i0);
        most_muts = std::max(most_muts, p->nuc_mut_offsets[b.i1] - p->nuc_mut_offsets[b.i0]);
        most_entries = std::max(most_entries, n);
    }
    Dev<int64_t> d_elems, d_line;
    Dev<MutEntry> d_entry;
    if (d_elems.alloc((size_t)most_muts + 1, false, st) != hipSuccess || d_line.alloc((size_t)most_nodes * 3 + 1, false, st) != hipSuccess ||
        d_entry.alloc((size_t)most_entries, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "mutation entries");
    clock.lap("mutations.layout");

    int64_t written = 0, entries = 0;
    double t_classify = 0.0, t_text = 0.0, t_down = 0.0;
    for (size_t bi = 0; bi < batches.size(); ++bi) {
        auto t0 = std::chrono::steady_clock::now();
        MutBatch b{};
        b.v0 = (int32_t)batches[bi].i0;
        b.n = (int32_t)(batches[bi].i1 - batches[bi].i0);
        b.m0 = p->nuc_mut_offsets[batches[bi].i0];
        b.m = p->nuc_mut_offsets[batches[bi].i1] - b.m0;
        b.entries = batch_entries[bi];
        b.node_mut = d_node_mut.p;
        b.elems = d_elems.p;
        b.entry = d_entry.p;
        b.name_off = d_name_at.p;
        b.names = d_names.p;
        b.line_len = d_line.p;
        int32_t error = 0;
        if ((e = launch_mut_count(c, a, b)) != hipSuccess || (e = exclusive_scan(c, d_elems.p, d_elems.p, b.m + 1)) != hipSuccess ||
            (e = launch_mut_classify(c, a, b)) != hipSuccess ||
            (e = hipMemcpyAsync(&error, d_error.p, sizeof error, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "mutation classify kernel");
        if (error) return fail(c, PM_ERR_ARG, "a mutation's cell does not exist");
        t_classify += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        int64_t bytes = 0;
        if ((e = launch_mut_line_len(c, a, b)) != hipSuccess || (e = exclusive_scan(c, d_line.p, d_line.p, 3 * (int64_t)b.n + 1)) != hipSuccess ||
            (e = hipMemcpyAsync(&bytes, d_line.p + 3 * (int64_t)b.n, sizeof bytes, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "mutation line kernel");
        if (grow_device(&c->text_buf, &c->text_cap, (size_t)bytes) != hipSuccess) return fail(c, PM_ERR_OOM, "mutation text");
        b.text = static_cast<char*>(c->text_buf);
        if ((e = launch_mut_write(c, a, b)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "mutation text kernel");
        t_text += seconds_since(t0);
        entries += b.entries;
        if ((rc = stream_text(c, "mutation", bytes, sink, written, t_down)) != PM_OK) return rc;
    }
    unsigned long long odd = 0;
    if ((e = hipMemcpyAsync(&odd, d_odd.p, sizeof odd, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "mutation counters");
    phase_add("mutations.classify", t_classify);
    phase_add("mutations.text", t_text);
    phase_add("mutations.download_write", t_down);
    phase_add("mutations.text_bytes", (double)written);      // (a count)
    phase_add("mutations.nodes", (double)N);                 // (a count)
    phase_add("mutations.entries", (double)entries);         // (a count: elements expanded, kept or not)
    phase_add("mutations.batches", (double)batches.size());  // (a count)
    if (length) *length = written;
    if (odd_substitutions) *odd_substitutions = (int64_t)odd;
    return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_print_mutations_fd(pm_ctx* c, const pm_panmat* p, int fd, int64_t* length, int64_t* odd_substitutions) {
    if (!c) return PM_ERR_ARG;
    if (fd < 0) return fail(c, PM_ERR_ARG, "bad file descriptor");
    return guarded(c, "mutation", [&]() { return mutations_steps(c, p, fd_sink(fd), length, odd_substitutions); });
}

int pm_print_mutations(pm_ctx* c, const pm_panmat* p, char** text, int64_t* length, int64_t* odd_substitutions) {
    if (!c) return PM_ERR_ARG;
    if (!text || !length) return fail(c, PM_ERR_ARG, "bad arguments");
    return collect_text(c, "mutation", text, [&](const Sink& sink) { return mutations_steps(c, p, sink, length, odd_substitutions); });
}

}  // extern "C"
