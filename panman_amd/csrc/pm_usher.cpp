// pm_usher.cpp -- host driver of the UShER MAT export (panmanToUsher, src/panman2usher.cpp:564-604,
// with getNodeDFS at :282-562; the --toUsher command, src/panmanUtils.cpp:1205-1240).
//
// The reference walks the tree on one thread with a running sequence keyed by (block, position,
// slot) and hands every base of every nucleotide mutation to the Protobuf library.  Here the running
// sequence after every node is a replayed row: one replay of the derived PanMAT of pm_every_node.h
// in which every block is inserted forward at the root and no other block mutation is left (the
// reference's walk never reads block mutations).  The kernels of pm_usher.hip then expand the
// mutation lists into one entry per base, look ref up in the pseudo-root row (the replay's consensus
// row) and par in the parent's row, resolve the earlier writers of a cell within a list with a
// stable sort, size every node's mutation_list and write its wire bytes.  The host orders the nodes
// in pre-order, writes the newick field, cuts the ranks into batches (PM_OPT_USHER_BATCH_BYTES) and
// streams each batch's bytes through the pinned download slots.
#include <algorithm>
#include <string>
#include <vector>

#include "pm_dev.h"
#include "pm_every_node.h"
#include "pm_newick.h"
#include "pm_replay.h"

namespace pm {
namespace {

void put_varint(std::string& out, uint64_t v) {
    for (; v >= 128; v >>= 7) out.push_back((char)(uint8_t)(v | 128));
    out.push_back((char)(uint8_t)v);
}

int usher_steps(pm_ctx* c, const pm_panmat* p, const Sink& sink, int64_t* length, int64_t* mutations) {
    if (!c) return PM_ERR_ARG;
    if (!p || p->num_nodes < 1 || !p->child_offsets || !p->names || !p->nuc_mut_offsets || p->root < 0 || p->root >= p->num_nodes ||
        p->num_blocks < 0 || (p->num_blocks > 0 && !p->block_primary))
        return fail(c, PM_ERR_ARG, "bad arguments");
    (void)hipSetDevice(c->device);
    if (has_secondary_mutation(p)) return fail(c, PM_ERR_UNSUPPORTED, "secondary blocks");
    if (length) *length = 0;
    if (mutations) *mutations = 0;
    const int32_t N = p->num_nodes;
    for (int32_t v = 0; v < N; ++v)
        if (p->child_offsets[v] > p->child_offsets[v + 1] || p->nuc_mut_offsets[v] > p->nuc_mut_offsets[v + 1])
            return fail(c, PM_ERR_ARG, "bad offsets");

    PhaseClock clock;
    const EveryNodeATip every(p, true);
    clock.lap("usher.every_node_host");
    int rc = fasta_replay(c, &every.q);   // (refuses a mutation whose cell does not exist: PM_ERR_ARG)
    if (rc != PM_OK) return rc;
    clock = PhaseClock();
    const ReplayState& r = *c->replay;
    const int32_t M = r.max_id + 1;
    if (r.columns > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "UShER rows of 2^31 - 64 columns and more");
    const int64_t muts = p->nuc_mut_offsets[N];
    if (muts > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "2^31 - 64 nucleotide mutations and more");

    // ---- host tables: the pre-order, the mutations in rank order, the parents' rows, the cells
    std::vector<int32_t> order;   // (the replay has checked that every node hangs under the root once)
    order.reserve((size_t)N);
    {
        std::vector<int32_t> st{p->root};
        while (!st.empty()) {
            const int32_t v = st.back();
            st.pop_back();
            order.push_back(v);
            for (int32_t e = p->child_offsets[v + 1] - 1; e >= p->child_offsets[v]; --e) st.push_back(p->child_index[e]);
        }
    }
    bool in_id_order = true;
    for (int32_t i = 0; i < N; ++i) in_id_order = in_id_order && order[(size_t)i] == i;
    const std::vector<int32_t> row_of = every.rows_of_nodes(r, N);
    std::vector<int32_t> par_row((size_t)N);
    std::vector<int64_t> rank_mut((size_t)N + 1, 0), rank_entries((size_t)N, 0);
    for (int32_t i = 0; i < N; ++i) {
        const int32_t v = order[(size_t)i];
        par_row[(size_t)i] = v == p->root ? -1 : row_of[(size_t)r.parent[(size_t)v]];
        rank_mut[(size_t)i + 1] = rank_mut[(size_t)i] + (p->nuc_mut_offsets[v + 1] - p->nuc_mut_offsets[v]);
    }
    std::vector<int32_t> mut_rank((size_t)muts), primary, position, gap;
    std::vector<uint8_t> info;
    std::vector<uint32_t> nucs;
    if (!in_id_order) {
        primary.resize((size_t)muts);
        position.resize((size_t)muts);
        gap.resize((size_t)muts);
        info.resize((size_t)muts);
        nucs.resize((size_t)muts);
    }
    host_parallel_for((N + 15) / 16, [&](int task) {
        for (int32_t i = task * 16; i < std::min(N, task * 16 + 16); ++i) {
            const int32_t v = order[(size_t)i];
            int64_t at = rank_mut[(size_t)i];
            for (int64_t k = p->nuc_mut_offsets[v]; k < p->nuc_mut_offsets[v + 1]; ++k, ++at) {
                mut_rank[(size_t)at] = i;
                const uint32_t inf = p->nuc_mut_info[k], type = inf & 7u;
                rank_entries[(size_t)i] += type < 3u ? (int64_t)(inf >> 4) : type < 6u ? 1 : 0;
                if (in_id_order) continue;
                primary[(size_t)at] = p->nuc_mut_primary[k];
                position[(size_t)at] = p->nuc_mut_position[k];
                gap[(size_t)at] = p->nuc_mut_gap_position[k];
                info[(size_t)at] = p->nuc_mut_info[k];
                nucs[(size_t)at] = p->nuc_mut_nucs[k];
            }
        }
    });
    for (int32_t i = 0; i < N; ++i)   // (k_usher_sizes sums a node's bytes in 32 bits)
        if (rank_entries[(size_t)i] > ((int64_t)0x7fffffff - 64) / kUsherMutBytes)
            return fail(c, PM_ERR_UNSUPPORTED, "a node whose mutation list takes 2^31 bytes and more");
    std::vector<int64_t> pos_off, cell_base((size_t)M, 0);
    std::vector<int32_t> main_col, gap_col;
    cell_columns(r, pos_off, main_col, gap_col);
    // position(cell) = 1 + the cells before it over the blocks in ascending id: the replay lays the
    // blocks out in id order, so cell_base equals r.col_start; kept apart so that the positions do
    // not lean on that layout
    for (int32_t id = 0; id + 1 < M; ++id) cell_base[(size_t)id + 1] = cell_base[(size_t)id] + r.width[(size_t)id];
    Topology topo;
    topo.root = p->root;
    topo.name.assign(r.names.begin(), r.names.begin() + N);
    topo.kids.resize((size_t)N);
    for (int32_t v = 0; v < N; ++v) topo.kids[(size_t)v].assign(p->child_index + p->child_offsets[v], p->child_index + p->child_offsets[v + 1]);
    if (p->branch_length) topo.length.assign(p->branch_length, p->branch_length + N);
    const std::string newick = newick_of(topo);
    std::string head(1, (char)0x0a);
    put_varint(head, newick.size());
    head += newick;

    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    Dev<int32_t> d_par_row, d_main_col, d_gap_col, d_mut_rank, d_primary, d_position, d_gap, d_error;
    Dev<uint8_t> d_info;
    Dev<uint32_t> d_nucs;
    Dev<int64_t> d_pos_off, d_cell_base, d_rank_mut;
    if ((e = d_par_row.put(par_row, st)) != hipSuccess || (e = d_main_col.put(main_col, st)) != hipSuccess ||
        (e = d_gap_col.put(gap_col, st)) != hipSuccess || (e = d_pos_off.put(pos_off, st)) != hipSuccess ||
        (e = d_cell_base.put(cell_base, st)) != hipSuccess || (e = d_rank_mut.put(rank_mut, st)) != hipSuccess ||
        (e = d_mut_rank.put(mut_rank, st)) != hipSuccess ||
        (e = d_primary.put(in_id_order ? p->nuc_mut_primary : primary.data(), (size_t)muts, st)) != hipSuccess ||
        (e = d_position.put(in_id_order ? p->nuc_mut_position : position.data(), (size_t)muts, st)) != hipSuccess ||
        (e = d_gap.put(in_id_order ? p->nuc_mut_gap_position : gap.data(), (size_t)muts, st)) != hipSuccess ||
        (e = d_info.put(in_id_order ? p->nuc_mut_info : info.data(), (size_t)muts, st)) != hipSuccess ||
        (e = d_nucs.put(in_id_order ? p->nuc_mut_nucs : nucs.data(), (size_t)muts, st)) != hipSuccess ||
        (e = d_error.alloc(1, true, st)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "UShER tables");
    UsherArgs a{};
    a.rows = r.d_rows;
    a.row_stride = r.dev.row_stride;
    a.columns = r.columns;
    a.pseudo = r.d_cons;   // (consensus, '-' in the slots, 'x' at the sentinels: getPseudoRoot's)
    a.blocks = M;
    a.pos_off = d_pos_off.p;
    a.main_col = d_main_col.p;
    a.gap_col = d_gap_col.p;
    a.blk_lo = r.d_blk_lo;
    a.cell_base = d_cell_base.p;
    a.par_row = d_par_row.p;
    a.rank_mut = d_rank_mut.p;
    a.mut_rank = d_mut_rank.p;
    a.mut_primary = d_primary.p;
    a.mut_position = d_position.p;
    a.mut_gap = d_gap.p;
    a.mut_info = d_info.p;
    a.mut_nucs = d_nucs.p;
    a.error = d_error.p;

    // ---- batches of ranks: per entry its record, both halves of the sort's double buffers and the
    // longest wrapped mut; per mutation its scan slot; per node its sizes and header
    constexpr int64_t kPerEntry = (int64_t)sizeof(UsherEntry) + 2 * (sizeof(uint64_t) + sizeof(uint32_t)) + kUsherMutBytes;
    std::vector<int64_t> bound((size_t)N);
    for (int32_t i = 0; i < N; ++i)
        bound[(size_t)i] = rank_entries[(size_t)i] * kPerEntry + (rank_mut[(size_t)i + 1] - rank_mut[(size_t)i]) * 8 + 32;
    // (the sort and the entry indices take fewer than 2^31 entries a batch; a launch takes one workgroup a node)
    const std::vector<Batch> batches =
        cut_batches(bound, c->usher_batch_bytes, [&](int64_t i) { return rank_entries[(size_t)i] + 1; }, (int64_t)0x7fffffff - 64);
    int64_t most_nodes = 0, most_muts = 0, most_entries = 0;
    std::vector<int64_t> batch_entries;
    for (const Batch& b : batches) {
        int64_t n = 0;
        for (int64_t i = b.i0; i < b.i1; ++i) n += rank_entries[(size_t)i];
        batch_entries.push_back(n);
        most_nodes = std::max(most_nodes, b.i1 - b.i0);
        most_muts = std::max(most_muts, rank_mut[(size_t)b.i1] - rank_mut[(size_t)b.i0]);
        most_entries = std::max(most_entries, n);
    }
    Dev<int64_t> d_elems, d_node_off;
    Dev<UsherEntry> d_entry;
    Dev<uint64_t> d_key, d_key_alt;
    Dev<uint32_t> d_val, d_val_alt, d_list_len;
    if (d_elems.alloc((size_t)most_muts + 1, false, st) != hipSuccess || d_node_off.alloc((size_t)most_nodes + 1, false, st) != hipSuccess ||
        d_list_len.alloc((size_t)most_nodes, false, st) != hipSuccess || d_entry.alloc((size_t)most_entries, false, st) != hipSuccess ||
        d_key.alloc((size_t)most_entries, false, st) != hipSuccess || d_key_alt.alloc((size_t)most_entries, false, st) != hipSuccess ||
        d_val.alloc((size_t)most_entries, false, st) != hipSuccess || d_val_alt.alloc((size_t)most_entries, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "UShER entries");
    clock.lap("usher.tables_host");

    int64_t written = 0, entries = 0;
    double t_classify = 0.0, t_bytes = 0.0, t_down = 0.0;
    // every refusal lies before this first write, but for a failed write and a device failure: the
    // replay has refused every mutation whose cell does not exist, so the kernels' flag stays clear
    if (!sink(head.data(), head.size())) return write_failed(c, "UShER");
    written += (int64_t)head.size();
    for (size_t bi = 0; bi < batches.size(); ++bi) {
        auto t0 = std::chrono::steady_clock::now();
        UsherBatch b{};
        b.r0 = (int32_t)batches[bi].i0;
        b.n = (int32_t)(batches[bi].i1 - batches[bi].i0);
        b.m0 = rank_mut[(size_t)batches[bi].i0];
        b.m = rank_mut[(size_t)batches[bi].i1] - b.m0;
        b.entries = batch_entries[bi];
        b.elems = d_elems.p;
        b.entry = d_entry.p;
        b.key = d_key.p;
        b.key_alt = d_key_alt.p;
        b.val = d_val.p;
        b.val_alt = d_val_alt.p;
        b.list_len = d_list_len.p;
        b.node_off = d_node_off.p;
        int32_t error = 0;
        if ((e = launch_usher_count(c, a, b)) != hipSuccess || (e = exclusive_scan(c, d_elems.p, d_elems.p, b.m + 1)) != hipSuccess ||
            (e = launch_usher_classify(c, a, b)) != hipSuccess || (e = usher_earlier_writers(c, b)) != hipSuccess ||
            (e = hipMemcpyAsync(&error, d_error.p, sizeof error, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "UShER classify kernel");
        if (error) return fail(c, PM_ERR_ARG, "a mutation's cell does not exist");
        t_classify += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        int64_t bytes = 0;
        if ((e = launch_usher_sizes(c, a, b)) != hipSuccess || (e = exclusive_scan(c, d_node_off.p, d_node_off.p, (int64_t)b.n + 1)) != hipSuccess ||
            (e = hipMemcpyAsync(&bytes, d_node_off.p + b.n, sizeof bytes, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "UShER size kernel");
        if (grow_device(&c->text_buf, &c->text_cap, (size_t)bytes) != hipSuccess) return fail(c, PM_ERR_OOM, "UShER bytes");
        b.out = static_cast<char*>(c->text_buf);
        if ((e = launch_usher_write(c, a, b)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "UShER write kernel");
        t_bytes += seconds_since(t0);
        entries += b.entries;
        if ((rc = stream_text(c, "UShER", bytes, sink, written, t_down)) != PM_OK) return rc;
    }
    phase_add("usher.classify", t_classify);
    phase_add("usher.bytes", t_bytes);
    phase_add("usher.download_write", t_down);
    phase_add("usher.out_bytes", (double)written);        // (a count)
    phase_add("usher.nodes", (double)N);                  // (a count)
    phase_add("usher.entries", (double)entries);          // (a count: mut records)
    phase_add("usher.batches", (double)batches.size());   // (a count)
    if (length) *length = written;
    if (mutations) *mutations = entries;
    return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_to_usher_fd(pm_ctx* c, const pm_panmat* p, int fd, int64_t* length, int64_t* mutations) {
    if (!c) return PM_ERR_ARG;
    if (fd < 0) return fail(c, PM_ERR_ARG, "bad file descriptor");
    return guarded(c, "UShER", [&]() { return usher_steps(c, p, fd_sink(fd), length, mutations); });
}

int pm_to_usher(pm_ctx* c, const pm_panmat* p, char** bytes, int64_t* length, int64_t* mutations) {
    if (!c) return PM_ERR_ARG;
    if (!bytes || !length) return fail(c, PM_ERR_ARG, "bad arguments");
    return collect_text(c, "UShER", bytes, [&](const Sink& sink) { return usher_steps(c, p, sink, length, mutations); });
}

}  // extern "C"
