// pm_aa.cpp -- host driver of amino-acid translation (Tree::extractAminoAcidTranslations,
// src/aaTrans.cpp:185-304; the command at src/panmanUtils.cpp:895-938).
//
// The reference replays every node's whole sequence on one thread, finds the window of the two
// coordinates, cuts it into codons and merges them against the root's.  Here the rows of every
// node come from one replay: the replay produces leaf rows, so the driver replays a derived
// PanMAT in which every internal node has one more, childless child without mutations -- that
// child's row is the internal node's row, and no replay kernel changes.  The kernels of
// pm_aa.hip then locate the coordinates, build the codon tables, merge and write the lines;
// the host cuts the nodes into batches (PM_OPT_AA_BATCH_BYTES) and streams each batch's lines
// through the pinned download slots.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "pm_dev.h"
#include "pm_every_node.h"
#include "pm_replay.h"

namespace pm {
namespace {

// The device arrays of one batch's codon tables.
struct Tables {
    Dev<int32_t> node, cstart, cend, codons;
    Dev<uint8_t> base, error;
    AaTables t{};
    hipError_t alloc(int64_t slots, int32_t base_cap, int32_t codon_cap, hipStream_t st) {
        hipError_t e;
        if ((e = node.alloc((size_t)slots, false, st)) != hipSuccess || (e = codons.alloc((size_t)slots, true, st)) != hipSuccess ||
            (e = error.alloc((size_t)slots, true, st)) != hipSuccess || (e = base.alloc((size_t)(slots * base_cap), false, st)) != hipSuccess ||
            (e = cstart.alloc((size_t)(slots * codon_cap), false, st)) != hipSuccess ||
            (e = cend.alloc((size_t)(slots * codon_cap), false, st)) != hipSuccess)
            return e;
        t.base_cap = base_cap;
        t.codon_cap = codon_cap;
        t.node = node.p;
        t.base = base.p;
        t.cstart = cstart.p;
        t.cend = cend.p;
        t.codons = codons.p;
        t.error = error.p;
        return hipSuccess;
    }
    hipError_t set_nodes(const int32_t* v, int64_t n, hipStream_t st) {
        t.n = (int32_t)n;
        return hipMemcpyAsync(node.p, v, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st);
    }
};

int aa_steps(pm_ctx* c, const pm_panmat* p, int64_t start, int64_t end, const Sink& sink, int64_t* length, int64_t* ref_codons,
             int64_t* unlocated) {
    if (!c) return PM_ERR_ARG;
    if (!p || p->num_nodes < 1 || !p->child_offsets || !p->names || !p->block_mut_offsets || !p->nuc_mut_offsets ||
        p->root < 0 || p->root >= p->num_nodes)
        return fail(c, PM_ERR_ARG, "bad arguments");
    if (end <= start) return fail(c, PM_ERR_ARG, "End coordinate must be greater than start");
    (void)hipSetDevice(c->device);
    if (has_secondary_mutation(p)) return fail(c, PM_ERR_UNSUPPORTED, "secondary blocks");
    if (length) *length = 0;
    if (ref_codons) *ref_codons = 0;
    if (unlocated) *unlocated = 0;
    const int32_t N = p->num_nodes;
    for (int32_t v = 0; v < N; ++v)
        if (p->child_offsets[v] > p->child_offsets[v + 1]) return fail(c, PM_ERR_ARG, "bad child offsets");

    PhaseClock clock;
    const EveryNodeATip every(p);
    clock.lap("aa.every_node_host");
    int rc = fasta_replay(c, &every.q);
    if (rc != PM_OK) return rc;
    clock = PhaseClock();
    const ReplayState& r = *c->replay;
    const int32_t M = r.max_id + 1;
    if (r.columns > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "amino-acid rows of 2^31 columns and more");

    // ---- host tables: the row of every node, per (row, block) held / strand, the columns' positions
    const std::vector<int32_t> row_of = every.rows_of_nodes(r, N);
    const int32_t rows = (int32_t)r.leaves.size();
    const std::vector<uint8_t> held = held_table(r);
    std::vector<int32_t> col_main, col_first, rev_top((size_t)M, -1);
    column_positions(r, col_main, col_first);
    // a reverse-strand block that does not start the window is walked from block id 0's last
    // position, as the reference reads sequence[0] (aaTrans.cpp:39-40)
    const int64_t top0 = r.is_block[0] ? (int64_t)r.main_col[0].size() - 1 : -1;
    for (int32_t id = 0; id < M; ++id)
        if (r.is_block[id] && top0 >= 0 && top0 < (int64_t)r.main_col[id].size()) rev_top[(size_t)id] = (int32_t)r.main_col[id][(size_t)top0];
    std::vector<char> names;
    std::vector<int64_t> name_at;
    node_names(r, N, name_at, names);
    std::vector<int32_t> cls[3];   // width classes of k_maf_size
    for (int32_t id = 0; id < M; ++id) {
        if (!r.is_block[id]) continue;
        cls[r.width[id] <= kMafNarrow4 ? 0 : r.width[id] <= kMafNarrow16 ? 1 : 2].push_back(id);
    }

    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    Dev<uint8_t> d_held;
    Dev<int32_t> d_row_of, d_size, d_col_main, d_col_first, d_rev_top, d_cls[3];
    Dev<int64_t> d_name_at;
    Dev<char> d_names;
    Dev<AaSpan> d_span;
    if ((e = d_held.put(held, st)) != hipSuccess || (e = d_row_of.put(row_of, st)) != hipSuccess ||
        (e = d_size.alloc((size_t)rows * M, true, st)) != hipSuccess || (e = d_col_main.put(col_main, st)) != hipSuccess ||
        (e = d_col_first.put(col_first, st)) != hipSuccess || (e = d_rev_top.put(rev_top, st)) != hipSuccess ||
        (e = d_name_at.put(name_at, st)) != hipSuccess || (e = d_names.put(names, st)) != hipSuccess ||
        (e = d_span.alloc((size_t)N, false, st)) != hipSuccess || (e = d_cls[0].put(cls[0], st)) != hipSuccess ||
        (e = d_cls[1].put(cls[1], st)) != hipSuccess || (e = d_cls[2].put(cls[2], st)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "amino-acid tables");
    MafArgs ma{};   // the per (row, block) sizes are k_maf_size's
    ma.rows = r.d_rows;
    ma.row_stride = r.dev.row_stride;
    ma.tips = rows;
    ma.blocks = M;
    ma.blk_lo = r.d_blk_lo;
    ma.blk_hi = r.d_blk_hi;
    ma.held = d_held.p;
    ma.size = d_size.p;
    AaArgs a{};
    a.rows = r.d_rows;
    a.row_stride = r.dev.row_stride;
    a.nodes = N;
    a.blocks = M;
    a.row_of = d_row_of.p;
    a.blk_lo = r.d_blk_lo;
    a.blk_hi = r.d_blk_hi;
    a.held = d_held.p;
    a.size = d_size.p;
    a.col_main = d_col_main.p;
    a.col_first = d_col_first.p;
    a.rev_top = d_rev_top.p;
    a.start = start;
    a.end = end;
    a.span = d_span.p;
    clock.lap("aa.tables_host");

    // ---- locate: every node's start and end on its own row -------------------------------------
    std::vector<AaSpan> span;
    if ((e = launch_maf_size(c, ma, d_cls[0].p, (int32_t)cls[0].size(), 4)) != hipSuccess ||
        (e = launch_maf_size(c, ma, d_cls[1].p, (int32_t)cls[1].size(), 16)) != hipSuccess ||
        (e = launch_maf_size(c, ma, d_cls[2].p, (int32_t)cls[2].size(), 64)) != hipSuccess ||
        (e = launch_aa_locate(c, a)) != hipSuccess || (e = d_span.get(span, (size_t)N, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "amino-acid locate");
    clock.lap("aa.locate");
    auto located = [&](int32_t v) { return span[(size_t)v].cs >= 0 && span[(size_t)v].ce >= 0; };
    // a reverse-strand block after the window's first that the reference walks from outside it
    auto undefined_walk = [&](int32_t v) {
        const uint8_t* h = held.data() + (size_t)row_of[(size_t)v] * M;
        for (int32_t i = span[(size_t)v].b0 + 1; i <= span[(size_t)v].b1; ++i)
            if (r.is_block[i] && (h[i] & kMafHeld) && !(h[i] & kMafForward) && rev_top[(size_t)i] < 0) return true;
        return false;
    };
    static const char kUndefined[] = "a reverse-strand block inside the window is shorter than block 0: the reference's walk is undefined";
    if (!located(p->root)) return fail(c, PM_ERR_ARG, "coordinates out of range");
    if (undefined_walk(p->root)) return fail(c, PM_ERR_UNSUPPORTED, kUndefined);

    // ---- the root's codon table ------------------------------------------------------------------
    // bases between the two coordinates of a window that stops: end - start at most
    const int32_t base_cap = (int32_t)std::max<int64_t>(std::min<int64_t>(end - start, r.columns), 3);
    const int32_t codon_cap = base_cap / 3 + 1;
    Tables root;
    if (root.alloc(1, base_cap, codon_cap, st) != hipSuccess) return fail(c, PM_ERR_OOM, "amino-acid root table");
    int32_t root_codons = 0;
    uint8_t root_error = 0;
    if ((e = root.set_nodes(&p->root, 1, st)) != hipSuccess || (e = launch_aa_codons(c, a, root.t)) != hipSuccess ||
        (e = hipMemcpyAsync(&root_codons, root.codons.p, sizeof root_codons, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(&root_error, root.error.p, sizeof root_error, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "amino-acid root table");
    clock.lap("aa.root");
    if (root_error) return fail(c, PM_ERR_ARG, "the root's window does not reach the end coordinate");
    if (ref_codons) *ref_codons = root_codons;
    if (root_codons == 0) return PM_OK;   // (the reference returns before its header)
    int64_t lost = 0;
    for (int32_t v = 0; v < N; ++v) {
        if (!located(v)) ++lost;
        else if (undefined_walk(v)) return fail(c, PM_ERR_UNSUPPORTED, kUndefined);
    }
    if (unlocated) *unlocated = lost;

    // ---- batches of nodes: the codon tables and the largest text of a batch under the limit -----
    std::vector<int64_t> bound((size_t)N);
    for (int32_t v = 0; v < N; ++v)   // bases, starts and ends; an "I:" entry per codon and a "D:" entry per root codon
        bound[(size_t)v] = (int64_t)base_cap + 8 * (int64_t)codon_cap + 17 * (int64_t)codon_cap + 13 * (int64_t)root_codons +
                           (name_at[(size_t)v + 1] - name_at[(size_t)v]) + 2;
    const std::vector<Batch> batches = cut_batches(bound, c->aa_batch_bytes, [](int64_t) { return (int64_t)1; }, (int64_t)0x7fffffff);
    int64_t most = 0;
    for (const Batch& b : batches) most = std::max(most, b.i1 - b.i0);
    Tables tab;
    Dev<int64_t> d_len, d_off;
    Dev<int32_t> d_sec;
    if (tab.alloc(most, base_cap, codon_cap, st) != hipSuccess || d_len.alloc((size_t)most, false, st) != hipSuccess ||
        d_off.alloc((size_t)most, false, st) != hipSuccess || d_sec.alloc((size_t)most * 2, false, st) != hipSuccess)
        return fail(c, PM_ERR_OOM, "amino-acid codon tables");
    std::vector<int32_t> ids((size_t)N);
    for (int32_t v = 0; v < N; ++v) ids[(size_t)v] = v;
    clock.lap("aa.layout");

    static const char kHead[] = "node_id\taa_mutations\n";
    int64_t written = 0, lines = 0;
    double t_codons = 0.0, t_merge = 0.0, t_text = 0.0, t_down = 0.0;
    if (!sink(kHead, sizeof kHead - 1)) return write_failed(c, "amino-acid");
    written += (int64_t)sizeof kHead - 1;
    std::vector<int64_t> len;
    for (const Batch& b : batches) {
        auto t0 = std::chrono::steady_clock::now();
        const int64_t n = b.i1 - b.i0;
        if ((e = tab.set_nodes(ids.data() + b.i0, n, st)) != hipSuccess || (e = launch_aa_codons(c, a, tab.t)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "amino-acid codon kernel");
        t_codons += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        AaText x{};
        x.name_off = d_name_at.p;
        x.names = d_names.p;
        x.line_len = d_len.p;
        x.sec = d_sec.p;
        x.line_off = d_off.p;
        if ((e = launch_aa_line_len(c, a, root.t, tab.t, x)) != hipSuccess || (e = d_len.get(len, (size_t)n, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "amino-acid merge kernel");
        t_merge += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        int64_t bytes = 0;
        for (int64_t k = 0; k < n; ++k) {
            bytes += len[(size_t)k];
            lines += len[(size_t)k] != 0;
        }
        if (bytes == 0) continue;
        if (grow_device(&c->text_buf, &c->text_cap, (size_t)bytes) != hipSuccess) return fail(c, PM_ERR_OOM, "amino-acid text");
        x.text = static_cast<char*>(c->text_buf);
        if ((e = exclusive_scan(c, d_len.p, d_off.p, n)) != hipSuccess || (e = launch_aa_write(c, a, root.t, tab.t, x)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "amino-acid text kernel");
        t_text += seconds_since(t0);
        if ((rc = stream_text(c, "amino-acid", bytes, sink, written, t_down)) != PM_OK) return rc;
    }
    phase_add("aa.codons", t_codons);
    phase_add("aa.merge", t_merge);
    phase_add("aa.text", t_text);
    phase_add("aa.download_write", t_down);
    phase_add("aa.text_bytes", (double)written);     // (a count)
    phase_add("aa.nodes", (double)N);                // (a count)
    phase_add("aa.lines", (double)lines);            // (a count)
    phase_add("aa.batches", (double)batches.size()); // (a count)
    if (length) *length = written;
    return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_aa_fd(pm_ctx* c, const pm_panmat* p, int64_t start, int64_t end, int fd, int64_t* length, int64_t* ref_codons,
             int64_t* unlocated) {
    if (!c) return PM_ERR_ARG;
    if (fd < 0) return fail(c, PM_ERR_ARG, "bad file descriptor");
    return guarded(c, "amino-acid", [&]() { return aa_steps(c, p, start, end, fd_sink(fd), length, ref_codons, unlocated); });
}

int pm_aa(pm_ctx* c, const pm_panmat* p, int64_t start, int64_t end, char** text, int64_t* length, int64_t* ref_codons,
          int64_t* unlocated) {
    if (!c) return PM_ERR_ARG;
    if (!text || !length) return fail(c, PM_ERR_ARG, "bad arguments");
    return collect_text(c, "amino-acid", text,
                        [&](const Sink& sink) { return aa_steps(c, p, start, end, sink, length, ref_codons, unlocated); });
}

}  // extern "C"
