// pm_maf.cpp -- host driver of MAF (m-WGA) extraction (Tree::printMAF, src/maf.cpp:68-188; the
// command at src/panmanUtils.cpp:741-763).
//
// The reference walks every tip's path once for the starts (getSequenceFromReference) and once
// more per (tip, block) for the text (getBlockSequenceFromReference).  Here all tips are
// replayed at once (fasta_replay) and the kernels of pm_maf.hip read the blocks straight from
// the canonical rows: sizes, starts over each tip's print order, line lengths and the
// block-major text.  The host groups the blocks by equal consensus words (a few thousand at
// most), cuts the lines into batches of whole lines and streams each batch through the pinned
// download slots.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "pm_dev.h"
#include "pm_replay.h"

namespace pm {
namespace {

int maf_steps(pm_ctx* c, const pm_panmat* p, const Sink& sink, int64_t* length) {
    if (!c) return PM_ERR_ARG;
    if (!p || p->num_nodes < 1 || !p->child_offsets || !p->names) return fail(c, PM_ERR_ARG, "bad arguments");
    (void)hipSetDevice(c->device);
    if (has_secondary_mutation(p)) return fail(c, PM_ERR_UNSUPPORTED, "secondary blocks");

    int rc = fasta_replay(c, p);
    if (rc != PM_OK) return rc;
    PhaseClock clock;
    const ReplayState& r = *c->replay;
    const int32_t L = (int32_t)r.leaves.size();
    const int32_t M = r.max_id + 1;
    if (L < 1) return fail(c, PM_ERR_ARG, "MAF needs a tip");
    if (r.columns > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "MAF rows of 2^31 columns and more");

    // ---- host tables: per (tip, block) held / strand and the print order; the name table ---
    std::vector<int32_t> order;
    const std::vector<uint8_t> held = held_table(r, &order);
    std::vector<int64_t> name_off;
    std::vector<char> names;
    tip_names(r, name_off, names);
    // ---- blocks grouped by equal consensusSeq words, groups in the map's order (unsigned words,
    // a proper prefix first), blocks of a group in block-list order (maf.cpp:71-75, 144-146)
    std::map<std::vector<uint32_t>, std::vector<int32_t>> groups;
    for (int32_t b = 0; b < p->num_blocks; ++b)
        groups[std::vector<uint32_t>(p->block_seq + p->block_seq_offsets[b], p->block_seq + p->block_seq_offsets[b + 1])]
            .push_back(p->block_primary[b]);
    std::vector<int32_t> rank_blk;
    std::vector<uint8_t> rank_fold;
    for (const auto& g : groups)
        for (size_t k = 0; k < g.second.size(); ++k) {
            rank_blk.push_back(g.second[k]);
            rank_fold.push_back((uint8_t)((k == 0 ? kMafOpens : 0) | (k + 1 == g.second.size() ? kMafCloses : 0)));
        }
    const int32_t R = (int32_t)rank_blk.size();
    // width classes of k_maf_size: narrow blocks share a wave
    std::vector<int32_t> cls[3];
    for (int32_t id = 0; id < M; ++id) {
        if (!r.is_block[id]) continue;
        cls[r.width[id] <= kMafNarrow4 ? 0 : r.width[id] <= kMafNarrow16 ? 1 : 2].push_back(id);
    }
    std::vector<int32_t> circular(r.circular.begin(), r.circular.end());

    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    Dev<uint8_t> d_held, d_fold;
    Dev<int32_t> d_order, d_circ, d_size, d_start, d_src, d_rank, d_cls[3];
    Dev<int64_t> d_name_off, d_len;
    Dev<char> d_names;
    const int64_t entries = (int64_t)R * L;
    if ((e = d_held.put(held, st)) != hipSuccess || (e = d_order.put(order, st)) != hipSuccess ||
        (e = d_circ.put(circular, st)) != hipSuccess || (e = d_rank.put(rank_blk, st)) != hipSuccess ||
        (e = d_fold.put(rank_fold, st)) != hipSuccess || (e = d_name_off.put(name_off, st)) != hipSuccess ||
        (e = d_names.put(names, st)) != hipSuccess || (e = d_size.alloc((size_t)L * M, true, st)) != hipSuccess ||
        (e = d_start.alloc((size_t)L * M, true, st)) != hipSuccess || (e = d_src.alloc((size_t)L, true, st)) != hipSuccess ||
        (e = d_len.alloc((size_t)entries, false, st)) != hipSuccess || (e = d_cls[0].put(cls[0], st)) != hipSuccess ||
        (e = d_cls[1].put(cls[1], st)) != hipSuccess || (e = d_cls[2].put(cls[2], st)) != hipSuccess)
        return fail(c, PM_ERR_OOM, "MAF tables");
    MafArgs a{};
    a.rows = r.d_rows;
    a.row_stride = r.dev.row_stride;
    a.tips = L;
    a.blocks = M;
    a.blk_lo = r.d_blk_lo;
    a.blk_hi = r.d_blk_hi;
    a.held = d_held.p;
    a.order = d_order.p;
    a.circular = d_circ.p;
    a.size = d_size.p;
    a.start = d_start.p;
    a.src_size = d_src.p;
    a.ranks = R;
    a.rank_blk = d_rank.p;
    a.rank_fold = d_fold.p;
    a.name_off = d_name_off.p;
    a.names = d_names.p;
    a.line_len = d_len.p;
    clock.lap("maf.tables_host");
    if ((e = launch_maf_size(c, a, d_cls[0].p, (int32_t)cls[0].size(), 4)) != hipSuccess ||
        (e = launch_maf_size(c, a, d_cls[1].p, (int32_t)cls[1].size(), 16)) != hipSuccess ||
        (e = launch_maf_size(c, a, d_cls[2].p, (int32_t)cls[2].size(), 64)) != hipSuccess ||
        (e = launch_maf_start(c, a)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "MAF sizes");
    clock.lap("maf.size");
    std::vector<int64_t> len;
    if ((e = launch_maf_line_len(c, a)) != hipSuccess || (e = d_len.get(len, (size_t)entries, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return hip_fail(c, e, "MAF line lengths");
    // batches of whole lines: entries under the byte limit (at least one entry) and, by their
    // workgroups, the launch grid's limit
    auto chunks_of = [&](int64_t entry) { return (int64_t)maf_chunks(r.width[rank_blk[(size_t)(entry / L)]]); };
    const std::vector<Batch> batches = cut_batches(len, c->maf_batch_bytes, chunks_of, (int64_t)0x7fffffff);
    int64_t most = 0;
    for (const Batch& b : batches) most = std::max(most, b.i1 - b.i0);
    Dev<int64_t> d_off;
    if (d_off.alloc((size_t)most, false, st) != hipSuccess) return fail(c, PM_ERR_OOM, "MAF line offsets");
    clock.lap("maf.layout");

    // ---- text: the header from the host, the lines from the device in batches ----------------
    static const char kHead[] = "##maf version=1\n";
    int64_t written = 0;
    double t_text = 0.0, t_down = 0.0;
    if (!sink(kHead, sizeof kHead - 1)) return write_failed(c, "MAF");
    written += (int64_t)sizeof kHead - 1;
    for (const Batch& b : batches) {
        const auto t0 = std::chrono::steady_clock::now();
        const int32_t rank0 = (int32_t)(b.i0 / L), rank1 = (int32_t)((b.i1 - 1) / L);
        std::vector<int32_t> wg_off{0};
        for (int32_t k = rank0; k <= rank1; ++k) {
            const int64_t first = std::max<int64_t>((int64_t)k * L, b.i0), last = std::min<int64_t>((int64_t)(k + 1) * L, b.i1);
            wg_off.push_back((int32_t)(wg_off.back() + (last - first) * maf_chunks(r.width[rank_blk[(size_t)k]])));
        }
        Dev<int32_t> d_wg;
        if (d_wg.put(wg_off, st) != hipSuccess ||
            grow_device(&c->text_buf, &c->text_cap, (size_t)std::max<int64_t>(b.bytes, 1)) != hipSuccess)
            return fail(c, PM_ERR_OOM, "MAF text");
        MafBatch mb{};
        mb.e0 = b.i0;
        mb.e1 = b.i1;
        mb.rank0 = rank0;
        mb.nr = rank1 - rank0 + 1;
        mb.wg_off = d_wg.p;
        mb.line_off = d_off.p;
        mb.text = static_cast<char*>(c->text_buf);
        if ((e = exclusive_scan(c, d_len.p + b.i0, d_off.p, b.i1 - b.i0)) != hipSuccess ||
            (e = launch_maf_write(c, a, mb, wg_off.back())) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "MAF text kernel");
        t_text += seconds_since(t0);
        if ((rc = stream_text(c, "MAF", b.bytes, sink, written, t_down)) != PM_OK) return rc;
    }
    phase_add("maf.text", t_text);
    phase_add("maf.download_write", t_down);
    phase_add("maf.text_bytes", (double)written);   // (a count)
    phase_add("maf.entries", (double)entries);      // (block rank, tip) pairs, held or not
    if (length) *length = written;
    return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_maf_fd(pm_ctx* c, const pm_panmat* p, int fd, int64_t* length) {
    if (!c) return PM_ERR_ARG;
    if (fd < 0) return fail(c, PM_ERR_ARG, "bad file descriptor");
    return guarded(c, "MAF", [&]() { return maf_steps(c, p, fd_sink(fd), length); });
}

int pm_maf(pm_ctx* c, const pm_panmat* p, char** text, int64_t* length) {
    if (!c) return PM_ERR_ARG;
    if (!text || !length) return fail(c, PM_ERR_ARG, "bad arguments");
    return collect_text(c, "MAF", text, [&](const Sink& sink) { return maf_steps(c, p, sink, length); });
}

}  // extern "C"
