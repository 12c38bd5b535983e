// pm_vcf.cpp -- host driver of VCF extraction (Tree::printVCFParallel, src/vcf.cpp:177-382;
// the command at src/panmanUtils.cpp:654-697).
//
// The reference re-derives every tip's aligned sequence on the host and compares it with the
// reference tip's, column by column.  Here all tips are replayed at once and laid out as the
// aligned FASTA text on the device (fasta_replay + format_device(aligned)); the kernels of
// pm_vcf.hip read the rows from that text, classify leaves x columns, list the events and
// emit (tip, POS, REF, ALT) records with their strings.  The host groups the records into
// lines (one per distinct (POS, REF), ALTs in byte order) and hands the device each line's
// prefix; the genotype matrix and its text are produced on the device in batches of whole
// lines and streamed through the pinned download slots.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <string_view>
#include <vector>

#include "pm_dev.h"
#include "pm_replay.h"

namespace pm {
namespace {

int vcf_steps(pm_ctx* c, const pm_panmat* p, const char* reference, const Sink& sink, int64_t* length, int64_t* skipped) {
    if (!c) return PM_ERR_ARG;
    if (!p || !reference || p->num_nodes < 1 || !p->child_offsets || !p->names) return fail(c, PM_ERR_ARG, "bad arguments");
    (void)hipSetDevice(c->device);
    // the reference must name a tip, and there must be a tip to compare with it
    int32_t ref_node = -1, tips = 0;
    {
        const char* nm = p->names;
        for (int32_t v = 0; v < p->num_nodes; ++v) {
            const bool tip = p->child_offsets[v] == p->child_offsets[v + 1];
            tips += tip;
            if (ref_node < 0 && std::strcmp(nm, reference) == 0) {
                if (!tip) return fail(c, PM_ERR_ARG, "VCF reference '" + std::string(reference) + "' is not a tip");
                ref_node = v;
            }
            nm += std::strlen(nm) + 1;
        }
    }
    if (ref_node < 0) return fail(c, PM_ERR_ARG, "VCF reference '" + std::string(reference) + "' not found");
    if (tips < 2) return fail(c, PM_ERR_ARG, "VCF needs at least two tips");

    int rc = fasta_replay(c, p);
    if (rc != PM_OK) return rc;
    PhaseClock clock;
    int64_t fasta_bytes = 0;
    std::vector<int64_t> row_base, row_len;
    if ((rc = format_device(c, 1, fasta_bytes, clock, &row_base, &row_len)) != PM_OK) return rc;
    const ReplayState& r = *c->replay;
    const int32_t L = (int32_t)r.leaves.size();
    int32_t ref_leaf = -1;
    for (int32_t li = 0; li < L; ++li)
        if (r.leaves[li] == ref_node) ref_leaf = li;
    if (ref_leaf < 0) return fail(c, PM_ERR_STATE, "VCF reference row missing");
    const int64_t n = row_len[ref_leaf];
    if (n > (int64_t)0x7fffffff - 64) return fail(c, PM_ERR_UNSUPPORTED, "VCF rows of 2^31 columns and more");
    std::vector<uint8_t> live(L, 0);
    int64_t skip_count = 0;
    for (int32_t li = 0; li < L; ++li) {
        if (li == ref_leaf) continue;
        live[li] = row_len[li] == n;   // (vcf.cpp:229-232: other lengths are not compared)
        skip_count += !live[li];
    }
    // samples: every tip but the reference, in byte order of the names
    std::vector<int32_t> samples;
    for (int32_t li = 0; li < L; ++li)
        if (li != ref_leaf) samples.push_back(li);
    std::sort(samples.begin(), samples.end(), [&](int32_t x, int32_t y) {
        const int k = r.names[r.leaves[x]].compare(r.names[r.leaves[y]]);
        return k != 0 ? k < 0 : x < y;
    });
    const int32_t S = (int32_t)samples.size();
    std::vector<int32_t> sample_of(L, -1);
    for (int32_t s = 0; s < S; ++s) sample_of[samples[s]] = s;

    // ---- device: classification, events, records ------------------------------------------
    hipStream_t st = c->stream;
    hipError_t e = hipSuccess;
    std::vector<VcfRec> recs;
    std::vector<char> pool;
    const int64_t words = (n + 63) / 64;
    int64_t events = 0;
    if (n > 0) {
        const int64_t chunks = (words + 63) / 64;
        if (chunks * L > (int64_t)0x7fffffff) return fail(c, PM_ERR_UNSUPPORTED, "VCF over this many leaves x columns");
        Dev<int64_t> d_base, d_nstart, d_chain, d_erecs, d_ebytes;
        Dev<uint8_t> d_live;
        Dev<char> d_ref, d_pool;
        Dev<int32_t> d_coord, d_eleaf, d_ecol;
        Dev<uint64_t> d_skip, d_equal;
        Dev<VcfRec> d_recs;
        if ((e = d_base.put(row_base, st)) != hipSuccess || (e = d_live.put(live, st)) != hipSuccess ||
            (e = d_ref.alloc((size_t)n, false, st)) != hipSuccess || (e = d_coord.alloc((size_t)n, false, st)) != hipSuccess ||
            (e = d_skip.alloc((size_t)L * words, false, st)) != hipSuccess ||
            (e = d_equal.alloc((size_t)L * words, false, st)) != hipSuccess ||
            (e = d_nstart.alloc((size_t)L + 1, true, st)) != hipSuccess || (e = d_chain.alloc((size_t)L, false, st)) != hipSuccess)
            return fail(c, PM_ERR_OOM, "VCF planes");
        VcfArgs a{};
        a.text = static_cast<const char*>(c->text_buf);
        a.row_base = d_base.p;
        a.live = d_live.p;
        a.leaves = L;
        a.ref_leaf = ref_leaf;
        a.n = n;
        a.words = words;
        a.ref = d_ref.p;
        a.coord = d_coord.p;
        a.skip = d_skip.p;
        a.equal = d_equal.p;
        a.nstart = d_nstart.p;
        a.chain = d_chain.p;
        if ((e = launch_vcf_classify(c, a)) != hipSuccess || (e = exclusive_scan(c, d_nstart.p, d_nstart.p, (int64_t)L + 1)) != hipSuccess ||
            (e = hipMemcpy(&events, d_nstart.p + L, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail(c, e, "VCF classification");
        clock.lap("vcf.classify");
        if (events > (int64_t)0x7ffffff0) return fail(c, PM_ERR_UNSUPPORTED, "VCF with 2^31 events and more");
        int64_t nrec = 0, nbytes = 0;
        if (events > 0) {
            if ((e = d_eleaf.alloc((size_t)events, false, st)) != hipSuccess || (e = d_ecol.alloc((size_t)events, false, st)) != hipSuccess ||
                (e = d_erecs.alloc((size_t)events + 1, true, st)) != hipSuccess ||
                (e = d_ebytes.alloc((size_t)events + 1, true, st)) != hipSuccess)
                return fail(c, PM_ERR_OOM, "VCF events");
            a.events = events;
            a.ev_leaf = d_eleaf.p;
            a.ev_col = d_ecol.p;
            a.ev_recs = d_erecs.p;
            a.ev_bytes = d_ebytes.p;
            if ((e = launch_vcf_list(c, a)) != hipSuccess || (e = launch_vcf_emit(c, a, false)) != hipSuccess ||
                (e = exclusive_scan(c, d_erecs.p, d_erecs.p, events + 1)) != hipSuccess ||
                (e = exclusive_scan(c, d_ebytes.p, d_ebytes.p, events + 1)) != hipSuccess ||
                (e = hipMemcpy(&nrec, d_erecs.p + events, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess ||
                (e = hipMemcpy(&nbytes, d_ebytes.p + events, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess)
                return hip_fail(c, e, "VCF event count");
            if ((e = d_recs.alloc((size_t)nrec, false, st)) != hipSuccess || (e = d_pool.alloc((size_t)nbytes, false, st)) != hipSuccess)
                return fail(c, PM_ERR_OOM, "VCF records");
            a.recs = d_recs.p;
            a.pool = d_pool.p;
            recs.resize((size_t)nrec);
            pool.resize((size_t)nbytes);
            if ((e = launch_vcf_emit(c, a, true)) != hipSuccess ||
                (nrec && (e = hipMemcpyAsync(recs.data(), d_recs.p, sizeof(VcfRec) * (size_t)nrec, hipMemcpyDeviceToHost, st)) != hipSuccess) ||
                (e = hipStreamSynchronize(st)) != hipSuccess ||
                (nbytes && (e = d2h_large(c, pool.data(), d_pool.p, (size_t)nbytes)) != hipSuccess))
                return hip_fail(c, e, "VCF records");
        }
        clock.lap("vcf.emit");
    }

    // ---- host: lines = distinct (POS, REF), their ALTs in byte order ------------------------
    const int64_t R = (int64_t)recs.size();
    auto ref_of = [&](const VcfRec& x) { return std::string_view(pool.data() + x.off, (size_t)x.rlen); };
    auto alt_of = [&](const VcfRec& x) { return std::string_view(pool.data() + x.off + x.rlen, (size_t)x.alen); };
    // (sorted by a 64-bit key first -- POS, then REF's leading four bytes, which orders as the
    // strings do since they hold no NUL -- so that most comparisons never touch the pool)
    std::vector<std::pair<uint64_t, int64_t>> keyed((size_t)R);
    for (int64_t i = 0; i < R; ++i) {
        const VcfRec& x = recs[(size_t)i];
        uint64_t k = (uint64_t)(uint32_t)x.pos;
        for (int b = 0; b < 4; ++b) k = (k << 8) | (b < x.rlen ? (uint8_t)pool[(size_t)x.off + b] : 0);
        keyed[(size_t)i] = {k, i};
    }
    auto before = [&](const std::pair<uint64_t, int64_t>& x, const std::pair<uint64_t, int64_t>& y) {
        if (x.first != y.first) return x.first < y.first;
        const VcfRec &u = recs[(size_t)x.second], &v = recs[(size_t)y.second];
        int k = ref_of(u).compare(ref_of(v));
        if (k == 0) k = alt_of(u).compare(alt_of(v));
        if (k != 0) return k < 0;
        return sample_of[u.leaf] != sample_of[v.leaf] ? sample_of[u.leaf] < sample_of[v.leaf] : x.second < y.second;
    };
    {   // pieces sorted side by side by the host threads, then merged pairwise (a total order: one result)
        constexpr int64_t kPiece = 1024;
        int pieces = 1;
        while (pieces < host_threads() && R / (2 * pieces) >= kPiece) pieces *= 2;
        auto cut = [&](int k) { return keyed.begin() + R * k / pieces; };
        host_parallel_for(pieces, [&](int k) { std::sort(cut(k), cut(k + 1), before); });
        for (int w = 1; w < pieces; w *= 2)
            host_parallel_for(pieces / (2 * w), [&](int k) {
                std::inplace_merge(cut(2 * w * k), cut(2 * w * k + w), cut(2 * w * k + 2 * w), before);
            });
    }
    std::vector<int64_t> order((size_t)R);
    for (int64_t i = 0; i < R; ++i) order[(size_t)i] = keyed[(size_t)i].second;
    std::vector<std::pair<uint64_t, int64_t>>().swap(keyed);
    const std::string ref_name = r.names[ref_node];
    std::vector<int64_t> prefix_off{0}, cell_off{0}, est;   // per line
    std::string prefix;
    std::vector<int32_t> cells;   // (line, sample, ALT index) per record, in line order
    {
        std::string alts;
        int32_t alt = 0;
        int64_t extra = 0;
        auto close_line = [&]() {
            prefix += alts;
            prefix += "\t.\t.\t.\t.";
            prefix_off.push_back((int64_t)prefix.size());
            cell_off.push_back((int64_t)cells.size() / 3);
            // (an upper bound when a tip carries two ALTs of the line: the batches are cut by it)
            est.push_back(prefix_off.back() - prefix_off[prefix_off.size() - 2] + 2 * (int64_t)S + extra + 1);
        };
        for (int64_t i = 0; i < R; ++i) {
            const VcfRec& x = recs[(size_t)order[(size_t)i]];
            const bool first = i == 0;
            const VcfRec* prev = first ? nullptr : &recs[(size_t)order[(size_t)i - 1]];
            const bool new_line = first || prev->pos != x.pos || ref_of(*prev) != ref_of(x);
            if (new_line) {
                if (!first) close_line();
                const int64_t id = (int64_t)prefix_off.size() - 1;
                prefix += ref_name;
                prefix += '\t';
                prefix += std::to_string(x.pos);
                prefix += '\t';
                prefix += std::to_string(id);
                prefix += '\t';
                if (x.rlen == 0) prefix += '.';
                else prefix.append(ref_of(x));
                prefix += '\t';
                alts.clear();
                alt = 0;
                extra = 0;
            }
            if (new_line || alt_of(*prev) != alt_of(x)) {
                if (alt) alts += ',';
                if (x.alen == 0) alts += '.';
                else alts.append(alt_of(x));
                ++alt;
            }
            cells.push_back((int32_t)(prefix_off.size() - 1));
            cells.push_back(sample_of[x.leaf]);
            cells.push_back(alt);
            extra += digits_of((uint64_t)alt) - 1;
        }
        if (R) close_line();
    }
    const int64_t lines = (int64_t)prefix_off.size() - 1;
    clock.lap("vcf.group_host");
    phase_add("vcf.records", (double)R);   // (counts)
    phase_add("vcf.lines", (double)lines);

    // ---- text: header from the host, genotype lines from the device in batches -------------
    std::string head = "##fileformat=VCFv4.2\n##fileDate=";
    {
        const std::time_t t = std::time(nullptr);
        std::tm now{};
        localtime_r(&t, &now);
        head += std::to_string(now.tm_year + 1900) + std::to_string(now.tm_mon + 1) + std::to_string(now.tm_mday);
    }
    head += "\n##source=PanMATv2.0-beta\n##reference=" + ref_name + "\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    for (int32_t s = 0; s < S; ++s) {
        head += '\t';
        head += r.names[r.leaves[samples[s]]];
    }
    head += '\n';
    int64_t written = 0;
    double t_text = 0.0, t_down = 0.0;
    if (!sink(head.data(), head.size())) return write_failed(c, "VCF");
    written += (int64_t)head.size();
    // batches of whole lines under the byte limit by their bounds (at least one line) and the launch grid's limit
    for (const Batch& b : cut_batches(est, c->vcf_batch_bytes, [](int64_t) { return (int64_t)1; }, (int64_t)0x7fffffff)) {
        const int64_t l0 = b.i0, l1 = b.i1;
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t nl = l1 - l0, c0 = cell_off[(size_t)l0], nc = cell_off[(size_t)l1] - c0;
        std::vector<int32_t> bc(cells.begin() + 3 * c0, cells.begin() + 3 * (c0 + nc));
        for (int64_t k = 0; k < nc; ++k) bc[(size_t)(3 * k)] -= (int32_t)l0;
        std::vector<int64_t> bo((size_t)nl + 1);
        for (int64_t k = 0; k <= nl; ++k) bo[(size_t)k] = prefix_off[(size_t)(l0 + k)] - prefix_off[(size_t)l0];
        std::vector<char> bp(prefix.begin() + prefix_off[(size_t)l0], prefix.begin() + prefix_off[(size_t)l1]);
        Dev<int32_t> d_cell;
        Dev<uint32_t> d_gt;
        Dev<int64_t> d_poff, d_loff;
        Dev<char> d_pre;
        if ((e = d_cell.put(bc, st)) != hipSuccess || (e = d_poff.put(bo, st)) != hipSuccess || (e = d_pre.put(bp, st)) != hipSuccess ||
            (e = d_gt.alloc((size_t)nl * S, false, st)) != hipSuccess || (e = d_loff.alloc((size_t)nl + 1, true, st)) != hipSuccess)
            return fail(c, PM_ERR_OOM, "VCF text batch");
        VcfTextArgs t{};
        t.lines = (int32_t)nl;
        t.samples = S;
        t.cells = nc;
        t.cell = d_cell.p;
        t.gt = d_gt.p;
        t.prefix_off = d_poff.p;
        t.prefix = d_pre.p;
        t.line_off = d_loff.p;
        int64_t total = 0;
        if ((e = launch_vcf_text_count(c, t)) != hipSuccess || (e = exclusive_scan(c, d_loff.p, d_loff.p, nl + 1)) != hipSuccess ||
            (e = hipMemcpy(&total, d_loff.p + nl, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail(c, e, "VCF text count");
        if (total > b.bytes) return fail(c, PM_ERR_STATE, "VCF text batch longer than its bound");
        if (grow_device(&c->text_buf, &c->text_cap, (size_t)std::max<int64_t>(total, 1)) != hipSuccess)
            return fail(c, PM_ERR_OOM, "VCF text");
        t.text = static_cast<char*>(c->text_buf);
        if ((e = launch_vcf_text_write(c, t)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(c, e, "VCF text kernel");
        t_text += seconds_since(t0);
        if ((rc = stream_text(c, "VCF", total, sink, written, t_down)) != PM_OK) return rc;
    }
    phase_add("vcf.text", t_text);
    phase_add("vcf.download_write", t_down);
    phase_add("vcf.text_bytes", (double)written);
    if (length) *length = written;
    if (skipped) *skipped = skip_count;
    return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_vcf_fd(pm_ctx* c, const pm_panmat* p, const char* reference, int fd, int64_t* length, int64_t* skipped) {
    if (!c) return PM_ERR_ARG;
    if (fd < 0) return fail(c, PM_ERR_ARG, "bad file descriptor");
    // (138 M records at C5 are gigabytes of host vectors)
    return guarded(c, "VCF", [&]() { return vcf_steps(c, p, reference, fd_sink(fd), length, skipped); });
}

int pm_vcf(pm_ctx* c, const pm_panmat* p, const char* reference, char** text, int64_t* length, int64_t* skipped) {
    if (!c) return PM_ERR_ARG;
    if (!text || !length) return fail(c, PM_ERR_ARG, "bad arguments");
    return collect_text(c, "VCF", text, [&](const Sink& sink) { return vcf_steps(c, p, reference, sink, length, skipped); });
}

}  // extern "C"
