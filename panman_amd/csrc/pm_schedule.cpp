// pm_schedule.cpp -- which kernels a pm_run launches, decided on the host tables alone
// (pm_schedule.h; executed by launch_fitch / launch_sankoff through pm_launch.h).
#include "pm_schedule.h"

#include <algorithm>

namespace pm {

RunPaths run_paths(const HostTree& ht, const RunOpts& o, int mode) {
    RunPaths p{};
    p.sankoff = mode == PM_MODE_SANKOFF || mode == PM_MODE_BLOCK_SANKOFF;
    p.block = mode == PM_MODE_BLOCK_FITCH || mode == PM_MODE_BLOCK_SANKOFF;
    p.ap = o.leaves_all_present != 0;
    p.virt = !p.block && o.virtual_leaf_parents;
    p.sub = p.virt && o.subtree_form && p.ap && ht.num_sshape > 0;
    const ClusterPlan& cl = ht.cl;
    const bool plan = cl.band_wg.size() > 1;
    p.planned = p.sub && o.cluster && plan;
    // post-order sweeps.  Fitch: above the plan's first level; Sankoff: only a plan that covers every height
    // with no node above 255 children.  Grouped launches: in Fitch, on a tree with a sweep plan (PM_OPT_CLUSTER
    // on or off), only below the sweeps; in Sankoff whenever PM_OPT_UP_GROUP is on
    p.clu = p.planned && (!p.sankoff || (cl.h0 == 0 && cl.max_degree <= 255));
    p.grp = p.sub && o.up_group && (p.sankoff || p.clu || !plan);
    p.sub_down = !p.sankoff && p.sub && o.sub_down;
    p.cld = p.planned && cl.down && !p.sub_down;
    p.form = p.sub ? 2 : p.virt ? 1 : 0;
    p.up_form = p.grp ? (p.sankoff ? 4 : 3) : p.form;
    // Non-temporal set-record loads when the tree has a level of at least 64k (node, tile) waves: there the records a
    // wave reads have left the caches anyway (N* Fitch 14.7 -> 14.06 ms; C3, small levels, keeps ordinary loads: 4.42 -> 4.30 ms)
    int64_t widest = 0;
    for (size_t l = 0; l + 1 < ht.down_level_off.size(); ++l) widest = std::max<int64_t>(widest, ht.down_level_off[l + 1] - ht.down_level_off[l]);
    p.nt = o.nt_loads >= 0 ? o.nt_loads != 0 : widest * o.tiles >= 65536;
    return p;
}

RunForm run_form(const HostTree& ht, const RunPaths& p) {
    RunForm f{};
    const bool g = p.grp, gs = g && p.sankoff;
    f.up_level_off = gs ? &ht.up_level_off_gs : g ? &ht.up_level_off_g : p.sub ? &ht.up_level_off_k : p.virt ? &ht.up_level_off_v : &ht.up_level_off;
    f.up_class_off = gs ? &ht.up_class_off_gs : g ? &ht.up_class_off_g : p.sub ? &ht.up_class_off_k : p.virt ? &ht.up_class_off_v : &ht.up_class_off;
    f.down_level_off = p.sub ? &ht.down_level_off_k : p.virt ? &ht.down_level_off_v : &ht.down_level_off;
    f.part_off = gs ? &ht.part_off_gs : p.sub ? &ht.part_off_k : p.virt ? &ht.part_off_v : &ht.part_off;
    f.up_degree = &ht.up_degree[gs ? 3 : p.form];
    f.up_leafy = gs ? &ht.up_leafy_gs : g ? &ht.up_leafy_g : p.sub ? &ht.up_leafy_k : p.virt ? &ht.up_leafy_v : nullptr;
    f.up_recomp = gs ? &ht.up_recomp_gs : g ? &ht.up_recomp_g : nullptr;
    f.up_plain = gs ? &ht.up_plain_gs : g ? &ht.up_plain_g : nullptr;
    f.dense_base_k = p.sub ? &ht.down_dense_base_k : nullptr;
    f.num_tail = p.sub ? ht.num_tail_k : p.virt ? ht.num_tail_v : ht.num_tail;
    f.dense = p.sub ? ht.down_dense_k : p.virt && ht.down_dense_v;
    return f;
}

Schedule schedule_run(const HostTree& ht, const RunOpts& o, int mode) {
    Schedule s;
    const RunPaths p = s.paths = run_paths(ht, o, mode);
    const RunForm f = run_form(ht, p);
    const ClusterPlan& cl = ht.cl;
    const int32_t tiles = (int32_t)o.tiles;
    const std::vector<int32_t>&class_off = *f.up_class_off, &down_off = *f.down_level_off;

    // one step; `span`: its part in a timer span of class `cls` (a launch alone in its span: kOwnSpan)
    enum { kNoSpan = 0, kOpens = 1, kCloses = 2, kOwnSpan = 3 };
    auto add = [&](StepKind kind, int cls, int h0, int h1, int32_t first, int32_t count, uint32_t grid_x, int span = kOwnSpan,
                   bool side = false, int variant = 0) -> Step& {
        s.steps.push_back(Step{kind, (uint8_t)variant, side, (span & kOpens) != 0, (span & kCloses) != 0, (uint8_t)cls, h0, h1,
                               first, count, grid_x});   // (Step's fields in order, up to grid_x)
        return s.steps.back();
    };
    // the sweeps, one launch per band that holds a cluster, one wave per (cluster, tile): the post-order's (class 0)
    // bottom-up, the pre-order's top-down
    auto sweeps = [&](StepKind kind, int cls) {
        for (size_t i = 0, n = cl.band_wg.size() - 1; i < n; ++i) {
            const size_t bnd = cls == 0 ? i : n - 1 - i;
            const int32_t wg0 = cl.band_wg[bnd], nwg = cl.band_wg[bnd + 1] - wg0;
            if (nwg > 0) add(kind, cls, cl.band_level[bnd], cl.band_level[bnd + 1], wg0, nwg, (uint32_t)((int64_t)nwg * tiles));
        }
    };
    // Sankoff, nodes [b, e) of one level with more than 255 children: parts, then the merge, in one span
    auto parts = [&](int h, int32_t b, int32_t e, bool side) {
        const int32_t p0 = (*f.part_off)[b], np = (*f.part_off)[e] - p0;
        int32_t widest = 0;
        for (int32_t i = b; i < e; ++i) widest = std::max(widest, (*f.up_degree)[i]);
        add(StepKind::kUpParts, 0, h, h + 1, p0, np, wave_grid_x(np, tiles), kOpens, side);
        add(StepKind::kUpMerge, 0, h, h + 1, b, e - b, wave_grid_x(e - b, tiles), kCloses, side, widest < (1 << 16) ? 16 : 32);
    };

    // ---- post-order: the levels below the sweeps, then the sweeps band by band.  Sankoff's sweeps
    // take every height or none (h0 == 0); Fitch's the heights from cl.h0 (the grouped order holds
    // the levels below h0 only)
    const int H = p.clu && (p.sankoff || !p.grp) ? cl.h0 : (int)f.up_level_off->size() - 1;
    // runs of >= 2 narrow levels (PM_OPT_NARROW): one band launch each (Sankoff: levels of
    // out-degree <= 3 nodes only)
    auto narrow_up = [&](int h) {
        const int32_t b = class_off[h * kDegreeClasses], m = class_off[h * kDegreeClasses + 1], e = class_off[(h + 1) * kDegreeClasses];
        return p.sankoff ? e == m && m - b <= o.narrow_max : (m - b) + 4 * (e - m) <= o.narrow_max;
    };
    const int64_t plain_min = o.plain_min_waves > 0 ? o.plain_min_waves : kPlainMinWaves;
    for (int h = 0; h < H; ++h) {
        if (o.narrow_max > 0 && narrow_up(h)) {
            int h1 = h + 1;
            while (h1 < H && narrow_up(h1)) ++h1;
            if (h1 - h >= 2) {
                add(StepKind::kUpBand, 0, h, h1, h, h1 - h, (uint32_t)tiles);
                h = h1 - 1;
                continue;
            }
        }
        // out-degree <= 3: one wave per (node, tile); wider: one workgroup per (node, tile), in
        // Sankoff by counter width (<= 15, <= 255 children; more: parts)
        const int32_t* co = &class_off[h * kDegreeClasses];
        const int32_t b = co[0], m = co[1], e = co[kDegreeClasses];
        const int32_t we = p.sankoff ? co[3] : e;   // the wide nodes one mixed launch takes
        if (m > b && we > m && (int64_t)(m - b) * tiles <= kMixedMaxWaves) {   // both kinds: one launch, blocks on one axis
            add(StepKind::kUpMixed, 0, h, h + 1, b, m - b, wave_grid_x(m - b, tiles) + (uint32_t)((int64_t)(we - m) * tiles), kOwnSpan,
                false, !p.sankoff ? 0 : co[3] > co[2] ? 8 : 4).count2 = we - m;
            if (e > we) parts(h, we, e, false);
            continue;
        }
        // a level's narrow and wide nodes are independent: the wide launches run beside the
        // narrow one on the side stream (parallel graph branches) instead of after it
#ifdef PM_NO_SIDE
        const bool fork = false;
#else
        const bool fork = m > b && e > m;
#endif
        if (fork) add(StepKind::kFork, 0, h, h + 1, 0, 0, 0, kNoSpan);
        if (p.sankoff) {
            if (e > co[3]) {   // (the empty span the launcher has always timed here)
                add(StepKind::kSpan, 0, h, h + 1, 0, 0, 0);
                parts(h, co[3], e, fork);
            }
            for (int k = 2; k >= 1; --k)
                if (co[k + 1] > co[k])
                    add(StepKind::kUpWide, 0, h, h + 1, co[k], co[k + 1] - co[k], block_grid_x(co[k + 1] - co[k], tiles), kOwnSpan, fork, k == 1 ? 4 : 8);
        } else if (e > m) {   // (Fitch: untimed beside the narrow launch)
            add(StepKind::kUpWide, 0, h, h + 1, m, e - m, block_grid_x(e - m, tiles), fork ? kNoSpan : kOwnSpan, fork);
        }
        if (m > b) {
            const bool leafy = f.up_leafy && (*f.up_leafy)[h];
            // the grouped order's plain prefix (binary, no S2 / S3 child, nothing recomputed):
            // the lean kernel, then the rest of the class
            int32_t np = f.up_plain && o.plain_up && (p.sankoff || !leafy) ? std::min((*f.up_plain)[h], m - b) : 0;
            if ((int64_t)np * tiles < plain_min) np = 0;
            const int32_t rest = m - b - np;
            // Sankoff: a span per launch.  Fitch: one span over both, closed at the join when the level forks
            auto span = [&](bool first, bool last) {
                return p.sankoff ? (int)kOwnSpan : (first ? kOpens : 0) | (last && !fork ? kCloses : 0);
            };
            if (np > 0) add(StepKind::kUpNarrow, 0, h, h + 1, b, np, wave_grid_x(np, tiles), span(true, rest == 0), false, kNarrowPlain);
            if (rest > 0)
                add(StepKind::kUpNarrow, 0, h, h + 1, b + np, rest, wave_grid_x(rest, tiles), span(np == 0, true), false,
                    !p.sankoff && leafy && (p.sub || p.ap) ? kNarrowLeafy : f.up_recomp && (*f.up_recomp)[h] ? kNarrowRecomp : kNarrowBase);
        }
        if (fork) add(StepKind::kJoin, 0, h, h + 1, 0, 0, 0, p.sankoff ? kNoSpan : kCloses);
    }
    if (p.clu) sweeps(StepKind::kUpSweep, 0);
    s.first_down = s.steps.size();

    // ---- pre-order: sweeps over the post-order's clusters (every level swept), the bands top-down
    if (p.cld) sweeps(StepKind::kDownSweep, 1);
    const int D = p.cld ? 0 : (int)down_off.size() - 1;
    auto level_items = [&](int l) { return down_off[l + 1] - down_off[l]; };
    auto narrow_down = [&](int l) { return o.narrow_max > 0 && level_items(l) <= o.narrow_max; };
    auto band_at = [&](int l) { return narrow_down(l) && l + 1 < D && narrow_down(l + 1); };
    // level groups (PM_OPT_GROUP_*): Fitch's block mode launches every level alone
    const bool groups = o.group_waves > 0 && (p.sankoff || !p.block);
    // packed levels (PM_OPT_DOWN_PACK): ungrouped, non-band launches of k_down<Fitch, AP, DENSE>
    const bool pack_form = !kCxCompact && !p.sankoff && !p.block && p.ap && !p.sub_down;
    const int64_t down_pack_min = o.down_pack_min_waves != 0 ? o.down_pack_min_waves : kDownPackMinWaves;
    for (int d = 0; d < D; ++d) {
        if (band_at(d)) {
            int d1 = d + 2;
            while (d1 < D && narrow_down(d1)) ++d1;
            add(StepKind::kDownBand, 1, d, d1, d, d1 - d, (uint32_t)tiles).variant = o.group_waves > 0;
            d = d1 - 1;
            continue;
        }
        const int32_t count = level_items(d);
        if (count == 0) continue;
        // levels d .. d + g - 1 in one launch, none of them starting a band
        int g = 1;
        int64_t items = count;
        while (groups && g < std::min<int64_t>(o.group_levels, kGroupLevels) && d + g < D) {
            const int32_t ng = level_items(d + g);
            if (ng == 0 || (items + ng) * tiles > o.group_waves || band_at(d + g)) break;
            items += ng;
            ++g;
        }
        if (g > 1) {
            Step& st = add(StepKind::kDownGroup, 1, d, d + g, down_off[d], (int32_t)items, wave_grid_x((int32_t)items, tiles));
            st.dense_base = f.dense_base(d);
            for (int k = 0; k < 4; ++k) {
                if (k > 0) st.split[k - 1] = k < g ? down_off[d + k] - down_off[d] : (int32_t)items;
                st.dense_g[k] = f.dense_base(std::min(d + k, d + g - 1));
            }
            d += g - 1;
            continue;
        }
        // a large dense level of the lean all-present kernel, below the root's, in groups of
        // kDownPack items per wave
        const bool packs = pack_form && f.dense && d > 0 && (int64_t)count * tiles >= down_pack_min;
        if (packs) s.down_pack_ranges.insert(s.down_pack_ranges.end(), {f.dense_base(d), count});
        const bool packed = packs && o.down_pack;
        add(packed ? StepKind::kDownPacked : StepKind::kDownLevel, 1, d, d + 1, down_off[d], count,
            wave_grid_x(packed ? (count + kDownPack - 1) / kDownPack : count, tiles)).dense_base = f.dense_base(d);
        s.packed_levels += packed;
    }
    // The tail (children beyond the second, S2 / S3 subtrees) needs only its parents' finals: flat launches after
    // the levels.  PM_OPT_SUB_DOWN: the levels did the S2 / S3 items, the first num_tail_s.  PM_OPT_TAIL_PACK
    // (Fitch): those items in groups per wave, the others after them, one wave each.
    const int64_t tail_pack_min = o.tail_pack_min_waves != 0 ? o.tail_pack_min_waves : kTailPackMinWaves;
    s.tail_s_waves = p.sub ? (int64_t)ht.num_tail_s * tiles : 0;
    s.tail_pack = !p.sankoff && p.sub && !p.sub_down && o.tail_pack && ht.num_tail_s > 0 && s.tail_s_waves >= tail_pack_min;
    if (s.tail_pack)
        add(StepKind::kTailPacked, 5, D, D, 0, ht.num_tail_s, wave_grid_x((ht.num_tail_s + kTailPack - 1) / kTailPack, tiles));
    const int32_t skip = p.sub_down || s.tail_pack ? ht.num_tail_s : 0;
    if (f.num_tail - skip > 0)
        add(StepKind::kTail, 5, D, D, skip, f.num_tail - skip, wave_grid_x(f.num_tail - skip, tiles)).count2 =
            p.sub && skip == 0 ? ht.num_tail_s : 0;
    return s;
}

}  // namespace pm
