// pm_launch.h -- what launch_fitch and launch_sankoff share: the device tables of the chosen form,
// the kernel arguments, the loop over a Schedule's steps (pm_schedule.h) and the executor of the
// pre-order steps.  Included by pm_fitch.hip and pm_sankoff.hip, inside the build's kernel namespace.
#pragma once

#include "pm_kernels.h"

namespace pm {
inline namespace PM_KNS {

// The DevTree arrays of the chosen form (RunForm's counterpart on the device).
struct DevForm {
    const int32_t* child_enc;
    const NodeDesc *up_desc, *down_desc;
    const PartDesc* parts;
    const int32_t* pslot;
    const TailDesc* tail;
    const int32_t *lvl_up, *lvl_down, *lvl_base;   // level tables of the band launches (lvl_base: null unless dense)
};

inline DevForm dev_form(const pm_ctx* c, const RunPaths& p) {
    const DevTree& dt = c->dt;
    const HostTree& ht = c->ht;
    const bool g = p.grp, gs = g && p.sankoff;
    DevForm f;
    f.child_enc = p.sub ? dt.child_enc_k : p.virt ? dt.child_enc_v : dt.child_enc;
    f.up_desc = gs ? dt.up_desc_gs : g ? dt.up_desc_g : p.sub ? dt.up_desc_k : p.virt ? dt.up_desc_v : dt.up_desc;
    f.down_desc = p.sub_down ? dt.down_desc_ks : p.sub ? dt.down_desc_k : p.virt ? dt.down_desc_v : dt.down_desc;
    f.parts = gs ? dt.part_desc_gs : p.sub ? dt.part_desc_k : p.virt ? dt.part_desc_v : dt.part_desc;
    // (up slots with Fitch's sweeps: the level items' slots follow the sweep plan)
    f.pslot = gs ? dt.pslot_gs : p.sankoff ? dt.pslot_k : g ? (p.clu ? dt.pslot_gc : dt.pslot_g) : p.clu ? dt.pslot_kc : dt.pslot_k;
    f.tail = p.sub ? dt.tail_desc_k : p.virt ? dt.tail_desc_v : dt.tail_desc;
    f.lvl_up = dt.lvl + ht.lvl_up[p.up_form];
    f.lvl_down = dt.lvl + ht.lvl_down[p.form];
    f.lvl_base = p.sub ? (ht.down_dense_k ? dt.lvl + ht.lvl_base_k : nullptr) : p.virt && ht.down_dense_v ? f.lvl_down : nullptr;
    return f;
}

// the grid of a step that runs one wave or one workgroup per (item, tile)
inline dim3 step_grid(const Step& st, int32_t tiles) { return PM_TILE_FAST ? dim3(st.grid_x) : dim3(st.grid_x, tiles); }

// The fields UpArgs and DownArgs share (A a{}: every other field zero).
template <class A>
A common_args(const pm_ctx* c, const DevForm& f) {
    A a{};
    a.child_off = c->dt.child_off;
    a.child_enc = f.child_enc;
    a.vleaf = reinterpret_cast<const int4*>(c->dt.vleaf);
    a.leaf_flag = c->leaf_flag;
    a.leaf_planes = c->leaf_planes;
    a.leaf_present = c->leaf_present;
    a.sets = reinterpret_cast<uint4*>(c->sets);
    a.cmask = c->cmask;
    a.cons = c->cons;
    a.all_present = c->leaves_all_present;
    a.root_dense = c->dt.root_dense;
    a.tiles = (c->words + kWave - 1) / kWave;
    a.wpad = (int64_t)a.tiles * kWave;
    return a;
}

// Everything of UpArgs but forced and absent_code0, which the modes set differently.
inline UpArgs fill_up_args(const pm_ctx* c, const RunPaths& p, const DevForm& f) {
    UpArgs up = common_args<UpArgs>(c, f);
    up.desc_all = f.up_desc;   // grouped launches: pad0 / pad1 index the whole array
    // up slots: the subtree form's kernels (alloc_work sizes them for its up orders)
    up.upm = p.sub ? c->upm : nullptr;
    up.pslot = f.pslot;
    return up;
}

// ... and of DownArgs.
inline DownArgs fill_down_args(const pm_ctx* c, const RunPaths& p, const DevForm& f) {
    const DevTree& dt = c->dt;
    DownArgs dn = common_args<DownArgs>(c, f);
    dn.parent_dense = dt.parent_dense;
    dn.internal_id = dt.internal_id;
    dn.leaf_id = dt.leaf_id;
    dn.root_final = c->root_final;
    dn.dense_base = -1;
    dn.words = c->words;
    dn.sites = c->num_sites;
    dn.recs = c->recs;
    dn.shard_cap = c->shard_cap;
    dn.shard_cnt = c->shard_cnt;
    dn.root_code = c->root_code;
    dn.vinner = dt.vinner;
    dn.sbase = c->ht.sbase;
    dn.sub_planes = c->sub_planes;
    // PM_OPT_SUB_DOWN: the S children's leaf words and node ids (their tail descriptors)
    dn.tail = p.sub_down ? dt.tail_desc_k : nullptr;
    dn.num_s = p.sub_down ? c->ht.num_tail_s : 0;
    return dn;
}

// Steps [i0, i1) in order: forks and joins of the side stream, timer spans, and `launch(step,
// stream)` for every other step.
template <class Launch>
hipError_t run_steps(pm_ctx* c, const Schedule& s, size_t i0, size_t i1, Launch&& launch) {
    for (size_t i = i0; i < i1; ++i) {
        const Step& st = s.steps[i];
        if (st.timer_open) timer_begin(c, st.cls);
        hipError_t e = hipSuccess;
        if (st.kind == StepKind::kFork) e = side_fork(c);
        else if (st.kind == StepKind::kJoin) e = side_join(c);
        else launch(st, st.side ? c->side : c->stream);
        if (e != hipSuccess) return e;
        if (st.timer_close) timer_end(c, st.cls);
    }
    return hipSuccess;
}

// One pre-order step.  FITCH: k_down / k_down_band / k_tail of Mode::kFitch, and of
// Mode::kBlockFitch in the block mode; else Mode::kSankoff, whose block mode differs in
// DownArgs::absent_code0 alone.  The chains name every instantiation a build holds.
template <bool FITCH>
void launch_down_step(pm_ctx* c, const Schedule& s, const Step& st, const DevForm& f, const DownArgs& args) {
    constexpr Mode M = FITCH ? Mode::kFitch : Mode::kSankoff;
    const RunPaths& p = s.paths;
    const bool ap = p.ap, block = FITCH && p.block, sub_down = p.sub_down, dense = st.dense_base >= 0;
    const dim3 grid = step_grid(st, args.tiles);
    const dim3 kb(kBlock);
    hipStream_t q = c->stream;
    DownArgs dn = args;
    // (the level kinds' items; a band indexes the whole array)
    dn.desc = st.kind >= StepKind::kDownLevel && st.kind <= StepKind::kDownPacked ? f.down_desc + st.first : f.down_desc;
    dn.count = st.count;
    dn.dense_base = st.dense_base;
    switch (st.kind) {
    case StepKind::kDownSweep: {
        const ClDownArgs ca{c->dt.cl_down_items, c->dt.cl_wg_off, st.first};
        hipLaunchKernelGGL(k_down_cluster<M>, dim3(st.grid_x), dim3(kWave), 0, q, dn, ca);
        break;
    }
    case StepKind::kDownBand: {
        const dim3 tg(st.grid_x), tb(kBandBlock);
        const bool grp = st.variant != 0;   // level groups inside the band (PM_OPT_GROUP_WAVES on)
        if constexpr (FITCH) {
            // (subtree form: the lean body as in the level kernels, S2 / S3 records in k_tail)
            if (block && ap) hipLaunchKernelGGL((k_down_band<Mode::kBlockFitch, true>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
            else if (block) hipLaunchKernelGGL((k_down_band<Mode::kBlockFitch, false>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
            else if (sub_down && grp) hipLaunchKernelGGL((k_down_band<M, true, true, true>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
            else if (sub_down) hipLaunchKernelGGL((k_down_band<M, true, true>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
        }
        if (block || sub_down) break;
        if (ap && grp) hipLaunchKernelGGL((k_down_band<M, true, false, true>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
        else if (ap) hipLaunchKernelGGL((k_down_band<M, true>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
        else if (grp) hipLaunchKernelGGL((k_down_band<M, false, false, true>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
        else hipLaunchKernelGGL((k_down_band<M, false>), tg, tb, 0, q, dn, f.lvl_down, f.lvl_base, st.h0, st.h1);
        break;
    }
    case StepKind::kDownGroup:   // levels h0 .. h1 - 1 in one launch
        for (int k = 0; k < 3; ++k) dn.split[k] = st.split[k];
        for (int k = 0; k < 4; ++k) dn.dense_g[k] = st.dense_g[k];
        if constexpr (FITCH) {
            if (sub_down && dense) hipLaunchKernelGGL((k_down<M, true, true, true, true>), grid, kb, 0, q, dn);
            else if (sub_down) hipLaunchKernelGGL((k_down<M, true, false, true, true>), grid, kb, 0, q, dn);
        }
        if (sub_down) break;
        if (ap && dense) hipLaunchKernelGGL((k_down<M, true, true, false, true>), grid, kb, 0, q, dn);
        else if (ap) hipLaunchKernelGGL((k_down<M, true, false, false, true>), grid, kb, 0, q, dn);
        else hipLaunchKernelGGL((k_down<M, false, false, false, true>), grid, kb, 0, q, dn);
        break;
    case StepKind::kDownPacked:   // kDownPack items per wave (Fitch, all present, dense)
        if constexpr (FITCH) hipLaunchKernelGGL((k_down<M, true, true, false, false, kDownPack>), grid, kb, 0, q, dn);
        break;
    case StepKind::kDownLevel:
        // (subtree form: the levels' descriptors omit S2 / S3 children, whose records come from the
        // tail launch, so the lean kernels run every level)
        if constexpr (FITCH) {
            if (block && ap) hipLaunchKernelGGL((k_down<Mode::kBlockFitch, true, false>), grid, kb, 0, q, dn);
            else if (block) hipLaunchKernelGGL((k_down<Mode::kBlockFitch, false, false>), grid, kb, 0, q, dn);
            else if (sub_down && dense) hipLaunchKernelGGL((k_down<M, true, true, true>), grid, kb, 0, q, dn);
            else if (sub_down) hipLaunchKernelGGL((k_down<M, true, false, true>), grid, kb, 0, q, dn);
        }
        if (block || sub_down) break;
        if (ap && dense) hipLaunchKernelGGL((k_down<M, true, true>), grid, kb, 0, q, dn);
        else if (ap) hipLaunchKernelGGL((k_down<M, true, false>), grid, kb, 0, q, dn);
        else hipLaunchKernelGGL((k_down<M, false, false>), grid, kb, 0, q, dn);
        break;
    case StepKind::kTailPacked:   // the S2 / S3 items, kTailPack per wave (Fitch)
        dn.tail = c->dt.tail_desc_k;
        dn.num_s = st.count;
        dn.count = (st.count + kTailPack - 1) / kTailPack;
        if constexpr (FITCH) hipLaunchKernelGGL((k_tail<M, true, true, kTailPack>), grid, kb, 0, q, dn);
        break;
    case StepKind::kTail:
        dn.tail = f.tail + st.first;
        dn.num_s = st.count2;
        if (p.sub) hipLaunchKernelGGL((k_tail<M, true, true>), grid, kb, 0, q, dn);
        else if (block) {
            if constexpr (FITCH) {
                if (ap) hipLaunchKernelGGL((k_tail<Mode::kBlockFitch, true>), grid, kb, 0, q, dn);
                else hipLaunchKernelGGL((k_tail<Mode::kBlockFitch, false>), grid, kb, 0, q, dn);
            }
        } else if (ap) hipLaunchKernelGGL((k_tail<M, true>), grid, kb, 0, q, dn);
        else hipLaunchKernelGGL((k_tail<M, false>), grid, kb, 0, q, dn);
        break;
    default:
        break;
    }
}

// The pre-order half of a launcher: the shard counters cleared, then the steps from first_down.
template <bool FITCH>
hipError_t run_down(pm_ctx* c, const Schedule& s, const DevForm& f, const uint4* forced, bool absent_code0) {
    const hipError_t e = hipMemsetAsync(c->shard_cnt, 0, sizeof(uint32_t) * kShards, c->stream);
    if (e != hipSuccess) return e;
    DownArgs dn = fill_down_args(c, s.paths, f);
    dn.forced = forced;
    dn.absent_code0 = absent_code0;
    return run_steps(c, s, s.first_down, s.steps.size(), [&](const Step& st, hipStream_t) { launch_down_step<FITCH>(c, s, st, f, dn); });
}

}  // namespace PM_KNS
}  // namespace pm
