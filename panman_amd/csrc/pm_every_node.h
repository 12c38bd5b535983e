// pm_every_node.h -- the rows of every node, internal ones included, for the drivers that read
// them (pm_aa, pm_mutations, pm_usher): the replay produces leaf rows, so they replay a derived PanMAT in
// which every internal node has one more, childless child without mutations -- that child's row
// is the internal node's row, and no replay kernel changes.  Also the columns' positions.
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "pm_replay.h"

namespace pm {

// `p` with a childless, mutation-free child under every internal node (ids num_nodes, ... in
// the order of their parents); its arrays live in the object.  With `every_block_at_root` the block
// mutations of `p` are replaced by one plain insertion of every block at the root: every node then
// holds every block forward, and every nucleotide mutation of its path applies (pm_usher).
struct EveryNodeATip {
    pm_panmat q;
    std::vector<int32_t> child_offsets, child_index, tip_of;   // tip_of[v]: the leaf whose row is v's
    std::vector<int64_t> block_mut_offsets, nuc_mut_offsets;
    std::vector<char> names;
    std::vector<int32_t> block_mut_primary;
    std::vector<uint8_t> block_mut_info, block_mut_inversion;

    explicit EveryNodeATip(const pm_panmat* p, bool every_block_at_root = false) : q(*p) {
        const int32_t N = p->num_nodes;
        tip_of.resize(N);
        int32_t extra = 0;
        for (int32_t v = 0; v < N; ++v) tip_of[v] = p->child_offsets[v] == p->child_offsets[v + 1] ? v : N + extra++;
        const char* end = p->names;
        for (int32_t v = 0; v < N; ++v) end += std::strlen(end) + 1;
        names.assign(p->names, end);
        names.insert(names.end(), (size_t)extra, '\0');   // (the extra tips' names are never printed)
        child_offsets.assign(1, 0);
        for (int32_t v = 0; v < N; ++v) {
            child_index.insert(child_index.end(), p->child_index + p->child_offsets[v], p->child_index + p->child_offsets[v + 1]);
            if (tip_of[v] != v) child_index.push_back(tip_of[v]);
            child_offsets.push_back((int32_t)child_index.size());
        }
        child_offsets.insert(child_offsets.end(), (size_t)extra, child_offsets.back());
        if (every_block_at_root) {
            const int32_t B = std::max(p->num_blocks, 0);
            block_mut_primary.assign(p->block_primary, p->block_primary + B);
            block_mut_info.assign((size_t)B, 1);
            block_mut_inversion.assign((size_t)B, 0);
            block_mut_offsets.assign((size_t)N + 1 + extra, B);
            std::fill(block_mut_offsets.begin(), block_mut_offsets.begin() + p->root + 1, 0);
            q.block_mut_primary = block_mut_primary.data();
            q.block_mut_info = block_mut_info.data();
            q.block_mut_inversion = block_mut_inversion.data();
        } else {
            block_mut_offsets.assign(p->block_mut_offsets, p->block_mut_offsets + N + 1);
            block_mut_offsets.insert(block_mut_offsets.end(), (size_t)extra, block_mut_offsets.back());
        }
        nuc_mut_offsets.assign(p->nuc_mut_offsets, p->nuc_mut_offsets + N + 1);
        nuc_mut_offsets.insert(nuc_mut_offsets.end(), (size_t)extra, nuc_mut_offsets.back());
        q.num_nodes = N + extra;
        q.child_offsets = child_offsets.data();
        q.child_index = child_index.data();
        q.names = names.data();
        q.block_mut_offsets = block_mut_offsets.data();
        q.nuc_mut_offsets = nuc_mut_offsets.data();
        // per-node options play no part (rotate = false) and branch lengths are not read
        q.circular_offset = nullptr;
        q.rotation_index = nullptr;
        q.sequence_inverted = nullptr;
        q.branch_length = nullptr;
    }

    // row_of[v]: the replayed row of node v of `p`, after fasta_replay(c, &q) filled `r`
    std::vector<int32_t> rows_of_nodes(const ReplayState& r, int32_t N) const {
        std::vector<int32_t> row_of_tip((size_t)q.num_nodes, -1), row_of((size_t)N);
        for (size_t li = 0; li < r.leaves.size(); ++li) row_of_tip[(size_t)r.leaves[li]] = (int32_t)li;
        for (int32_t v = 0; v < N; ++v) row_of[(size_t)v] = row_of_tip[(size_t)tip_of[(size_t)v]];
        return row_of;
    }
};

// Per column of the canonical row: the column of its position's main character and of the
// position's first gap slot (the column's slot index is column - col_first, -1 at col_main).
inline void column_positions(const ReplayState& r, std::vector<int32_t>& col_main, std::vector<int32_t>& col_first) {
    col_main.resize((size_t)r.columns);
    col_first.resize((size_t)r.columns);
    host_parallel_for(r.max_id + 1, [&](int id) {
        if (!r.is_block[id]) return;
        const std::vector<int64_t>& mc = r.main_col[id];
        for (size_t j = 0; j < mc.size(); ++j)
            for (int64_t col = r.gap_col[id][j]; col <= mc[j]; ++col) {
                col_main[(size_t)col] = (int32_t)mc[j];
                col_first[(size_t)col] = (int32_t)r.gap_col[id][j];
            }
    });
}

// A cell (block, position, slot) as a column: main_col / gap_col[pos_off[block] + position] are the
// columns of the position's main character and of its first gap slot (a block's positions 0..n_b).
inline void cell_columns(const ReplayState& r, std::vector<int64_t>& pos_off, std::vector<int32_t>& main_col, std::vector<int32_t>& gap_col) {
    const int32_t M = r.max_id + 1;
    pos_off.assign((size_t)M + 1, 0);
    for (int32_t id = 0; id < M; ++id) pos_off[(size_t)id + 1] = pos_off[(size_t)id] + (int64_t)r.main_col[id].size();
    main_col.resize((size_t)pos_off[(size_t)M]);
    gap_col.resize((size_t)pos_off[(size_t)M]);
    host_parallel_for(M, [&](int id) {
        if (!r.is_block[id]) return;
        for (size_t j = 0; j < r.main_col[id].size(); ++j) {
            main_col[(size_t)pos_off[(size_t)id] + j] = (int32_t)r.main_col[id][j];
            gap_col[(size_t)pos_off[(size_t)id] + j] = (int32_t)r.gap_col[id][j];
        }
    });
}

// The nodes' names back to back: node v's is names[name_at[v] .. name_at[v + 1]).
inline void node_names(const ReplayState& r, int32_t N, std::vector<int64_t>& name_at, std::vector<char>& names) {
    names.clear();
    name_at.assign((size_t)N + 1, 0);
    for (int32_t v = 0; v < N; ++v) {
        names.insert(names.end(), r.names[(size_t)v].begin(), r.names[(size_t)v].end());
        name_at[(size_t)v + 1] = (int64_t)names.size();
    }
}

}  // namespace pm
