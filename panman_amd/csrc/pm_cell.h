// pm_cell.h -- device helpers of the drivers that expand nucleotide-mutation lists into one element
// per base over the replayed rows (pm_mutations.hip, pm_usher.hip): the element's mutation and the
// column of its cell.  Included by .hip files only.
#pragma once

#include <cstdint>

namespace pm {

// The last k with elems[k] <= e, elems being the exclusive scan of the elements per mutation
// (elems[m] = all elements > e): element e belongs to mutation k and is its (e - elems[k])-th.
__device__ __forceinline__ int64_t mutation_of_element(const int64_t* elems, int64_t m, int64_t e) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (elems[mid + 1] <= e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The canonical column of element j of a mutation at (blk, pos, gap): the cell (blk, pos, gap + j)
// when gap != -1, else (blk, pos + j, -1).  A block's positions 0..n_b are main_col / gap_col
// [pos_off[blk] .. pos_off[blk + 1]) (the column of the main character and of the first gap slot).
// -1: no such cell.
__device__ __forceinline__ int64_t cell_column(const int64_t* pos_off, const int32_t* main_col, const int32_t* gap_col,
                                               int32_t blocks, int32_t blk, int32_t pos, int32_t gap, int32_t j) {
    int64_t col = -1;
    if (blk >= 0 && blk < blocks && pos >= 0 && gap >= -1) {
        const int64_t o = pos_off[blk], n = pos_off[blk + 1] - o;
        if (gap != -1) {
            if (pos < n && gap + j < main_col[o + pos] - gap_col[o + pos]) col = (int64_t)gap_col[o + pos] + gap + j;
        } else if ((int64_t)pos + j < n) {
            col = main_col[o + pos + j];
        }
    }
    return col;
}

}  // namespace pm
