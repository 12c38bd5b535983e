// pm_impute_plan.h -- the host plan of pm_impute (pm_impute_plan.cpp): everything of Tree::imputeNs
// (src/impute.cpp) that is a walk over the tree and not a pass over mutation records -- the insertion
// census with mergeIndels' quirks (:147-183, src/panman.hpp:408-421), the block lookup tables with
// their drifting strand (:186-203, :130-139), the candidate walk of findNearbyInsertions (:288-337)
// as (node, candidate) pairs with their path steps, consolidateBlockMutations of a path's block lists
// and the winner rule (:277-282).  No HIP header: plain g++ compiles it (tests/impute_host_check.cpp).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/panman_gpu.h"

namespace pm {

// One merged insertion run of a node: an IndelPosition and the N codes among its bases.
struct ImputeRun {
    int32_t blk, pos, gap, length, ns;
};

// One list of a pair's path, candidate first: the nucleotide and block lists of `node`, inverted
// (MutationList::invertMutations, src/panman.cpp:2374-2420) or as they are.
struct ImputeStep {
    int32_t node;
    uint8_t inverted;
};

struct ImputePair {
    int32_t attempt, candidate;
    int64_t step0, step1;          // its steps in ImputePlan::steps; the last is the moving node's own list
    int32_t block_improvement;     // node->blockMutation.size() - consolidateBlockMutations(path).size()
};

struct ImputeAttempt {
    int32_t node, runs_with_n;     // the moving node and its runs that hold an N
    int64_t pair0, pair1;          // its candidates in walk order
};

struct ImputeBlockMut {
    int32_t primary;
    uint8_t info, inversion;
};

struct ImputePlan {
    std::vector<int32_t> parent;
    std::vector<int64_t> run_off;              // [nodes + 1] into runs
    std::vector<ImputeRun> runs;               // per node in list order, equal IndelPositions collapsed to the first
    std::vector<int64_t> was_inv_off;          // [nodes + 1] into was_inv
    std::vector<ImputeBlockMut> was_inv;       // wasBlockInv: per deletion of a node (primary, -, originalState)
    std::vector<ImputeAttempt> attempts;       // in node-id order
    std::vector<ImputePair> pairs;
    std::vector<ImputeStep> steps;
};

// Topology, types, lengths and secondary blocks of `p`: PM_OK, or the code with its text in `err`.
int impute_check(const pm_panmat* p, std::string& err);
// The plan of `p` (impute_check has passed).  PM_ERR_ARG with the reference's message when
// consolidateBlockMutations throws on a pair's block lists.
int impute_plan(const pm_panmat* p, int32_t max_distance, ImputePlan& out, std::string& err);
// consolidateBlockMutations of a pair's block lists, in ascending block id.
bool impute_pair_blocks(const pm_panmat* p, const ImputePlan& plan, const ImputePair& pair, std::vector<ImputeBlockMut>& out,
                        std::string& err);
// The winner among n candidates in walk order: the last one that raised the ratchet (nucImprovement >
// best and blockImprovement >= best, from (-1, 0)); -1: none.
int64_t impute_winner(const int64_t* nuc_improvement, const ImputePair* pairs, int64_t n);

}  // namespace pm
