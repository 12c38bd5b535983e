/* panman_gpu.h -- C-ABI of the MI355X small-parsimony engine (libpanman_amd.so).
 *
 * Drop-in boundary for the reference's per-column parsimony path.  The reference
 * (faithokamoto/panman) has no FFI of its own: its kernels are C++ Tree members called
 * once per alignment column from the construction drivers.  Each entry point below names
 * the reference interface it replaces (paths relative to the reference root):
 *
 *   per-column Fitch      Tree::nucFitchForwardPass / BackwardPass / AssignMutations
 *                         src/panman.hpp:846-857, src/fitchSankoff.cpp:30-171
 *   per-column Sankoff    Tree::nucSankoff{Forward,Backward}Pass / AssignMutations
 *                         src/panman.hpp:860-875, src/fitchSankoff.cpp:359-703
 *   GPU batch entry       fitch_sankoff_on_gpu(Tree*, seqs, util*)   gpu/fitchSankoff.cuh:11
 *   column drivers        Tree(ifstream&, ifstream&, FILE_TYPE::MSA | MSA_OPTIMIZE, ref)
 *                         src/panman.cpp:1274-1649
 *
 * Conventions
 *   - Plain pointers and sizes only.  Host pointers unless a name says `_device`.
 *   - Every function returns PM_OK (0) or a negative PM_ERR_*; pm_last_error() gives the
 *     message.  Nothing here exits or aborts (the reference exit()s, src/panman.cpp:1297).
 *   - One pm_ctx per GPU; a ctx is not thread-safe, independent ctxs are.
 *   - Device work is queued on the ctx stream (pm_set_stream); functions that return
 *     host data synchronise that stream.
 *   - Codes are the reference's 4-bit NucCode (src/panman.hpp:27-44): A=1 C=2 G=4 T=8
 *     R=5 Y=10 S=6 W=9 K=12 M=3 B=14 D=13 H=11 V=7 N=15, gap/other=0.
 *     Packed code arrays hold two codes per byte, even site in the low nibble.
 */
#ifndef PANMAN_GPU_H
#define PANMAN_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_ERR_ARG (-1)
#define PM_ERR_OOM (-2)
#define PM_ERR_HIP (-3)
#define PM_ERR_UNSUPPORTED (-4)
#define PM_ERR_STATE (-5)

#define PM_MODE_FITCH 0   /* F1-F3: 16-bit one-hot state sets, M1 semantics            */
#define PM_MODE_SANKOFF 1 /* S1-S3: unit-cost Sankoff over 16 codes, M2 semantics      */
/* Block-level parsimony (columns = blocks; codes 0 block absent, 1 forward, 2 reverse):
 * B1 Tree::blockFitch*New   src/fitchSankoff.cpp:224-308 (leaf not in the column: state 0)
 * B2 Tree::blockSankoff*    src/fitchSankoff.cpp:707-818 (leaf not in the column: absent
 *    block, cost {0, INF, INF}).  Root parent state = consensus code (0 in the PanGraph
 *    driver, src/panman.cpp:906-909, :952-956); `forced` = defaultState of the backward
 *    pass.  Records: PM_MUT_NI -> BlockMut(BI, inversion = code == 2), PM_MUT_ND ->
 *    BlockMut(BD, false), PM_MUT_NS -> BlockMut(BD, inversion = true). */
#define PM_MODE_BLOCK_FITCH 2
#define PM_MODE_BLOCK_SANKOFF 3

#define PM_MUT_NS 0 /* NucMutationType::NS  src/panman.hpp:48 */
#define PM_MUT_ND 1 /* NucMutationType::ND  src/panman.hpp:50 */
#define PM_MUT_NI 2 /* NucMutationType::NI  src/panman.hpp:52 */

typedef struct pm_ctx pm_ctx;

/* Tree topology as CSR.  Replaces the Node* graph built by
 * Tree::createTreeFromNewickString (src/panman.cpp:310-450) and the flattening in
 * gpu/fitchSankoff.cu:40-83.  Children keep their Newick order.  A node with no
 * children is a leaf.  Node ids are the caller's; mutation records use them. */
typedef struct pm_tree {
    int32_t num_nodes;
    int32_t root;
    const int32_t* child_offsets; /* [num_nodes + 1] */
    const int32_t* child_index;   /* [child_offsets[num_nodes]] */
} pm_tree;

/* One mutation record: the (node, column, type, char) tuple the reference pushes into
 * nonGapMutationsMSA (src/panman.cpp:1426-1430, 1607-1610). */
typedef struct pm_mut {
    uint32_t node;      /* caller node id                                    */
    uint32_t site_info; /* (site << 8) | (type << 4) | code; type = PM_MUT_* */
} pm_mut;

/* Context / device (replaces the device setup of gpu/fitchSankoff.cu:370-440). */
int pm_create(int device, pm_ctx** out);
void pm_destroy(pm_ctx* ctx);
/* Initialise the HIP runtime on `device` and load the library's code objects (what the
 * first pm_create and first launches would otherwise pay), from any thread: a caller with
 * host work to do first (reading and decoding input) can overlap it.  Optional. */
int pm_warmup(int device);
const char* pm_last_error(const pm_ctx* ctx);
/* Queue all work on `hip_stream` (a hipStream_t; NULL = the ctx's own stream). */
int pm_set_stream(pm_ctx* ctx, void* hip_stream);
/* Options (results are identical either way):
 *   PM_OPT_VIRTUAL (default 1): the level kernels evaluate internal nodes whose children
 *                  are one or two leaves inline in their parent instead of materialising them.
 *   PM_OPT_GRAPH   (default 0): pm_run captures its launch sequence (per-level kernels,
 *                  memsets) into a hipGraph once and replays it while the tree, columns,
 *                  mode and buffers stay the same; kernel_times then reports the whole run
 *                  as class 4.
 *   PM_OPT_SUBTREE (default 1): Fitch with every leaf present also evaluates, inside its
 *                  binary parent, any node whose children are leaves or two-leaf cherries
 *                  (three- and four-leaf subtrees), so those are not materialised either.
 *   PM_OPT_NARROW  (default 16): Fitch -- a run of consecutive levels with at most this many
 *                  nodes each (a node of out-degree > 3 counts 4) is walked by one launch,
 *                  one 1024-thread workgroup per 2048-site tile with a barrier between levels,
 *                  instead of one launch per level (deep, ladder-like trees); 0 = off.
 *   PM_OPT_GROUP_WAVES (default 32768): Fitch -- up to PM_OPT_GROUP_LEVELS consecutive
 *                  pre-order levels of at most this many (node, tile) waves together go to one
 *                  launch, the lower levels' waves recomputing their ancestors' finals; 0 = off.
 *   PM_OPT_GROUP_LEVELS (default 4): 2 to 4 levels per such launch.
 *   PM_OPT_UP_GROUP (default 1): Fitch, subtree form -- a node of out-degree <= 3 whose
 *                  latest children have out-degree <= 3 runs in their post-order launch,
 *                  recomputing them, instead of one launch per height; 0 = by height.
 *   PM_OPT_SUB_DOWN (default 0): Fitch, subtree form -- a three- or four-leaf subtree's
 *                  finals and records come from its parent's pre-order wave instead of a
 *                  wave of their own after the levels.
 *   PM_OPT_TAIL_PACK (default 1): Fitch, subtree form -- the tail launch's three- and
 *                  four-leaf subtrees run eight consecutive items per wave, the dirty (item,
 *                  word) pairs of the eight gathered into full waves, instead of one wave per
 *                  (item, tile) with only its dirty lanes busy; the other tail items keep
 *                  their own launch -- when those subtrees make at least 65536 (item, tile)
 *                  waves: a launch the chip holds at once is no faster packed.  A value >= 2
 *                  sets that threshold, -1 packs at any size, 0 = one wave per item.  Results
 *                  identical.  Sankoff and PM_OPT_SUB_DOWN runs do not use it.
 *   PM_OPT_DOWN_PACK (default 1): Fitch, every leaf present -- a pre-order level that is a
 *                  launch of its own (no level group, no band, not the root's, not under
 *                  PM_OPT_SUB_DOWN) and a dense range of nodes runs eight consecutive nodes per
 *                  wave, the live (node, word) pairs of the eight -- the node's or its parent's
 *                  word is complex, or a leaf / leaf-parent child is read there; every word
 *                  under the root -- gathered into full waves, instead of one wave per (node,
 *                  tile) with about one lane in seven busy -- when the level makes at least
 *                  65536 (node, tile) waves.  A value >= 2 sets that threshold, -1 packs at any
 *                  size, 0 = one wave per (node, tile).  Results identical.  Sankoff, block
 *                  Fitch and inputs with absent leaves do not use it.
 *   PM_OPT_PLAIN_UP (default 1): Fitch / Sankoff, grouped subtree form -- a post-order launch's binary
 *                  nodes with no three- / four-leaf subtree child and nothing recomputed run in
 *                  a lean kernel (fewer registers, more waves in flight) before the rest, when
 *                  they are at least 65536 (node, tile) waves; a value >= 2 sets that threshold;
 *                  0 = off.
 *   PM_OPT_RECORD_CAP: the record buffer's capacity per shard (1024 shards), replacing the
 *                  first guess (about 1.5 % of node*site pairs); a run that overflows it is
 *                  re-run with a larger buffer when its results are read (pm_mutation_count,
 *                  pm_site_results*, pm_run_gather), so results never depend on it.
 *   PM_OPT_NT_LOADS (default -1): set records read with non-temporal loads (1), ordinary
 *                  loads (0), or by the tree's widest level (-1: non-temporal from 64k
 *                  (node, tile) waves up, where the records have left the caches by the time
 *                  they are read).
 *   PM_OPT_CLUSTER (default 1): subtree form -- the Fitch post-order runs as LDS-staged
 *                  sweeps from the first height above which the tree's bands are chain-like and
 *                  hold at most 16384 clusters (deep ladder trees: every height; a random-join
 *                  tree: none): bands of heights, one wave per (connected cluster of the band,
 *                  2048-site tile) walking the cluster's nodes depth first with its inner sets
 *                  in LDS.  When every height is swept, the pre-order (Fitch and Sankoff) and
 *                  the Sankoff post-order (nodes of <= 255 children) run over the same clusters.
 *                  0 = the level kernels everywhere.  A value >= 2 instead takes every height
 *                  from the first whose level (and every level above it) holds at most that
 *                  many nodes.  Takes effect at the next pm_tree_upload; results identical.
 *   PM_OPT_VCF_BATCH_BYTES (default 1 GiB, at least 4096): pm_vcf / pm_vcf_fd produce and
 *                  stream the genotype text in batches of whole lines of at most this many
 *                  bytes (always at least one line), so the device never holds lines x samples
 *                  at once.  The text does not depend on it.
 *   PM_OPT_MAF_BATCH_BYTES (default 1 GiB, at least 4096): pm_maf / pm_maf_fd produce and
 *                  stream the text in batches of whole lines of at most this many bytes
 *                  (always at least one line).  The text does not depend on it.
 *   PM_OPT_GFA_BATCH_BYTES (default 1 GiB, at least 4096): pm_gfa / pm_gfa_fd produce and
 *                  stream the "P" lines in batches of whole lines of at most this many bytes
 *                  (always at least one line).  The text does not depend on it.
 *   PM_OPT_GFA_IN_BATCH_SITES (default and most 2^24 - 1, the most sites pm_leaves_upload takes;
 *                  at least 1): pm_gfa_build uploads and runs the block columns in batches of at
 *                  most this many.  The result does not depend on it.
 *   PM_OPT_SUBNET_BATCH_ENTRIES (default 2^25, 1 .. 2^31 - 2): pm_subnet expands, sorts and folds the merged
 *                  chains' nucleotide mutations in batches of whole new nodes of at most this many bases (a node
 *                  whose chain holds more gets a batch of its own).  The result does not depend on it.
 *   PM_OPT_AA_BATCH_BYTES (default 1 GiB, at least 4096): pm_aa / pm_aa_fd build the codon tables and
 *                  the lines of a batch of nodes in at most this much device memory (always at least
 *                  one node) and stream the text batch by batch.  The text does not depend on it.
 *   PM_OPT_MUTATIONS_BATCH_BYTES (default 1 GiB, at least 4096): pm_print_mutations / pm_print_mutations_fd
 *                  cut the nodes in id order into batches by the bytes of their entry records plus the
 *                  worst-case text (a node above the limit runs alone) and stream the text batch by
 *                  batch.  The text does not depend on it.
 *   PM_OPT_REROOT_CHUNK_SITES (default 0, or 1 .. 2^24 - 4096): pm_reroot runs the nucleotide Fitch over the
 *                  canonical columns in chunks.  0 sizes a chunk from the tree alone (at least 65536 columns, at
 *                  most 2^24 - 4096, as many as fit 24 GiB of sets, finals and codes); another value is the
 *                  chunk, capped by that size.  Odd values are allowed: a chunk may start on an odd column.  The
 *                  result does not depend on it.
 *   PM_OPT_USHER_BATCH_BYTES (default 1 GiB, at least 4096): pm_to_usher / pm_to_usher_fd cut the nodes in
 *                  pre-order into batches by the bytes of their entry records, sort keys and worst-case
 *                  output (a node above the limit runs alone) and stream the bytes batch by batch.  The
 *                  bytes do not depend on it.
 *   PM_OPT_IMPUTE_BATCH_ENTRIES (default 2^25, 1 .. 2^31 - 2): pm_impute lays out, sorts and folds the path lists of
 *                  whole (node, candidate) pairs of at most this many bases per batch (a pair whose path holds
 *                  more gets a batch of its own), and sorts the cells of whole nodes' lists in batches of the
 *                  same size.  The result does not depend on it.
 * (Option ids 1, 4, 5 and 11 -- subtree-region, heavy-path-chain and level-band schedules,
 * tail records overlapped with the pre-order levels -- were measured slower than, or no
 * faster than, the level kernels on MI355X and removed.) */
#define PM_OPT_VIRTUAL 2
#define PM_OPT_GRAPH 3
#define PM_OPT_SUBTREE 6
#define PM_OPT_NARROW 7
#define PM_OPT_GROUP_WAVES 8
#define PM_OPT_GROUP_LEVELS 9
#define PM_OPT_UP_GROUP 10
#define PM_OPT_RECORD_CAP 12
#define PM_OPT_SUB_DOWN 13
#define PM_OPT_PLAIN_UP 14
#define PM_OPT_NT_LOADS 16
#define PM_OPT_CLUSTER 17
#define PM_OPT_TAIL_PACK 18
#define PM_OPT_VCF_BATCH_BYTES 19
#define PM_OPT_MAF_BATCH_BYTES 20
#define PM_OPT_GFA_BATCH_BYTES 21
#define PM_OPT_DOWN_PACK 22
#define PM_OPT_GFA_IN_BATCH_SITES 23
#define PM_OPT_SUBNET_BATCH_ENTRIES 24
#define PM_OPT_AA_BATCH_BYTES 25
#define PM_OPT_MUTATIONS_BATCH_BYTES 26
#define PM_OPT_REROOT_CHUNK_SITES 27
#define PM_OPT_USHER_BATCH_BYTES 28
#define PM_OPT_IMPUTE_BATCH_ENTRIES 29
int pm_set_option(pm_ctx* ctx, int option, int64_t value);
/* Accumulate per-kernel-class device time with HIP events (see pm_kernel_times). */
int pm_set_profiling(pm_ctx* ctx, int enable);

/* Upload the topology (host arrays).  Levels, dense indices and the device copy are built
 * here, once; replaces the recursion over Node* children in every per-column call. */
int pm_tree_upload(pm_ctx* ctx, const pm_tree* tree);

/* Upload the leaf columns.  Replaces the per-column `states` maps of the drivers
 * (src/panman.cpp:1409-1417 Fitch, :1574-1582 Sankoff).
 *   codes4[row * row_stride + s/2]: 4-bit code of site s for alignment row `row`.
 *   node_row[node]: the row of leaf `node`, or -1 if the leaf is absent from the
 *     alignment (reference: state 0 / all-INF, src/fitchSankoff.cpp:33-36, :362-368).
 *   present (nullable): per-row bitmask of present sites (bit s%8 of byte
 *     row * present_stride + s/8); a cleared bit makes that (leaf, site) absent, as the
 *     PanGraph driver does for leaves lacking a block (src/panman.cpp:1026-1028). */
int pm_leaves_upload(pm_ctx* ctx, int64_t num_sites, const uint8_t* codes4, int64_t row_stride,
                     const int32_t* node_row, const uint8_t* present, int64_t present_stride);

/* The same upload from sparse rows: equivalent to pm_leaves_upload (present = NULL) of the dense
 * matrix that holds `fill_code` everywhere except code[i] at (row, site[i]) for the entries
 * i in [row_off[row], row_off[row + 1]) of each row.  For matrices that are almost entirely one
 * code, as the block states of a GFA are (paths x segments, src/panman.cpp:784-797: "absent"
 * wherever the path has no step): the host validates and uploads only the three arrays, and a
 * kernel expands them into the packed staging rows on the device.
 *   row_off [num_rows + 1], row_off[0] = 0, non-decreasing;
 *   site    [nnz] strictly increasing within a row, 0 <= site < num_sites;
 *   code    [nnz] 0..15; fill_code 0..15;
 *   node_row[node] < num_rows (-1: the leaf is absent).
 * The same state and errors as pm_leaves_upload; PM_ERR_ARG for an entry or a node_row outside
 * those ranges. */
int pm_leaves_upload_sparse(pm_ctx* ctx, int64_t num_sites, int32_t num_rows, const int64_t* row_off,
                            const int32_t* site, const uint8_t* code, uint8_t fill_code, const int32_t* node_row);

/* Per-site constants (packed codes, ceil(S/2) bytes each).
 *   consensus: the root's parent state, i.e. the block consensus character
 *     (src/panman.cpp:1424-1425, :1600-1606).
 *   forced (nullable): Fitch: refState forcing the root forward set (:1419);
 *     Sankoff: defaultState forcing the root (:1583-1596). */
int pm_sites_upload(pm_ctx* ctx, const uint8_t* consensus4, const uint8_t* forced4);

/* Run post-order, pre-order and mutation assignment for every uploaded site (async). */
int pm_run(pm_ctx* ctx, int mode);

/* Results (synchronise the stream). */
int pm_mutation_count(pm_ctx* ctx, int64_t* count);
/* Records sorted by (node, site); `cap` records fit in `out`. */
int pm_mutations_fetch(pm_ctx* ctx, pm_mut* out, int64_t cap, int64_t* count);
/* Per site: number of mutated edges below the root (parsimony score of the assignment)
 * and the root's final code (255 = unresolved).  Either pointer may be NULL. */
int pm_site_results(pm_ctx* ctx, int32_t* score, uint8_t* root_code);
/* Same, copied device-to-device into caller buffers on the ctx stream (async after the
 * record-buffer check, which synchronises), so that a collective can gather them without a
 * host copy. */
int pm_site_results_device(pm_ctx* ctx, void* score_device, void* root_code_device);
/* Accumulated device milliseconds and launch counts per kernel class since the last
 * call; classes: 0 post-order, 1 pre-order + assignment (levels, bands, sweeps), 2 score
 * histogram, 3 replay, 4 whole pm_run replayed from a hipGraph (PM_OPT_GRAPH), 5 the
 * pre-order's tail launch (children beyond the second, S2 / S3 subtrees). */
int pm_kernel_times(pm_ctx* ctx, double* ms, int64_t* launches, int classes);

/* ---- multi-GPU column shards ----------------------------------------- */
/* The reference runs one parsimony call per column (src/panman.cpp:1381 Fitch, :1568
 * Sankoff) -- columns are independent, so each GPU owns a contiguous site range with the
 * tree replicated.  The per-site results (parsimony score, root code) are reassembled with
 * ONE RCCL all-gather over xGMI; mutation records stay on their rank (site indices local
 * to the shard) and merge on the host by (node, site_begin + site).  RCCL is opened at run
 * time (librccl.so.1; inside a PyTorch process, torch's own copy).
 *   pm_comm_unique_id   rank 0 makes the id (ncclGetUniqueId); the caller broadcasts it.
 *   pm_comm_init_rank   one process per GPU: bind ctx to rank `rank` of `nranks`.
 *   pm_comm_init_all    one process, several GPUs: ncclCommInitAll over the ctxs' devices
 *                       (distinct devices; rank i = ctxs[i]).
 *   pm_run_gather       pm_run on this rank's shard [site_begin, site_begin + uploaded
 *                       sites) of `total_sites`, then the all-gather: score_device
 *                       [total_sites] int32 and root_device [total_sites] u8 (device
 *                       memory) receive every rank's sites.  Every rank must call it; it
 *                       returns when the gathered vectors are complete.  A rank whose shard
 *                       fails (bad range, run error) still joins the collective with a
 *                       failed chunk head, so every rank returns an error instead of one
 *                       rank leaving the others blocked.  Shards hold at most
 *                       ceil(total/ranks)+2 sites.
 *   pm_multi_run        the same for pm_comm_init_all contexts from one thread (RCCL group
 *                       call); site_begin[i] per ctx; results to host (nullable).
 *   pm_shard_range      the balanced rule [r*S/n, (r+1)*S/n) bench.py and shard.py use.
 * The gathered unit is one chunk per rank of `per` = ceil(S/ranks)+3 u64 entries: entry 0 =
 * site_begin << 32 | count (count 0xffffffff: that rank failed), then one entry per site =
 * score (int32) | root code << 32.  The same layout moves through any other collective:
 *   pm_pack_site_results    the ctx's last run into a chunk in device memory; syncs;
 *   pm_unpack_site_results  ranks x per gathered entries (device) into score / root device
 *                           vectors; checks the heads (failed rank, overlaps, gaps); syncs.
 *   pm_chunk_entries / pm_chunk_pack / pm_chunk_unpack  the same on host memory, no GPU. */
#define PM_COMM_ID_BYTES 128
int pm_comm_unique_id(uint8_t* id, int64_t len);
int pm_comm_init_rank(pm_ctx* ctx, const uint8_t* id, int nranks, int rank);
int pm_comm_init_all(pm_ctx* const* ctxs, int n);
int pm_run_gather(pm_ctx* ctx, int mode, int64_t total_sites, int64_t site_begin, void* score_device,
                  void* root_device);
int pm_multi_run(pm_ctx* const* ctxs, int n, int mode, const int64_t* site_begin, int64_t total_sites,
                 int32_t* score, uint8_t* root_code);
int pm_shard_range(int rank, int ranks, int64_t total_sites, int64_t* begin, int64_t* end);
int pm_pack_site_results(pm_ctx* ctx, int64_t site_begin, int64_t per, void* chunk_device);
int pm_unpack_site_results(pm_ctx* ctx, const void* all_device, int64_t per, int ranks, int64_t total_sites,
                           void* score_device, void* root_device);
int pm_chunk_entries(int64_t total_sites, int ranks, int64_t* per);
int pm_chunk_pack(int64_t site_begin, int64_t count, const int32_t* score, const uint8_t* root, int64_t per,
                  uint64_t* chunk);
int pm_chunk_unpack(const uint64_t* all, int64_t per, int ranks, int64_t total_sites, int32_t* score,
                    uint8_t* root);

/* ---- measurement (bench.py roofline; not part of the reference interface) ------------ */
/* Bytes this design must move in the last pm_run (nucleotide modes), counted from the run's
 * record masks at the kernels' 16-B-per-lane granularity: out[0] post-order (leaf words,
 * child records read, own record + masks written), out[1] pre-order + assignment (own
 * record, parent final, dirty-lane leaf words, compact finals, 8 B per mutation record),
 * out[2] score histogram, out[3] floor = 0.5 B per leaf-site + 8 B per record, out[4] the
 * record count; with n >= 14, out[5..13] split them: post-order leaf words, child records read,
 * own records + pushed masks written; pre-order own records, parent finals, dirty-lane leaf
 * words of the nodes' first two children (k_down), finals written, tail items and their
 * dirty-lane leaf words (k_tail).  With the LDS-staged sweeps (PM_OPT_CLUSTER) a child record
 * read from an LDS slot, and a parent final likewise, is not counted.  With n >= 20, out[14..19]:
 * the pre-order's reads at 128-B line granularity (every line a load touches, as the memory
 * fetches them: tools/calib_fetch.hip) -- level kernels: descriptors + masks + own records,
 * parent finals, dirty-lane leaf words; tail: descriptors + masks, dirty-lane leaf words,
 * parent finals.  In the levels PM_OPT_DOWN_PACK packed, own simple codes and parent finals count
 * at live lanes only, as the packed kernel reads them.  With n >= 31, out[20..30]: the live lanes
 * of those levels' (node, tile) waves -- or, the option off, of the levels it would pack -- as
 * waves counted, live lanes in total and a histogram of live lanes per wave (0, 1-8, 9-16, ..,
 * 57-64).  `n` >= 5.
 * Synchronises the ctx stream. */
int pm_design_bytes(pm_ctx* ctx, double* out, int n);
/* FETCH_SIZE calibration for scattered reads: `lanes` threads each read 4 x 16 B, one 16-B
 * slot every `stride_bytes` (16 = a coalesced stream), and write 16 B coalesced; `reps`
 * launches, *ms_per_launch their average (profile it with rocprofv3 --pmc FETCH_SIZE). */
int pm_gather_probe(int device, int64_t lanes, int stride_bytes, int reps, double* ms_per_launch);
/* Device bytes the context holds now (n entries of): out[0] total, [1] leaf rows (code planes,
 * presence, flags), [2] the S2 / S3 side-by-side leaf copy, [3] state-set records, [4] record
 * masks, [5] Sankoff part counters, [6] mutation-record shards, [7] the flattened tree
 * (descriptors, level tables), [8] per-site columns (consensus, forced, finals of the root,
 * score, root code), [9] replay rows, FASTA text, gather and generator buffers.  No GPU call. */
int pm_memory_footprint(pm_ctx* ctx, int64_t* out, int n);
/* Hash of the library's sources (16 hex digits): profiled PMC traffic is tied to it. */
const char* pm_build_id(void);
/* Achievable HBM rate on `device`: a 16-B-per-lane streaming copy of `bytes` bytes, `reps`
 * times; *gbs = (read + write bytes) / s / 1e9. */
int pm_stream_copy_rate(int device, int64_t bytes, int reps, double* gbs);
/* The same for writes only (the replay rows' access pattern): 16 B per lane, 4 non-temporal
 * stores in flight; *gbs = written bytes / s / 1e9. */
int pm_stream_write_rate(int device, int64_t bytes, int reps, double* gbs);

/* Phase log: the drivers (pm_fasta, pm_msa_build / pm_msa_to_panman*, pm_panman_load /
 * pm_panman_write, pm_create) append the wall time of each host / device phase of every
 * call to one process-wide log.  pm_phase_report writes it as "name\tseconds\n" lines into
 * buf (truncated to len - 1 bytes, NUL-terminated) and returns the bytes the whole report
 * needs (with the NUL); pm_phase_reset empties it (it also stops growing at 4096 entries). */
void pm_phase_reset(void);
int64_t pm_phase_report(char* buf, int64_t len);

/* ---- column drivers ------------------------------------------------------------------ */
/* Drop-in for Tree(msa, newick, FILE_TYPE::MSA (mode PM_MODE_FITCH, "M1") or
 * FILE_TYPE::MSA_OPTIMIZE (PM_MODE_SANKOFF, "M2"), reference) -- src/panman.cpp:1274-1649:
 * Newick + aligned FASTA text -> consensus block, root block insertion and every node's
 * NucMut list (grouped as src/panman.cpp:1445-1466), computed on `device`.  Returns a
 * malloc'd text dump (release with pm_free):
 *   "#consensus\t<seq>\n" "#blockmut\t<root>\t0\t-1\t1\t0\n" then one line per NucMut,
 *   nodes in name order: "<node>\t<nucPosition>\t<nucGapPosition>\t<mutInfo>\t<nucs %06x>\n";
 * or "#error\t<message>\n" where the reference would exit or has undefined behaviour. */
char* pm_msa_build(const char* newick, const char* msa_text, const char* reference, int mode, int device);
void pm_free(void* p);
/* The same construction written as a PanMAN file (Tree(...) + writePanMAN,
 * src/panmanUtils.cpp:1409-1465, :271-299): one tree, one block. */
int pm_msa_to_panman(const char* newick, const char* msa_text, const char* reference, int mode, int device,
                     const char* out_path, char* err, int64_t err_len);
/* The same with the columns split into contiguous ranges over `devices` (one host thread
 * and context each; entries may repeat); records are merged by (node, site) on the host,
 * so the file is byte-identical to the single-device build. */
int pm_msa_to_panman_multi(const char* newick, const char* msa_text, const char* reference, int mode,
                           const int* devices, int num_devices, const char* out_path, char* err, int64_t err_len);

/* ---- root-to-leaf mutation replay (FASTA extraction) ---------------------------------- */
/* PanMAT fields used by printFASTAUltraFast (src/panman.hpp:520-543 Block / GapList,
 * :429-517 BlockMut, :75-313 NucMut, Tree::circularSequences / rotationIndexes /
 * sequenceInverted).  Per-node lists are CSR in list order; arrays are host memory. */
typedef struct pm_panmat {
    int32_t num_nodes;
    int32_t root;
    const int32_t* child_offsets;    /* [num_nodes + 1] */
    const int32_t* child_index;
    const char* names;               /* num_nodes NUL-terminated identifiers, back to back */
    int32_t num_blocks;
    const int32_t* block_primary;    /* [num_blocks] primaryBlockId */
    const int64_t* block_seq_offsets;/* [num_blocks + 1] into block_seq */
    const uint32_t* block_seq;       /* consensusSeq: 8 codes per word, MSB first, code 0 ends */
    int32_t num_gaps;
    const int32_t* gap_primary;      /* [num_gaps] */
    const int64_t* gap_offsets;      /* [num_gaps + 1] into gap_position / gap_length */
    const uint32_t* gap_position;
    const uint32_t* gap_length;
    const int64_t* block_mut_offsets;/* [num_nodes + 1] */
    const int32_t* block_mut_primary;
    const uint8_t* block_mut_info;   /* 1 = insertion (BI), 0 = deletion / inversion */
    const uint8_t* block_mut_inversion;
    const int64_t* nuc_mut_offsets;  /* [num_nodes + 1] */
    const int32_t* nuc_mut_primary;
    const int32_t* nuc_mut_secondary;
    const int32_t* nuc_mut_position;
    const int32_t* nuc_mut_gap_position; /* -1 = main position */
    const uint8_t* nuc_mut_info;     /* (length << 4) | type */
    const uint32_t* nuc_mut_nucs;    /* code i at bits 4 * (5 - i) */
    const int32_t* circular_offset;  /* nullable [num_nodes]; < 0 = not circular */
    const int32_t* rotation_index;   /* nullable [num_nodes] */
    const uint8_t* sequence_inverted;/* nullable [num_nodes] */
    const float* branch_length;      /* nullable [num_nodes]; Newick branch lengths (root 0) */
} pm_panmat;

/* Drop-in for Tree::printFASTAUltraFast(fout, aligned) (src/fasta.cpp:1981-2099): one
 * record per leaf, ">name\n" + 70-column lines + "\n", leaves in node-id order (the
 * reference's order is TBB-scheduled).  `*text` is malloc'd (release with pm_free).
 * Replay runs on the GPU (consensus expansion + path mutations per leaf); block order,
 * strands, rotation, circular offset and line wrapping are applied by the host formatter.
 * A nucleotide mutation's secondary block id is ignored (applied to its primary block), as
 * printFASTAUltraFastHelper does (src/fasta.cpp:1838-1842).
 * Memory: the replayed rows (leaves x columns bytes) and the text stay on the device in
 * grow-only per-context buffers until pm_destroy, so the next pm_fasta on the context does not
 * allocate again; a later large allocation on the context that fails releases them and
 * retries once. */
int pm_fasta(pm_ctx* ctx, const pm_panmat* panmat, int aligned, char** text, int64_t* length);
/* pm_fasta over several devices: leaves split into contiguous ranges, one host thread and
 * context per entry of `devices` (entries may repeat), texts concatenated in leaf order --
 * byte-identical to pm_fasta.  On failure `err` receives the first shard's reason. */
int pm_fasta_multi(const pm_panmat* panmat, int aligned, const int* devices, int num_devices, char** text,
                   int64_t* length, char* err, int64_t err_len);
/* The same in stages: prepare (host flattening + upload), run (GPU replay, async on the
 * ctx stream; profiling class 3), format (download + text). */
int pm_replay_prepare(pm_ctx* ctx, const pm_panmat* panmat);
/* Prepare only leaves [leaf_begin, leaf_end) of the PanMAT (leaves in node-id order): one
 * GPU's shard when FASTA extraction is split by leaves. */
int pm_replay_prepare_range(pm_ctx* ctx, const pm_panmat* panmat, int64_t leaf_begin, int64_t leaf_end);
int pm_replay_run(pm_ctx* ctx);
int pm_replay_format(pm_ctx* ctx, int aligned, char** text, int64_t* length);
/* The same FASTA text written to the file descriptor `fd` (a pipe, stdout, a file) instead of
 * returned: the device text streams through pinned slots to `fd` while later chunks are still
 * in flight, with no host copy of the whole text.  `length` (nullable): the bytes written.
 * pm_fasta_fd = pm_fasta to a descriptor; pm_fasta_multi_fd = pm_fasta_multi to a descriptor
 * (the shards' texts in leaf order).  A failed write returns PM_ERR_ARG (errno kept). */
int pm_replay_format_fd(pm_ctx* ctx, int aligned, int fd, int64_t* length);
int pm_fasta_fd(pm_ctx* ctx, const pm_panmat* panmat, int aligned, int fd, int64_t* length);
int pm_fasta_multi_fd(const pm_panmat* panmat, int aligned, const int* devices, int num_devices, int fd, int64_t* length,
                      char* err, int64_t err_len);
/* Drop-in for Tree::printVCFParallel(refnode, fout) (src/vcf.cpp:177-382; the --vcf command,
 * src/panmanUtils.cpp:654-697): the variants of every tip against the tip named `reference`.
 * A tip's row is what pm_fasta(aligned = 1) prints for it without the line breaks (block print
 * order, rotation, inversion, strands and absent-block dashes included); a tip whose row
 * length differs from the reference tip's is not compared (vcf.cpp:229-232): it stays a sample
 * column of zeros and is counted in `*skipped` (nullable).  Each compared tip is scanned left
 * to right with the reference's rules (differences merge until the next column where both
 * rows hold the same base, which anchors the next difference; a leading insertion is closed by
 * that base instead).  Text: the four ## header lines (fileDate = year, month, day unpadded,
 * local time), the #CHROM line with the samples -- every tip but the reference in byte order
 * of the names -- and one line per distinct (POS, REF) in (POS, REF bytes) order, ID the
 * running line number from 0, ALT the distinct ALTs in byte order (an empty REF or ALT is "."),
 * ".\t.\t.\t.", then per sample the 1-based index of its ALT, or 0.
 * The rows are replayed and compared on the GPU (profiling class 3); the host groups the
 * records into lines; the genotype text is produced on the device in batches
 * (PM_OPT_VCF_BATCH_BYTES) and streamed through the pinned download slots.  Phase log: vcf.*.
 * `*text` is malloc'd (release with pm_free); pm_vcf_fd writes to `fd` instead (`length`
 * nullable).  Errors: an unknown `reference`, one that is not a tip, or fewer than two tips:
 * PM_ERR_ARG; a failed write: PM_ERR_ARG (errno kept), as pm_fasta_fd. */
int pm_vcf(pm_ctx* ctx, const pm_panmat* panmat, const char* reference, char** text, int64_t* length,
           int64_t* skipped);
int pm_vcf_fd(pm_ctx* ctx, const pm_panmat* panmat, const char* reference, int fd, int64_t* length,
              int64_t* skipped);
/* Drop-in for Tree::printMAF(fout) (src/maf.cpp:68-188; the --maf command,
 * src/panmanUtils.cpp:741-763): the multiple whole-genome alignment, block by block.  Tips are
 * the leaves in node-id order (the order pm_fasta prints its records).
 *   text(t, b)  block b's canonical, forward row of tip t (per main position its gap slots,
 *               then its main character, the end sentinel last) with every 'x' printed as '-',
 *               as getBlockSequenceFromReference builds it (src/panman.cpp:3070-3261); a
 *               reverse strand only changes the strand field.
 *   size(t, b)  the characters of text(t, b) that are not '-' (stripGaps).
 *   start(t, b) the sum of size(t, b') over the blocks b' the tip holds that come before b in
 *               the tip's print order (block ids rotated left to the rotation_index-th held
 *               block, then reversed when sequence_inverted: getSequenceFromReference(rotate =
 *               true), src/panman.cpp:4974-4999); with circular_offset >= 0 the offset is
 *               subtracted and, if the result is negative, srcSize added once (maf.cpp:125-136:
 *               no modulo, so an offset above srcSize prints a negative start).
 *   srcSize(t)  the sum of size(t, b) over the blocks the tip holds.
 * Text: "##maf version=1\n"; then one paragraph per group of blocks with equal consensusSeq
 * words (the raw block_seq words), groups in lexicographic order over unsigned words with a
 * proper prefix first (std::map<std::vector<uint32_t>, ...>), blocks of a group in block-list
 * order: "a\n", per block and per tip that holds it
 * "s\t<name>\t<start>\t<size>\t<+ or ->\t<srcSize>\t<text>\n", then "\n" -- also for a group
 * no tip holds.  Inside a block the lines are in tip order (the reference iterates a
 * concurrent map there: scheduler-defined).
 * Sizes, starts, line lengths and the text are computed on the GPU from the replayed rows
 * (profiling class 3), the text in batches of whole lines (PM_OPT_MAF_BATCH_BYTES) streamed
 * through the pinned download slots.  Phase log: maf.*.
 * `*text` is malloc'd (release with pm_free); pm_maf_fd writes to `fd` instead (`length`
 * nullable).  Errors: a PanMAT with a nucleotide mutation on a secondary block:
 * PM_ERR_UNSUPPORTED (getBlockSequenceFromReference skips it where the replay applies it to the
 * primary block); no tip: PM_ERR_ARG; a failed write: PM_ERR_ARG (errno kept), as pm_fasta_fd. */
int pm_maf(pm_ctx* ctx, const pm_panmat* panmat, char** text, int64_t* length);
int pm_maf_fd(pm_ctx* ctx, const pm_panmat* panmat, int fd, int64_t* length);
/* Drop-in for Tree::convertToGFA(fout) (src/gfa.cpp:3-500; the --gfa command,
 * src/panmanUtils.cpp:699-732): the tips as paths through a sequence graph.  Tips are the leaves
 * in node-id order.  The reference has two branches.
 * A. No node carries a nucleotide mutation (gfa.cpp:13-118), a graph of whole blocks:
 *   "S\t<id>\t<text>\n" per block, id = the rank from 0 of its primary id, text = its
 *   consensusSeq words, each decoded up to its first code 0 -- also for a block no tip holds;
 *   a tip holds a block when the last block mutation of it on the tip's path is an insertion
 *   (anything else, an inversion included, clears it; no strands here);
 *   "L\t<a>\t+\t<b>\t+\t0M\n" per distinct pair of blocks consecutive in a tip's path (the held
 *   blocks in id order), pairs in ascending (from, to) order;
 *   "P\t<name>\t<a>+,<b>+\t*\n" per tip, in tip order.  No "H" line.  (A held id that is no
 *   block's prints as 0, as the reference's map lookup does.)
 * B. Otherwise (gfa.cpp:119-499), a graph of 32-column chunks of the canonical rows
 *   rows[tip][blk_lo .. blk_hi) of getSequenceFromReference(rotate = false): rotation, sequence
 *   inversion and circular offset play no part.
 *   chunks   of a forward block: 32 columns each from the block's first column, the last one
 *            shorter; of a reverse block: 32 columns each from the block's last column down, the
 *            short one at the block's beginning, walked from the last chunk of the row to the
 *            first and read in canonical order (not complemented).
 *   node     (start, string): string = the chunk without '-' and 'x' (an empty one makes no node
 *            and no path step); start = the chunk's first column as (block, position, gap slot)
 *            on the forward strand, its lowest column as (-block - 1, position, -1) or
 *            (-block, position, gap slot) on the reverse strand -- so block 0's reverse gap-slot
 *            starts collide with forward starts, as they do in the reference.
 *   ids      a new node gets the next id from 0 and the strand of the tip that made it.  Defined
 *            schedule: tips in order, each completely before the next; blocks ascending; chunks
 *            in walk order.  (The reference runs the tips under tbb::parallel_for_each.)
 *   Then the reference's chain compaction, duplicate removal and renumbering (gfa.cpp:311-472),
 *   restated literally on the host over the integer ids, tip names compared by their bytes.
 *   Text: "H\tVN:Z:1.1\n"; "S\t<id>\t<text>\n" per final node; "L\t<a>\t<+|->\t<b>\t<+|->\t0M\n"
 *   in the edge set's order; "P\t<name>\t<id><+|->,...\t*\n" per tip in tip order ("P\t<name>\t\t*\n"
 *   for a tip without a step; the reference iterates a concurrent map here).
 * Chunk keys, the exact unique over them (radix sort of the whole keys, neighbours compared in
 * full), the ids and the "P" lines are computed on the GPU (profiling class 3), the "P" lines in
 * batches of whole lines (PM_OPT_GFA_BATCH_BYTES) streamed through the pinned download slots;
 * "H", "S" and "L" come from the host.  Phase log: gfa.*.
 * `*text` is malloc'd (release with pm_free); pm_gfa_fd writes to `fd` instead (`length`
 * nullable).  Errors: a nucleotide mutation on a secondary block: PM_ERR_UNSUPPORTED (as pm_maf);
 * no tip: PM_ERR_ARG; in branch A a block mutation's id >= num_blocks + 1: PM_ERR_ARG (the
 * reference indexes out of range); rows of 2^31 columns or more, or 2^31 path steps or more:
 * PM_ERR_UNSUPPORTED; a failed write: PM_ERR_ARG (errno kept), as pm_fasta_fd. */
int pm_gfa(pm_ctx* ctx, const pm_panmat* panmat, char** text, int64_t* length);
int pm_gfa_fd(pm_ctx* ctx, const pm_panmat* panmat, int fd, int64_t* length);
/* Drop-in for Tree::extractAminoAcidTranslations(fout, start, end) (src/aaTrans.cpp:185-304; the
 * --aa-translation command, src/panmanUtils.cpp:895-938): per node of the tree, internal ones
 * included, the amino-acid substitutions, insertions and deletions of the window between two
 * global coordinates against the root's.  Rotation, sequence inversion and circular offset play
 * no part (getSequenceFromReference(rotate = false)); a node's sequence is its canonical row:
 * per held block, per position 0..n_b (n_b the 'x' sentinel) its gap slots, then its main
 * character.  An absent block counts as forward.
 *   locate(v, g)  globalCoordinateToBlockCoordinate with circular offset 0 (src/panman.cpp:
 *                 5726-5798): L = the characters of v's held blocks that are neither '-' nor 'x';
 *                 g' = g when g < L, else g - L (one wrap: a negative or still too large g' is not
 *                 found); held blocks in ascending id, a forward block's positions ascending (slots
 *                 ascending, then the main character), a reverse block's descending (the main
 *                 character, then slots descending); the g'-th such character is (b, j, k), k = -1
 *                 for a main character.
 *   window(v, S = (b0, j0, k0), E)  getNucleotideSequenceFromBlockCoordinates (aaTrans.cpp:3-67),
 *                 quirks included.  For every id b0..b1 (an id without a block has no position; a
 *                 block that is not held emits '-' per character): a forward block walks j from
 *                 (i == b0 ? j0 : 0) up to n_i, in every position the slots k0.. when k0 >= 0 and no
 *                 slot at all when k0 == -1 (the reference's slot loop always starts at
 *                 get<3>(start)), then the main character; a reverse block walks j from
 *                 (i == b0 ? j0 : n_0) down to 0 -- n_0 being block id 0's last index, as the
 *                 reference reads sequence[0] -- the main character first, then the slots from
 *                 (i == b0 and j == j0 ? k0 : the last) down to 0.  Before every character the
 *                 walk stops if its coordinate is E; a walk that never stops is "ERROR".
 *   codons(W)     every character that is not A, C, G or T becomes '-'; the others are grouped in
 *                 threes in order, codon c = (amino acid of the standard genetic code as its
 *                 three-letter name, "*" for TAA, TAG and TGA; the window index of its first and
 *                 of its third character); an incomplete last group is dropped; "ERROR": none.
 * The call: every node, the root included, is located and windowed on its own row; a node whose S
 * or E is not found is counted in `*unlocated` and prints no line.  Every node's codons are merged
 * against the root's (aa, start, end) lists with the reference's two-pointer loop
 * (aaTrans.cpp:259-285); a node whose window is "ERROR" has no codons, so every root codon is a
 * deletion.  A node's string: "S:<root index>:<AA>;" per match whose amino acid differs, then
 * "I:<root index>:<AA>;" per insertion, then "D:<root index>;" per deletion.
 * Text: "node_id\taa_mutations\n", then "<name>\t<string>\n" per node with a non-empty string.
 * `*ref_codons` = the root's codon count (the reference prints it three times on stdout); when it
 * is 0 the text is empty and the call returns PM_OK, as the reference returns before its header.
 * Deviations: lines are in node-id order (the reference iterates a tbb::concurrent_unordered_map);
 * a root window that is "ERROR" returns PM_ERR_ARG (the reference goes on and reports every node's
 * codons as insertions at 0); a reverse-strand block i != b0 inside some located node's window
 * with n_0 > n_i, or without a block of id 0, returns PM_ERR_UNSUPPORTED (the reference indexes
 * out of range there).
 * The rows of all nodes come from one replay of a derived PanMAT in which every internal node has
 * one more childless child without mutations (that child's row is the node's), so the replay
 * kernels are pm_fasta's.  Per-block sizes, the rank-select of both coordinates, the codon tables,
 * the merge (an order-free form of the two-pointer loop, one codon per lane), the line lengths and
 * the text are computed on the GPU (profiling class 3), batch by batch of nodes
 * (PM_OPT_AA_BATCH_BYTES), the text streamed through the pinned download slots.  Phase log: aa.*.
 * Memory: the replayed rows are nodes x columns bytes, as leaves x columns for the other
 * extractions; sharding by node ranges and a window-only replay are not implemented.
 * `*text` is malloc'd (release with pm_free); pm_aa_fd writes to `fd` instead (`length`,
 * `ref_codons`, `unlocated` nullable).  Errors: end <= start: PM_ERR_ARG ("End coordinate must be
 * greater than start"); the root's S or E not found: PM_ERR_ARG ("coordinates out of range"); a
 * nucleotide mutation on a secondary block: PM_ERR_UNSUPPORTED (as pm_maf); rows of 2^31 columns
 * or more: PM_ERR_UNSUPPORTED; a failed write: PM_ERR_ARG (errno kept), as pm_fasta_fd. */
int pm_aa(pm_ctx* ctx, const pm_panmat* panmat, int64_t start, int64_t end, char** text, int64_t* length,
          int64_t* ref_codons, int64_t* unlocated);
int pm_aa_fd(pm_ctx* ctx, const pm_panmat* panmat, int64_t start, int64_t end, int fd, int64_t* length,
             int64_t* ref_codons, int64_t* unlocated);
/* Drop-in for Tree::printMutationsNew(std::ostream&) (src/panman.cpp:3699-4057; the --printMutations
 * command without --input-file, src/panmanUtils.cpp:1008-1071): per node of the tree, which bases
 * changed against its parent, in the root's coordinates.  Rotation, sequence inversion and circular
 * offset play no part.  A node's sequence is getSequenceFromReference(rotate = false) (src/panman.cpp:
 * 4676-4972): all block mutations of its path first, then the nucleotide mutations of the blocks it
 * holds at the end of the path only, so a block it does not hold keeps its consensus and its empty
 * gap slots.  A cell is (block, position 0..n_b, slot), slot -1 the main character, n_b the 'x'
 * sentinel.
 *   root map      (:3725-3806) the root's blocks by id; a held forward block is walked per position
 *                 (slots ascending, then the main character), a held reverse block with positions
 *                 descending (the main character, then the slots descending).  coord(cell) = the root
 *                 characters that are neither '-' nor 'x' walked before the cell; gap(cell) = the
 *                 root's own character there is '-' or 'x'.  In a block the root does not hold every
 *                 cell gets the running count unchanged and gap = false.
 *   seqChar(u)    (:3810-3849) a slot: u's character, 'x' as '-', with no held test.  A main character
 *                 of a block whose strand flag is forward: u's character if it is neither '-' nor 'x'
 *                 and u holds the block, else '-'.  Of a block whose flag is reverse: the ROOT's
 *                 stored main character at that position, unnormalised ('x' at the sentinel), if u's
 *                 is neither '-' nor 'x', else '-' (a quirk of :3835, kept).
 *   entries       only the node's own nucleotide mutations, in list order (:3901); the root has none.
 *                 held(u, b) starts from the root's held blocks; an insertion anywhere on the path
 *                 sets it, a deletion that is no inversion clears it (:3874-3899).  `old` is always
 *                 the PARENT's seqChar, `new` the element's code as a character; element j's cell is
 *                 (b, pos, gap + j) when gap != -1, else (b, pos + j, -1).
 *                   NS (type 0), per element: nothing unless held(u, b); nothing when old is '-' or
 *                     'x'; otherwise an S entry.
 *                   NI (2): an I entry per element, no held test.
 *                   ND (1): a D entry per element with old as read (it may be '-'), no held test.
 *                   NSNPS (3): one S entry when held, also over an old '-' or 'x' (the reference
 *                     prints a notice); these are counted in `*odd_substitutions`.
 *                   NSNPI (4), NSNPD (5) and above: no entry at all (:3913, :3987), so single-base
 *                     insertions and deletions are missing from the reference's output and from this.
 * Text (:4025-4055), per node three lines, entries in list order within each, g present iff gap(cell):
 *   "Substitutions:\t<name>\t" { " > " [g] old coord+1 new } "\n"
 *   "Insertions:\t<name>\t"    { " > " [g] coord+1 new } "\n"
 *   "Deletions:\t<name>\t"     { " > " [g] coord+1 old } "\n"
 * Deviations: nodes are printed in node-id order (the reference iterates a
 * tbb::concurrent_unordered_map); the stdout notices ("INVERTED BLOCK FOUND", "INVERSION FOUND", "NOT
 * ACTUALLY A SUBSTITUTION") are not printed; a nucleotide mutation on a secondary block:
 * PM_ERR_UNSUPPORTED (as pm_maf / pm_aa); a node that ends its path with a block not held but flagged
 * reverse (an inversion of a block it does not hold): PM_ERR_UNSUPPORTED, found on the host before
 * any text is produced; a mutation (types 0 to 5) whose cell does not exist: PM_ERR_ARG, and on an id
 * that holds no block PM_ERR_UNSUPPORTED, both from the replay (the reference would default-insert
 * into its maps, or skip the id); rows of 2^31 - 64 columns and more: PM_ERR_UNSUPPORTED.
 * The rows of all nodes come from one replay of the derived PanMAT of pm_aa.  The root's coordinates
 * (a count over all columns), the expansion of the mutation lists into one entry per base, the
 * parent-row lookups, the line lengths and the text are computed on the GPU (profiling class 3),
 * batch by batch of nodes (PM_OPT_MUTATIONS_BATCH_BYTES), the text streamed through the pinned
 * download slots.  Phase log: mutations.*.  Memory: the replayed rows are nodes x columns bytes.
 * `*text` is malloc'd (release with pm_free); pm_print_mutations_fd writes to `fd` instead (`length`,
 * `odd_substitutions` nullable).  A failed write: PM_ERR_ARG (errno kept), as pm_fasta_fd. */
int pm_print_mutations(pm_ctx* ctx, const pm_panmat* panmat, char** text, int64_t* length, int64_t* odd_substitutions);
int pm_print_mutations_fd(pm_ctx* ctx, const pm_panmat* panmat, int fd, int64_t* length, int64_t* odd_substitutions);
/* Drop-in for panmanToUsher (src/panman2usher.cpp:564-604, the walk getNodeDFS at :282-562; the
 * --toUsher command, src/panmanUtils.cpp:1205-1240): the tree as an UShER mutation-annotated tree, a
 * Parsimony::data Protobuf message (usher.proto) of the Newick string and one mutation_list per node.
 * THE REFERENCE IS UNDEFINED AS WRITTEN: panmanToUsher indexes globalCoords_t and pseudoRoot while both
 * are still empty vectors (:565-569, used at :18 and :69).  What is restated here is what its code does
 * with both sized to the largest block id + 1.  Cells, positions 0..n_b, gap slots and nucleotide codes
 * are those of pm_print_mutations above.
 *   position      (getCoordMap, :3-51) the cells of a block are, per position 0..n_b, its gap slots
 *                 ascending and then its main character; position(cell) = 1 + the cells before it over
 *                 the blocks in ascending id (an id without a block has no cell).  That is the canonical
 *                 aligned column + 1.
 *   pseudo-root   (getPseudoRoot, :53-90) the consensus character at every main cell, '-' in every gap
 *                 slot, 'x' at the sentinel.
 *   the walk      (getNodeDFS) depth-first pre-order, children in stored order, the root included; every
 *                 node gives one mutation_list, possibly empty.  The running sequence starts as the
 *                 pseudo-root; a node's nucleotide mutations are applied to it in list order and undone
 *                 after its subtree.  Block mutations are tracked (:294-333) and never read: the output
 *                 does not depend on them, on which blocks a node holds or on strands, and nucleotide
 *                 mutations of every block apply at every node.
 *   entries       types 0 (NS), 1 (ND), 2 (NI) give info >> 4 elements, types 3, 4, 5 (NSNPS, NSNPI,
 *                 NSNPD) one, types 6 and 7 none.  Element j's cell is (b, pos, gap + j) when gap != -1,
 *                 else (b, pos + j, -1).  Per element, in order, one `mut`: position as above; ref_nuc =
 *                 code(pseudo-root[cell]) with code = getCodeFromNucleotide (0 for '-' and 'x'); par_nuc
 *                 = code of the RUNNING character at the cell (what an earlier element of the same list
 *                 left there if any, else the parent's; the pseudo-root's for the root); mut_nuc = the
 *                 ascending indices 0..3 of the set bits of c, c being the element's code for
 *                 substitutions and insertions (a code of 0 counts as 15: get_nuc(0) is 'N') and 15 for
 *                 both deletion types (newVal stays '-' there, :344, :432, :520, so deletions carry
 *                 mut_nuc = {0, 1, 2, 3}; kept).  The running character becomes the code's character,
 *                 '-' for a deletion.
 *   bytes         proto3 as the Protobuf C++ library writes it: fields in number order, zero scalars
 *                 left out, repeated int32 packed.  A mut is 08 varint(position) [10 ref] [18 par]
 *                 22 len b0.., wrapped as 0a len body (chromosome is never set); a node is 12 varint(L)
 *                 and its wrapped muts, L their bytes (an empty node: 12 00); the message is
 *                 0a varint(len(newick)) newick and then the nodes.  The newick is Tree::getNewickString
 *                 of the topology and branch lengths (defaults when `branch_length` is null), as the
 *                 PanMAN writer prints it.
 * `*mutations` (nullable) = the number of mut records.
 * Deviations: a nucleotide mutation on a secondary block: PM_ERR_UNSUPPORTED, as pm_maf / pm_aa /
 * pm_print_mutations (the reference would alias it onto the primary block); a mutation (types 0 to 5)
 * whose cell does not exist: PM_ERR_ARG (the reference indexes out of bounds), on an id that holds no
 * block or with a run longer than 6: PM_ERR_UNSUPPORTED, all from the replay; a duplicate primary block
 * id: PM_ERR_UNSUPPORTED (the reference would append the second block's cells to the first's); rows of
 * 2^31 - 64 columns and more, 2^31 - 64 nucleotide mutations and more, or a node whose list takes 2^31
 * bytes and more: PM_ERR_UNSUPPORTED; condensed_nodes and metadata are not written (nor by the
 * reference); no gzip.  Every refusal happens before the first byte reaches the sink or `fd`; only a
 * failed write or a device failure can leave a partial output there.
 * The rows of all nodes come from one replay of a derived PanMAT: that of pm_aa with the block mutations
 * replaced by one plain insertion of every block at the root, so row v is the reference's running
 * sequence after node v; the replay's consensus row is the pseudo-root.  The expansion of the lists into
 * one entry per base, the column, ref and par lookups, the earlier writers of a cell within a list (a
 * stable radix sort of (node, column) keys, each element reading its sorted predecessor), the sizes and
 * the bytes are computed on the GPU (profiling class 3), batch by batch of nodes in pre-order
 * (PM_OPT_USHER_BATCH_BYTES), the bytes streamed through the pinned download slots; the host writes the
 * newick field.  Phase log: usher.*.  Memory: the replayed rows are nodes x columns bytes.
 * `*bytes` is malloc'd (release with pm_free; `*length` bytes, NULs included, and one NUL after them);
 * pm_to_usher_fd writes to `fd` instead (`length`, `mutations` nullable).  A failed write: PM_ERR_ARG
 * (errno kept), as pm_fasta_fd. */
int pm_to_usher(pm_ctx* ctx, const pm_panmat* panmat, char** bytes, int64_t* length, int64_t* mutations);
int pm_to_usher_fd(pm_ctx* ctx, const pm_panmat* panmat, int fd, int64_t* length, int64_t* mutations);
/* Canonical aligned columns per leaf of the prepared PanMAT (gap slots before each main
 * position, block sentinels included) and the number of leaves. */
int pm_replay_shape(pm_ctx* ctx, int64_t* leaves, int64_t* columns, int64_t* edits);

/* ---- PanMAN files (xz + Cap'n Proto, schema panman.capnp) ----------------------------- */
typedef struct pm_panman pm_panman;
/* Load a .panman: TreeGroup(istream) + Tree::protoMATToTree (src/panman.cpp:6847-6877,
 * :1661-1751, mutations assigned in pre-order :576-618).  Host only, no device needed.
 * On failure `err` (nullable, err_len bytes) receives the reason. */
int pm_panman_load(const char* path, pm_panman** out, char* err, int64_t err_len);
/* The older Google Protobuf PanMAN (`panmanOld.treeGroup`, panman.proto; xz-compressed or
 * raw), as TreeGroup(istream, isOld = true) reads it (src/panman.cpp:6865-6876 with
 * Tree::protoMATToTree(panmanOld::tree), :1803-1866) -- into the same handle as
 * pm_panman_load, so pm_panman_write converts it (the reference's --protobuf2capnp,
 * src/panmanUtils.cpp:939-952). */
int pm_panman_load_old(const char* path, pm_panman** out, char* err, int64_t err_len);
int pm_panman_tree_count(const pm_panman* file);
/* View of tree `index` as a pm_panmat (pointers into `file`, valid until pm_panman_free);
 * node ids are pre-order positions of the stored Newick, names follow the reference's
 * Newick naming. */
int pm_panman_tree(const pm_panman* file, int index, pm_panmat* view);
const char* pm_panman_newick(const pm_panman* file, int index);
void pm_panman_free(pm_panman* file);
/* Write trees as TreeGroup::writeToFile + writePanMAN do (src/panman.cpp:6885-7015,
 * src/panmanUtils.cpp:271-299): capnp message, xz level 9 when `compress`. */
int pm_panman_write(const char* path, const pm_panmat* const* trees, int count, int compress);

/* Drop-in for Tree::reroot(leaf) (src/reroot.cpp:4-262; CLI --reroot,
 * src/panmanUtils.cpp:855-892): every leaf's sequence is replayed on the GPU
 * (getSequenceFromReference, src/panman.cpp:4676-5000), the root moves next to `leaf`
 * (transform, :5831-5906) and every block and nucleotide mutation is re-derived by Fitch
 * with the root forced to the leaf's states.  The result is a new one-tree pm_panman (in
 * the pre-order of the new topology; release with pm_panman_free).  Replaces the ctx's
 * tree, columns and replay state.  Within a node, block mutations are ordered by block
 * id (the reference's order is TBB-scheduled).  A PanMAT with secondary blocks (a nucleotide
 * mutation with secondaryBlockId != -1) returns PM_ERR_UNSUPPORTED ("secondary blocks"):
 * the reference rebuilds the secondary blocks' own sequences and block states
 * (src/reroot.cpp:55-89, src/panman.cpp:4722-4890), a second block level this layout does
 * not hold -- although pm_fasta, like printFASTAUltraFastHelper, replays such a PanMAT (the
 * mutation lands on the primary block).  A branch length that moves to another node (the
 * leaf's, and that of every node between it and the old root) loses its fraction, as
 * transform's `size_t oldBranchLen` makes it (:5855, :5888); a negative one is kept.  An old
 * root left without a child (a unary root above the leaf's chain) returns
 * PM_ERR_UNSUPPORTED: the reference reads children[0] of an empty list there (:5837).  The
 * nucleotide Fitch runs in column chunks (PM_OPT_REROOT_CHUNK_SITES). */
int pm_reroot(pm_ctx* ctx, const pm_panmat* tree, const char* leaf, pm_panman** out);

/* Drop-in for Tree::subtreeExtractParallel(ids, {}) (src/subnet.cpp:3-135; the --subnet command,
 * src/panmanUtils.cpp:584-652, through TreeGroup::subnetworkExtract, src/subnet.cpp:138-206): the tree cut down
 * to the nodes named in `ids` (tips or internal nodes; duplicates do no harm).  Those nodes and all their
 * ancestors are kept, with their child order; then every kept node with exactly one kept child is merged with
 * it (compressTreeParallel, mergeNodes, src/panman.cpp:2033-2055), the root included: the merged node has the
 * child's name and children, the sum of the branch lengths, consolidateNucMutations (src/panman.cpp:2233-2322)
 * of the parent's list followed by the child's -- per coordinate the left fold of replaceMutation (:2058-2085),
 * an insertion followed by a deletion removing the coordinate; the survivors sorted by (primary block,
 * position, gap position) and regrouped into runs of at most 6 -- and consolidateBlockMutations (:2324-2372) of
 * the two block lists, here in ascending block id (the reference's order is its hash map's).  A node that
 * merges with nothing keeps its lists as they are.  A one-tip request gives a one-node tree.
 * The result is a new one-tree pm_panman (in the pre-order of the new topology; release with pm_panman_free).
 * Blocks and gaps are copied; a surviving node keeps the circular_offset, rotation_index and sequence_inverted
 * of its surviving name (the reference also keeps those entries for dropped names: pm_panmat holds them per
 * node, so they cannot be kept, and nothing reads them); branch_length NULL gives a result without lengths.
 * Complex mutations are neither read nor written here, so nodeIdsToDefinitelyInclude is always empty.
 * The merged chains' nucleotide mutations are consolidated on the GPU (profiling class 3) in batches
 * (PM_OPT_SUBNET_BATCH_ENTRIES); a request that merges nothing launches nothing.  Phase log: subnet.*.
 * Errors: num_ids == 0: PM_ERR_ARG; an unknown identifier: PM_ERR_ARG "Some of the specified node identifiers
 * don't exist!!!"; on a merged chain, a nucleotide mutation with secondaryBlockId != -1: PM_ERR_UNSUPPORTED
 * ("secondary blocks", as pm_reroot; on a node that merges with nothing it is copied), one outside its block or
 * gap slots: PM_ERR_ARG, a block sequence the reference throws on (insertion after insertion, deletion or
 * inversion after deletion, insertion after inversion): PM_ERR_ARG with the reference's message; blocks and gap
 * slots of 2^32 coordinates or more in all: PM_ERR_UNSUPPORTED. */
int pm_subnet(pm_ctx* ctx, const pm_panmat* tree, const char* const* ids, int64_t num_ids, pm_panman** out);

/* Tree::imputeNs(allowedIndelDistance) (src/impute.cpp:4-79; the --impute command, src/panmanUtils.cpp:328-354) up to
 * and including the plan of moves.  THE PLAN IS NOT APPLIED: the moves (src/impute.cpp:46-70, moveNode :339-358) have
 * no defined behaviour to match -- moveNode falls off the end of a bool function, its dummy parent copies block
 * mutations the new parent keeps, newInternalNodeId() restarts at node_1 on a loaded file, and the moves run in the
 * hash order of an unordered_map of strings -- so the tree that comes back has the input's topology.
 *   `*out`   a one-tree pm_panman (release with pm_panman_free) equal to `tree` in topology, names, blocks, gaps,
 *            per-node options and branch lengths; the nucleotide lists are the substitution-imputed ones.
 *   `*plan`  malloc'd text (release with pm_free; `*plan_length` bytes and one NUL): one block per node whose
 *            insertions hold an N (an attempt), in node-id order.  Head line
 *              name \t runs-with-N \t candidates \t new-parent-name \t nucImprovement \t blockImprovement
 *            (without a winner the last three fields are ". -1 0"); under a winner its bestNewMuts, the block
 *            mutations as "name \t B \t block \t insertion \t inversion" in ascending block id (the reference's
 *            order is its hash map's), then the NucMuts as "name \t N \t block \t position \t gap \t info \t
 *            nucs as %06x", `name` being the node to move.
 *   `*stats` (nullable) the counts the command prints.
 * Substitution pass (:142-184, :205-225), every node but the root (the root's list is never visited, :98, its Ns
 *   stay): an NS or NSNPS record with an N among its first length() codes is erased; an NS's other bases come back
 *   in its place as single NSNPS records (NucMut(other, i), src/panman.hpp:233-248) at position + i when the gap
 *   position is -1, else at gap position + i; the count is length() minus the bases put back.  Ns inside insertion
 *   and deletion records stay.  (std::find erasing "the first equal record" gives the same lists as erasing each
 *   such record in place; nothing is searched.)
 * State.  originalNucs[v][cell] is the code of the character at `cell` just before v's list is applied (:161),
 *   anything that is no nucleotide letter being 0: the consensus, the root's nucleotide mutations on the blocks the
 *   root holds after its own block mutations (getSequenceFromReference, src/panman.cpp:4820-4835), and below the
 *   root every nucleotide mutation of the path whether or not its block is held (:151-163 never looks).  One replay
 *   of a derived PanMAT gives these rows; they are read at the parent.
 * Insertion census (:147-183), from the lists as given: runs of insertion records merged by
 *   IndelPosition::mergeIndels (src/panman.hpp:408-421) with its quirks -- only the last run is a merge target,
 *   records of other types in between do not end a run, a run headed at gap -1 merges a record whose nucPosition
 *   continues it whatever that record's gap position, a run headed in a gap slot compares gap positions without
 *   comparing nucPosition -- each with its N count; two runs of one node with equal IndelPosition collapse to the
 *   first.
 * Candidates (findNearbyInsertions, :288-337): from node->parent, at every node first the node, then its children in
 *   order (but where the walk came from), then its parent; every step passes allowedDistance - branchLength computed
 *   in float and truncated toward zero to an int (0 - 0.5 is 0: the walk goes on) and stops only below 0;
 *   `branch_length` NULL: all 0, the whole tree.  A node is a candidate when the first of the moving node's N-bearing
 *   runs that it also holds is not all N there (:300-308).  That "first" is in the moving node's list order here and
 *   in hash order in the reference; it matters only where a candidate holds two of them, one of them all N.
 * Score (:264-283): the lists from candidate to node -- a node the path leaves upward gives its list inverted
 *   (MutationList::invertMutations, src/panman.cpp:2374-2420: insertions become deletions of code 0, deletions
 *   insertions of the originals, substitutions go back to the originals; block insertions become deletions and block
 *   deletions insertions, whose strand stays false: convertToInsertion assigns its parameter to itself, so the
 *   wasBlockInv state it is handed is never stored), a node it enters downward its list as it is, the node's own list
 *   last, all substitution-imputed -- through consolidateNucMutations, the substitution pass again and
 *   consolidateBlockMutations.  nucImprovement = the sum of length() over the node's list minus that over the new
 *   list, blockImprovement = the difference of the block list sizes; a candidate wins with nucImprovement > best and
 *   blockImprovement >= best, from (-1, 0), both ratcheting: among equals the first in walk order.
 * The substitution pass, the test for a cell written twice, the originals, every pair's path lists, their fold and
 * length, and the winners' regrouped and imputed lists are computed on the GPU (profiling class 3), pairs in batches
 * (PM_OPT_IMPUTE_BATCH_ENTRIES); the census, the walk, the block tables (fillBlockLookupTables, :186-203, with the
 * strand undo of :130-139 that never applied the inversion on the way down) and the block folds run on the host.  A
 * tree without an N in any substitution or insertion below the root launches nothing after the replay.  Phase log:
 * impute.*.  Replaces the ctx's replay state.  Memory: the replayed rows are nodes x columns bytes.
 * Errors: a list that writes one cell twice: PM_ERR_UNSUPPORTED "a cell written twice in one list" (the reference's
 * undo, :122-128, would restore the wrong character and corrupt every later sibling); a nucleotide mutation with
 * secondaryBlockId != -1: PM_ERR_UNSUPPORTED "secondary blocks"; a deletion record that carries codes:
 * PM_ERR_UNSUPPORTED (the walk would write them as characters, the rows hold '-'); a cell outside its block or gap
 * slots, a length nibble above 6, a type above 5, an NSNP* record whose length is not 1: PM_ERR_ARG; a block sequence
 * on which consolidateBlockMutations throws: PM_ERR_ARG with the reference's message. */
typedef struct pm_impute_stats {
    int64_t imputed_bases;     /* "Imputed k/k SNPs/MNPs to N": the sum of imputeSubstitution's returns          */
    int64_t insertion_nodes;   /* nodes, the root excepted, with an insertion run holding an N (the attempts)    */
    int64_t moves_found;       /* of those, the ones findInsertionImputationMove gives a new parent              */
    int64_t pairs;             /* (node, candidate) pairs scored                                                 */
} pm_impute_stats;
int pm_impute(pm_ctx* ctx, const pm_panmat* tree, int32_t max_distance, pm_panman** out, char** plan, int64_t* plan_length,
              pm_impute_stats* stats);

/* Drop-in for Tree(pangraph.json, newick, FILE_TYPE::PANGRAPH, reference) (src/panman.cpp:
 * 820-1273; CLI -P/-N, src/panmanUtils.cpp:1364-1407): the PanGraph model
 * (src/panman.cpp:6200-6476), block order by chained alignment of the paths
 * (src/chaining.cpp) and rotation of circular paths (src/rotation.cpp) on the host; block
 * and nucleotide parsimony for every column on the GPU (Fitch, or Sankoff when the tree
 * has a polytomy).  `json` and `newick` are file contents; `reference` may be NULL / "".
 * Without a reference the main-column root forcing follows oneTBB's iteration order of
 * the per-block sequences.  Result: a one-tree pm_panman. */
int pm_pangraph_build(pm_ctx* ctx, const char* json, const char* newick, const char* reference, pm_panman** out);

/* Drop-in for Tree(gfa, newick, FILE_TYPE::GFA) (src/panman.cpp:728-819; CLI -G/-N,
 * src/panmanUtils.cpp:1326-1362) followed by TreeGroup({T}): `gfa_text` and `newick` are file
 * contents (the Newick is the first line of its text).  Result: a one-tree pm_panman.
 *   parse    line by line, fields split on tab as stringSplit does (src/panman.cpp:265-300).
 *            "S": nodes[f[1]] = f[2]; "P": the steps of f[2] split on ',', a step's name all but
 *            its last character, forward when that is '+'; a later duplicate of either wins; every
 *            other record type and blank lines are ignored.  Paths are taken in byte order of
 *            their names (std::map).
 *   blocks   GfaGraph::GfaGraph (:6060-6142): the first path seeds the consensus order, each later
 *            path is chain_align'ed against it (src/chaining.cpp), its unmatched steps become new
 *            blocks -- a repeated or moved segment is a second block with the same sequence.
 *            Block i has primary id i and Block(i, sequence) of its segment (:777-779); there are
 *            no gaps, no block gaps and no nucleotide mutations.
 *   states   per path the two-pointer walk against blocks 0..T-1 (:6144-6193): absent where the
 *            path lacks the block, else forward / reverse by the step's strand (:784-797).
 *   Fitch    PM_MODE_BLOCK_FITCH over every block (:798-800), also on a tree with polytomies
 *            (where the PanGraph driver switches to Sankoff); the root's parent state is absent
 *            and nothing is forced.  A tree leaf no path names is absent from every column; a
 *            path no leaf names takes part in the block order only.  The states reach the device
 *            as sparse rows (pm_leaves_upload_sparse: the steps, fill = absent) in batches of
 *            PM_OPT_GFA_IN_BATCH_SITES columns.
 *   Within a node the block mutations are in ascending block id (the reference's order is
 *   TBB-scheduled), (type, inversion) as src/fitchSankoff.cpp:279-303.
 * Errors (PM_ERR_ARG, the message names the offender): a step naming an undefined segment (the
 * reference makes an empty block), an empty step, an "S" or "P" line of fewer than 3 fields, no
 * "P" line, a Newick that does not parse.  Phase log: gfain.parse, gfain.chain, gfain.upload,
 * gfain.run, gfain.assemble.  Replaces the ctx's tree and columns. */
int pm_gfa_build(pm_ctx* ctx, const char* gfa_text, const char* newick, pm_panman** out);

/* ---- summary ------------------------------------------------------------------------- */
/* Drop-in for Tree::printSummary (src/summary.cpp:257-273; CLI --summary, src/panmanUtils.cpp:
 * 356-384): mutation counts reduced on the GPU from the PanMAT's flat mutation arrays
 * (getTotalParsimonyParallel, :3-59; getBlockMutationsParallelHelper, :61-109), leaf depths
 * as the Newick parser computes them (float sum in leaf order, src/panman.cpp:386-394),
 * block duplications / translocations by the reference's presence walk (:111-193). */
typedef struct pm_summary {
    int64_t nodes, samples;                                 /* Total Nodes / Samples in Tree */
    int64_t substitutions, insertions, deletions, inversions;
    int64_t max_depth;
    float mean_depth;
    int64_t block_insertions, block_deletions, block_inversions;
    int64_t block_duplications, block_translocations;
} pm_summary;
int pm_summary_compute(pm_ctx* ctx, const pm_panmat* tree, pm_summary* out);

/* ---- synthetic inputs (bench / tests; seeded, counter-based) ------------------------ */
/* Random-join binary tree on `leaves` leaves (SURVEY.md §8d family T1): writes
 * 2*leaves-1 nodes as CSR; leaves are ids [0, leaves), internal nodes follow. */
int pm_synth_tree_random_join(int64_t leaves, uint64_t seed, int32_t* child_offsets,
                              int32_t* child_index, int32_t* root);
/* "SARS-like" tree (SURVEY.md §8d family T2): ladderised sequential insertion (leaf i
 * splits the pendant edge of leaf i-1 with p = 0.9, else of a uniform earlier leaf), then
 * 10 % of the internal nodes contracted into polytomies of 3-64 children.  Buffers must
 * hold 2*leaves-1 nodes (child_offsets 2*leaves entries, child_index 2*leaves-2); the
 * node count written is returned in *num_nodes; leaves are ids [0, leaves). */
int pm_synth_tree_sars_like(int64_t leaves, uint64_t seed, int32_t* child_offsets, int32_t* child_index,
                            int32_t* root, int64_t* num_nodes);
/* Evolve columns [site_begin, site_begin + num_sites) of a seeded alignment down the
 * uploaded tree on the device and install them as the leaf columns plus the consensus
 * (the root sequence).  Identical global sites give identical columns on every rank. */
int pm_synth_columns(pm_ctx* ctx, int64_t site_begin, int64_t num_sites, uint64_t seed);
/* Copy leaf codes of sites [s0, s0+ns) to host, one byte per site:
 * out[leaf * ns + (s - s0)] for every leaf in increasing node-id order (absent = 0). */
int pm_leaf_codes_fetch(pm_ctx* ctx, int64_t s0, int64_t ns, uint8_t* out);
int pm_consensus_fetch(pm_ctx* ctx, int64_t s0, int64_t ns, uint8_t* out);

#ifdef __cplusplus
}
#endif

#endif /* PANMAN_GPU_H */
