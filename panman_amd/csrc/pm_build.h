// pm_build.h -- the host-only half of what the drivers that produce a PanMAT share (pm_msa,
// pm_pangraph, pm_gfa_in, pm_reroot, pm_subnet; the loader takes the tree arrays): the nucleotide
// code table and its packings, a Topology's arrays in a PanmanTree, the NucMut run rule and the
// block-mutation records.  No HIP header: plain g++ compiles it (tests/build_host_check.cpp).  The
// device-touching half is in pm_dev.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "pm_newick.h"
#include "pm_panman_tree.h"

namespace pm {

// ---- codes ------------------------------------------------------------------------------------

// src/panman.cpp:78-113; a gap, lower case, the replay's 'x' sentinel and anything else: 0.
inline uint8_t code_of(char ch) {
    switch (ch) {
        case 'A': return 1;  case 'C': return 2;  case 'G': return 4;  case 'T': return 8;
        case 'R': return 5;  case 'Y': return 10; case 'S': return 6;  case 'W': return 9;
        case 'K': return 12; case 'M': return 3;  case 'B': return 14; case 'D': return 13;
        case 'H': return 11; case 'V': return 7;  case 'N': return 15;
        default: return 0;
    }
}

// Block(i, seq): 8 codes per word, the first in the top nibble (src/panman.cpp:246-257).
inline std::vector<uint32_t> encode_block(const std::string& seq) {
    std::vector<uint32_t> w;
    for (size_t i = 0; i < seq.size(); i += 8) {
        uint32_t x = 0;
        for (size_t j = i; j < std::min(i + 8, seq.size()); ++j) x ^= (uint32_t)code_of(seq[j]) << (4 * (7 - (j - i)));
        w.push_back(x);
    }
    return w;
}

// The columns' packing: code(s) of n sites two to a byte, the even site in the low nibble, into
// the (n + 1) / 2 bytes at `out` (a last odd site leaves its high nibble 0).
template <class Code>
void pack4_into(uint8_t* out, size_t n, Code code) {
    for (size_t s = 0; s + 1 < n; s += 2) out[s / 2] = (uint8_t)(code(s) | code(s + 1) << 4);
    if (n & 1) out[n / 2] = (uint8_t)code(n - 1);
}

inline std::vector<uint8_t> pack4(const std::vector<uint8_t>& codes) {
    std::vector<uint8_t> out((codes.size() + 1) / 2);
    const uint8_t* in = codes.data();
    pack4_into(out.data(), codes.size(), [in](size_t s) { return in[s]; });
    return out;
}

// ---- topology ---------------------------------------------------------------------------------

// The first line of `text` as a topology.
inline bool parse_newick(const char* text, Topology& t, std::string& err) {
    std::string line(text);
    const size_t nl = line.find('\n');
    if (nl != std::string::npos) line.resize(nl);
    return parse_topology(line, t, err);
}

// A topology's arrays: the CSR child lists, the NUL-separated names, the branch lengths.
inline void set_topology(const Topology& t, PanmanTree& out) {
    const int32_t N = (int32_t)t.name.size();
    out.num_nodes = N;
    out.root = t.root;
    out.length = t.length;
    out.child_off.assign(N + 1, 0);
    out.child_idx.clear();
    out.child_idx.reserve(N);
    size_t bytes = 0;
    for (const std::string& name : t.name) bytes += name.size() + 1;
    out.names_blob.clear();
    out.names_blob.reserve(bytes);
    for (int32_t v = 0; v < N; ++v) {
        out.child_idx.insert(out.child_idx.end(), t.kids[v].begin(), t.kids[v].end());
        out.child_off[v + 1] = (int32_t)out.child_idx.size();
        out.names_blob += t.name[v];
        out.names_blob.push_back('\0');
    }
}

// A new tree over `t`: its arrays, no sequence circular, rotated or inverted, and the mutation
// lists open at node 0 (append_block_muts / append_nuc_muts close them node by node).  With
// `newick` the tree's text too, which a handle hands out (pm_panman_newick); a tree that is only
// written does without it, the writer prints its own.
inline void tree_from_topology(const Topology& t, PanmanTree& out, bool newick = true) {
    set_topology(t, out);
    out.newick = newick ? newick_of(t) : std::string();
    out.circular.assign(out.num_nodes, -1);
    out.rotation.assign(out.num_nodes, 0);
    out.inverted.assign(out.num_nodes, 0);
    out.bm_off.assign(out.num_nodes + 1, 0);
    out.nm_off.assign(out.num_nodes + 1, 0);
}

// What pm_tree_upload reads of a tree.
inline pm_tree tree_view(const PanmanTree& t) { return pm_tree{t.num_nodes, t.root, t.child_off.data(), t.child_idx.data()}; }

// The blocks and gap lists of `p`, which a rerooted tree or a subnetwork keeps as they are.
inline void copy_blocks(const pm_panmat& p, PanmanTree& out) {
    out.block_primary.assign(p.block_primary, p.block_primary + p.num_blocks);
    out.block_seq_off.assign(p.block_seq_offsets, p.block_seq_offsets + p.num_blocks + 1);
    out.block_seq.assign(p.block_seq, p.block_seq + p.block_seq_offsets[p.num_blocks]);
    out.gap_primary.assign(p.gap_primary, p.gap_primary + p.num_gaps);
    out.gap_off.assign(p.gap_offsets, p.gap_offsets + p.num_gaps + 1);
    out.gap_pos.assign(p.gap_position, p.gap_position + p.gap_offsets[p.num_gaps]);
    out.gap_len.assign(p.gap_length, p.gap_length + p.gap_offsets[p.num_gaps]);
}

// ---- mutation lists ---------------------------------------------------------------------------

// One block-parsimony record of a node: (block, type << 4 | code) as PM_MODE_BLOCK_* reports it.
using BlockRec = std::pair<int32_t, uint8_t>;

// Node v's block mutations, in the order given (src/fitchSankoff.cpp:279-303): NI -> BlockMut(BI,
// inversion = code == 2), ND -> BlockMut(BD, false), NS -> BlockMut(BD, inversion = true).
inline void append_block_muts(PanmanTree& out, int32_t v, const std::vector<BlockRec>& recs) {
    for (const BlockRec& bm : recs) {
        const int type = bm.second >> 4, code = bm.second & 15;
        out.bm_primary.push_back(bm.first);
        out.bm_info.push_back(type == PM_MUT_NI ? 1 : 0);
        out.bm_inv.push_back(type == PM_MUT_NI ? code == 2 : type == PM_MUT_NS);
    }
    out.bm_off[v + 1] = (int64_t)out.bm_primary.size();
}

struct Tup {   // one nucleotide record of a node; gap = -1: a main position
    int32_t block, pos, gap;
    uint8_t type, code;
};

// NucMut runs (src/panman.cpp:1236-1272, :1445-1466, src/reroot.cpp:228-262): at most 6 codes, one
// block, one type, consecutive positions (main) or consecutive slots of one position (gap).  The
// tuples are taken in the order given; `gap` says which of the two kinds they all are.
inline void group(const std::vector<Tup>& v, bool gap, PanmanTree& out) {
    size_t start = 0;
    auto emit = [&](size_t a, size_t b) {
        uint32_t nucs = 0;
        for (size_t i = a; i < b; ++i) nucs |= (uint32_t)v[i].code << (4 * (5 - (i - a)));
        out.nm_primary.push_back(v[a].block);
        out.nm_secondary.push_back(-1);
        out.nm_pos.push_back(v[a].pos);
        out.nm_gap.push_back(gap ? v[a].gap : -1);
        out.nm_info.push_back((uint8_t)(((b - a) << 4) + v[a].type));
        out.nm_nucs.push_back(nucs);
    };
    for (size_t i = 1; i < v.size(); ++i) {
        const Tup& p = v[i - 1];
        const Tup& q = v[i];
        const bool brk = i - start == 6 || q.block != p.block || q.type != p.type ||
                         (gap ? (q.pos != p.pos || q.gap != p.gap + 1) : q.pos != p.pos + 1);
        if (brk) {
            emit(start, i);
            start = i;
        }
    }
    if (!v.empty()) emit(start, v.size());
}

// Node v's nucleotide mutations: the main runs first, then the gap runs (nonGapMutations, then
// gapMutations).
inline void append_nuc_muts(PanmanTree& out, int32_t v, const std::vector<Tup>& main_t, const std::vector<Tup>& gap_t) {
    group(main_t, false, out);
    group(gap_t, true, out);
    out.nm_off[v + 1] = (int64_t)out.nm_primary.size();
}

}  // namespace pm
