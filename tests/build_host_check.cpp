// The host-only half of the construction drivers (panman_amd/csrc/pm_build.h) under
// AddressSanitizer, the leak checker and UBSan: the code table and its packings, a topology's
// arrays, the NucMut run rule and the block-mutation records.  Every expected value is written out
// by hand from the rules.  Stand-alone; built and run by tests/test_build_host.py.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../panman_amd/csrc/pm_build.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

using pm::PanmanTree;
using pm::Tup;
using U8 = std::vector<uint8_t>;
using U32 = std::vector<uint32_t>;
using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;

// ---- codes --------------------------------------------------------------------------------------

void code_table() {
    const char letters[] = "ACGTRYSWKMBDHVN";
    const uint8_t codes[] = {1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    for (int i = 0; i < 15; ++i) CHECK(pm::code_of(letters[i]) == codes[i]);
    for (const char ch : {'-', 'x', 'a', 'c', 'g', 't', 'n', ' ', '\0', '*', 'U', 'Z'}) CHECK(pm::code_of(ch) == 0);
    CHECK(pm::code_of((char)0xC1) == 0);   // a negative char
}

void pack4_cases() {
    CHECK(pm::pack4({}) == U8{});
    CHECK(pm::pack4({1}) == U8{0x01});
    CHECK((pm::pack4({1, 2, 4}) == U8{0x21, 0x04}));
    CHECK((pm::pack4({15, 15, 0, 8}) == U8{0xFF, 0x80}));
    uint8_t row[3] = {0xAA, 0xAA, 0xEE};   // pack4_into sets (n + 1) / 2 bytes whatever they held, and no more
    const std::string text = "ACG";
    pm::pack4_into(row, text.size(), [&](size_t s) { return pm::code_of(text[s]); });
    CHECK(row[0] == 0x21 && row[1] == 0x04 && row[2] == 0xEE);
    pm::pack4_into(row + 2, 0, [&](size_t) { return (uint8_t)15; });
    CHECK(row[2] == 0xEE);
}

void encode_block_cases() {
    CHECK(pm::encode_block("").empty());
    CHECK(pm::encode_block("A") == U32{0x10000000u});
    CHECK(pm::encode_block("ACGTACGT") == U32{0x12481248u});
    CHECK((pm::encode_block("ACGTACGTA") == U32{0x12481248u, 0x10000000u}));
    CHECK(pm::encode_block("NNNNNNNN") == U32{0xFFFFFFFFu});
    CHECK(pm::encode_block("Aa-cT") == U32{0x10008000u});   // lower case and '-': code 0
    CHECK(pm::encode_block("acgt-") == U32{0u});
}

// ---- NucMut runs --------------------------------------------------------------------------------

struct Run {
    int32_t primary, pos, gap;
    uint8_t info;
    uint32_t nucs;
};

void expect_runs(const PanmanTree& t, const std::vector<Run>& want, int line) {
    const size_t n = want.size();
    bool ok = t.nm_primary.size() == n && t.nm_secondary.size() == n && t.nm_pos.size() == n && t.nm_gap.size() == n &&
              t.nm_info.size() == n && t.nm_nucs.size() == n;
    for (size_t k = 0; ok && k < n; ++k)
        ok = t.nm_primary[k] == want[k].primary && t.nm_secondary[k] == -1 && t.nm_pos[k] == want[k].pos &&
             t.nm_gap[k] == want[k].gap && t.nm_info[k] == want[k].info && t.nm_nucs[k] == want[k].nucs;
    if (!ok) {
        std::fprintf(stderr, "%s:%d: NucMut runs differ (%zu records, %zu expected)\n", __FILE__, line, t.nm_primary.size(), n);
        ++failures;
    }
}

std::vector<Run> grouped(const std::vector<Tup>& v, bool gap) {
    PanmanTree t;
    pm::group(v, gap, t);
    std::vector<Run> out;
    for (size_t k = 0; k < t.nm_primary.size(); ++k)
        out.push_back(Run{t.nm_primary[k], t.nm_pos[k], t.nm_gap[k], t.nm_info[k], t.nm_nucs[k]});
    expect_runs(t, out, __LINE__);   // the six arrays grow together, nm_secondary is -1 throughout
    return out;
}

bool same(const std::vector<Run>& a, const std::vector<Run>& b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); ++k)
        if (a[k].primary != b[k].primary || a[k].pos != b[k].pos || a[k].gap != b[k].gap || a[k].info != b[k].info ||
            a[k].nucs != b[k].nucs)
            return false;
    return true;
}

void group_main() {
    CHECK(grouped({}, false).empty());
    // seven consecutive positions, one block, type 2: a run of six and a run of one
    const uint8_t seven[7] = {1, 2, 4, 8, 1, 2, 4};
    std::vector<Tup> v;
    for (int i = 0; i < 7; ++i) v.push_back(Tup{3, 10 + i, -1, 2, seven[i]});
    CHECK(same(grouped(v, false), {{3, 10, -1, 0x62, 0x124812u}, {3, 16, -1, 0x12, 0x400000u}}));
    // exactly six stay together
    v.pop_back();
    CHECK(same(grouped(v, false), {{3, 10, -1, 0x62, 0x124812u}}));
    // a single tuple
    CHECK(same(grouped({Tup{0, 5, -1, 0, 15}}, false), {{0, 5, -1, 0x10, 0xF00000u}}));
    // a position gap
    CHECK(same(grouped({Tup{0, 10, -1, 0, 1}, Tup{0, 12, -1, 0, 2}}, false), {{0, 10, -1, 0x10, 0x100000u}, {0, 12, -1, 0x10, 0x200000u}}));
    // a type change at consecutive positions
    CHECK(same(grouped({Tup{0, 10, -1, 0, 1}, Tup{0, 11, -1, 1, 2}}, false), {{0, 10, -1, 0x10, 0x100000u}, {0, 11, -1, 0x11, 0x200000u}}));
    // a block change at consecutive positions
    CHECK(same(grouped({Tup{0, 10, -1, 0, 1}, Tup{1, 11, -1, 0, 2}}, false), {{0, 10, -1, 0x10, 0x100000u}, {1, 11, -1, 0x10, 0x200000u}}));
    // consecutive, same block and type: one run of two
    CHECK(same(grouped({Tup{0, 10, -1, 0, 1}, Tup{0, 11, -1, 0, 2}}, false), {{0, 10, -1, 0x20, 0x120000u}}));
    // the order given is kept: descending positions never join
    CHECK(same(grouped({Tup{0, 11, -1, 0, 1}, Tup{0, 10, -1, 0, 2}}, false), {{0, 11, -1, 0x10, 0x100000u}, {0, 10, -1, 0x10, 0x200000u}}));
    // a main record's nm_gap is -1 whatever the tuple carries
    CHECK(same(grouped({Tup{0, 10, 7, 0, 1}}, false), {{0, 10, -1, 0x10, 0x100000u}}));
}

void group_gap() {
    CHECK(grouped({}, true).empty());
    // slots 0, 1, 2 of one position
    CHECK(same(grouped({Tup{2, 5, 0, 2, 1}, Tup{2, 5, 1, 2, 2}, Tup{2, 5, 2, 2, 4}}, true), {{2, 5, 0, 0x32, 0x124000u}}));
    // slot 0 of position 5, then slot 1 of position 6
    CHECK(same(grouped({Tup{2, 5, 0, 2, 1}, Tup{2, 6, 1, 2, 2}}, true), {{2, 5, 0, 0x12, 0x100000u}, {2, 6, 1, 0x12, 0x200000u}}));
    // slots 0 and 2 of one position
    CHECK(same(grouped({Tup{2, 5, 0, 2, 1}, Tup{2, 5, 2, 2, 2}}, true), {{2, 5, 0, 0x12, 0x100000u}, {2, 5, 2, 0x12, 0x200000u}}));
    // seven consecutive slots from slot 3: six and one
    const uint8_t seven[7] = {8, 4, 2, 1, 8, 4, 2};
    std::vector<Tup> v;
    for (int i = 0; i < 7; ++i) v.push_back(Tup{2, 5, 3 + i, 1, seven[i]});
    CHECK(same(grouped(v, true), {{2, 5, 3, 0x61, 0x842184u}, {2, 5, 9, 0x11, 0x200000u}}));
    // a type or a block change inside consecutive slots
    CHECK(same(grouped({Tup{2, 5, 0, 2, 1}, Tup{2, 5, 1, 0, 2}}, true), {{2, 5, 0, 0x12, 0x100000u}, {2, 5, 1, 0x10, 0x200000u}}));
    CHECK(same(grouped({Tup{2, 5, 0, 2, 1}, Tup{3, 5, 1, 2, 2}}, true), {{2, 5, 0, 0x12, 0x100000u}, {3, 5, 1, 0x12, 0x200000u}}));
}

void nuc_append() {   // main runs first, then gap runs, nm_off closed per node, an empty node too
    PanmanTree t;
    t.nm_off.assign(4, 0);
    pm::append_nuc_muts(t, 0, {Tup{0, 1, -1, 0, 1}, Tup{0, 2, -1, 0, 2}}, {Tup{0, 1, 0, 2, 8}});
    pm::append_nuc_muts(t, 1, {}, {});
    pm::append_nuc_muts(t, 2, {}, {Tup{1, 0, 4, 2, 4}});
    CHECK((t.nm_off == I64{0, 2, 2, 3}));
    expect_runs(t, {{0, 1, -1, 0x20, 0x120000u}, {0, 1, 0, 0x12, 0x800000u}, {1, 0, 4, 0x12, 0x400000u}}, __LINE__);
}

// ---- topology -----------------------------------------------------------------------------------

void expect_defaults(const PanmanTree& t, int32_t n) {
    CHECK(t.num_nodes == n);
    CHECK(t.circular == I32(n, -1));
    CHECK(t.rotation == I32(n, 0));
    CHECK(t.inverted == U8(n, 0));
    CHECK(t.bm_off == I64(n + 1, 0));
    CHECK(t.nm_off == I64(n + 1, 0));
}

void topology_cases() {
    {   // one node (the parser never yields one; a subnetwork of the root alone does)
        pm::Topology topo;
        topo.name = {"x"};
        topo.kids = {{}};
        topo.root = 0;
        PanmanTree t;
        pm::tree_from_topology(topo, t);
        CHECK(t.root == 0 && t.child_off == (I32{0, 0}) && t.child_idx.empty());
        CHECK(t.names_blob == std::string("x\0", 2));
        CHECK(t.length.empty());
        CHECK(t.newick == "x" && t.newick == pm::newick_of(topo));
        expect_defaults(t, 1);
        const pm_tree view = pm::tree_view(t);
        CHECK(view.num_nodes == 1 && view.root == 0 && view.child_offsets == t.child_off.data() && view.child_index == t.child_idx.data());
    }
    {   // a polytomy
        pm::Topology topo;
        std::string err;
        CHECK(pm::parse_newick("(a,b,c);", topo, err));
        PanmanTree t;
        pm::tree_from_topology(topo, t);
        CHECK(t.root == 0 && (t.child_off == I32{0, 3, 3, 3, 3}) && (t.child_idx == I32{1, 2, 3}));
        CHECK(t.names_blob == std::string("node_1\0a\0b\0c\0", 13));
        CHECK((t.length == std::vector<float>{0.0f, 1.0f, 1.0f, 1.0f}));
        CHECK(t.newick == "(a:1.000000,b:1.000000,c:1.000000)node_1:0.000000;" && t.newick == pm::newick_of(topo));
        expect_defaults(t, 4);
        pm::tree_from_topology(topo, t, false);   // a tree that is only written: everything but the text
        CHECK(t.newick.empty() && (t.child_idx == I32{1, 2, 3}) && t.names_blob.size() == 13);
        expect_defaults(t, 4);
    }
    {   // ((a,b),c); and a second line, which is cut off; a tree filled twice holds the second only
        pm::Topology topo;
        std::string err;
        CHECK(pm::parse_newick("((a:2,b:3):4,c:5);\n(x,y);\n", topo, err));
        PanmanTree t;
        pm::tree_from_topology(topo, t);
        pm::tree_from_topology(topo, t);
        CHECK(t.root == 0 && (t.child_off == I32{0, 2, 4, 4, 4, 4}) && (t.child_idx == I32{1, 4, 2, 3}));
        CHECK(t.names_blob == std::string("node_1\0node_2\0a\0b\0c\0", 20));
        CHECK((t.length == std::vector<float>{0.0f, 4.0f, 2.0f, 3.0f, 5.0f}));
        CHECK(t.newick == "((a:2.000000,b:3.000000)node_2:4.000000,c:5.000000)node_1:0.000000;" && t.newick == pm::newick_of(topo));
        expect_defaults(t, 5);
        pm::Topology same_line;
        CHECK(pm::parse_newick("((a:2,b:3):4,c:5);", same_line, err));
        CHECK(same_line.name == topo.name && same_line.kids == topo.kids && same_line.length == topo.length);
        pm::Topology bad;
        CHECK(!pm::parse_newick("((a,b),c;\n(x,y);", bad, err) && err == "incorrect Newick format");
    }
}

// ---- block mutations ----------------------------------------------------------------------------

void block_append() {
    PanmanTree t;
    t.bm_off.assign(4, 0);
    pm::append_block_muts(t, 0, {});   // an empty node still closes its list
    // type << 4 | code with NS = 0, ND = 1, NI = 2: an insertion, a deletion, an inversion (NS), an
    // inserted block on the reverse strand (NI with code 2)
    pm::append_block_muts(t, 1, {{7, 0x21}, {8, 0x10}, {9, 0x01}, {10, 0x22}});
    pm::append_block_muts(t, 2, {{4, 0x11}});   // a deletion's code does not matter
    CHECK((t.bm_off == I64{0, 0, 4, 5}));
    CHECK((t.bm_primary == I32{7, 8, 9, 10, 4}));
    CHECK((t.bm_info == U8{1, 0, 0, 1, 0}));
    CHECK((t.bm_inv == U8{0, 0, 1, 1, 0}));
}

void blocks_copied() {
    const int32_t primary[2] = {0, 5}, gap_primary[1] = {5};
    const int64_t seq_off[3] = {0, 1, 3}, gap_off[2] = {0, 2};
    const uint32_t seq[3] = {0x12480000u, 0x88888888u, 0x80000000u}, gap_pos[2] = {1, 4}, gap_len[2] = {3, 2};
    pm_panmat p{};
    p.num_blocks = 2;
    p.block_primary = primary;
    p.block_seq_offsets = seq_off;
    p.block_seq = seq;
    p.num_gaps = 1;
    p.gap_primary = gap_primary;
    p.gap_offsets = gap_off;
    p.gap_position = gap_pos;
    p.gap_length = gap_len;
    PanmanTree t;
    pm::copy_blocks(p, t);
    CHECK((t.block_primary == I32{0, 5}) && (t.block_seq_off == I64{0, 1, 3}) && (t.block_seq == U32{0x12480000u, 0x88888888u, 0x80000000u}));
    CHECK((t.gap_primary == I32{5}) && (t.gap_off == I64{0, 2}) && (t.gap_pos == U32{1, 4}) && (t.gap_len == U32{3, 2}));
}

}  // namespace

int main() {
    code_table();
    pack4_cases();
    encode_block_cases();
    group_main();
    group_gap();
    nuc_append();
    topology_cases();
    block_append();
    blocks_copied();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("build host checks ok");
    return 0;
}
