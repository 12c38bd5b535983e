// aa_host.cpp -- what pm_aa computes on the GPU, single-threaded on the host and written from
// tests/_aa_ref.py: per node the whole sequence by a path walk, locate, window, codons and the literal
// two-pointer merge.  A measurement tool to set beside the aa.* phase times and to compare texts at sizes
// the Python restatement cannot reach: it links the library only to read the PanMAN and is no part of it.
//
// Build, on one line:
//   g++ -O2 -std=c++17 -Iinclude tools/aa_host.cpp -o tools/aa_host
//       -Lpanman_amd -l:libpanman_amd.so -Wl,-rpath,'$ORIGIN/../panman_amd'
//   tools/aa_host in.panman START END out.tsv        (tree 0)
//
// Prints the root's codons, the unlocated nodes, the text's bytes and the seconds of the sequences and of the rest.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "panman_gpu.h"

namespace {

const char kNuc[] = "-ACMGRSVTWYHKDBN";
// the standard genetic code: the 64 codons in TCAG order, one letter each
const char kLetters[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
const char kNames[] = "Ala---CysAspGluPheGlyHisIle---LysLeuMetAsn---ProGlnArgSerThr---ValTrp---Tyr---";

struct Block {   // structure shared by all nodes: positions 0..n (n the sentinel), slot k of position j at slot_off[j] + k
    bool is_block = false;
    std::string main, slots;
    std::vector<int32_t> slot_off;
    int32_t positions() const { return (int32_t)main.size(); }
    int32_t nslots(int32_t j) const { return slot_off[(size_t)j + 1] - slot_off[(size_t)j]; }
};
struct Node {
    std::vector<std::string> main, slots;
    std::vector<char> held, forward;
};
using Coord = std::tuple<int32_t, int32_t, int32_t>;   // block, position, slot (-1: main)
struct Codons {
    std::vector<char> aa;
    std::vector<int64_t> start, end;
};

double since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}
bool real(char ch) { return ch != '-' && ch != 'x'; }
int code_of(char ch) { return ch == 'T' ? 0 : ch == 'C' ? 1 : ch == 'A' ? 2 : ch == 'G' ? 3 : -1; }

bool locate(const std::vector<Block>& bl, const Node& s, int64_t g, Coord& out) {
    const int32_t M = (int32_t)bl.size();
    int64_t len = 0;
    for (int32_t b = 0; b < M; ++b) {
        if (!s.held[b]) continue;
        for (char ch : s.main[b]) len += real(ch);
        for (char ch : s.slots[b]) len += real(ch);
    }
    if (!(g < len)) g -= len;
    int64_t ctr = 0;
    for (int32_t b = 0; b < M; ++b) {
        if (!s.held[b]) continue;
        const int32_t n = bl[b].positions();
        if (s.forward[b]) {
            for (int32_t j = 0; j < n; ++j) {
                for (int32_t k = 0; k < bl[b].nslots(j); ++k)
                    if (real(s.slots[b][(size_t)bl[b].slot_off[j] + k])) {
                        if (ctr == g) return out = Coord(b, j, k), true;
                        ++ctr;
                    }
                if (real(s.main[b][j])) {
                    if (ctr == g) return out = Coord(b, j, -1), true;
                    ++ctr;
                }
            }
        } else {
            for (int32_t j = n - 1; j >= 0; --j) {
                if (real(s.main[b][j])) {
                    if (ctr == g) return out = Coord(b, j, -1), true;
                    ++ctr;
                }
                for (int32_t k = bl[b].nslots(j) - 1; k >= 0; --k)
                    if (real(s.slots[b][(size_t)bl[b].slot_off[j] + k])) {
                        if (ctr == g) return out = Coord(b, j, k), true;
                        ++ctr;
                    }
            }
        }
    }
    return false;
}

// false: "ERROR"; exits on a walk the reference starts out of range
bool window(const std::vector<Block>& bl, const Node& s, const Coord& st, const Coord& en, std::string& w) {
    const auto [b0, j0, k0] = st;
    w.clear();
    for (int32_t i = b0; i <= std::get<0>(en); ++i) {
        const Block& b = bl[i];
        const int32_t n = b.positions();
        if (s.forward[i]) {
            for (int32_t j = i == b0 ? j0 : 0; j < n; ++j) {
                if (k0 != -1)
                    for (int32_t k = k0; k < b.nslots(j); ++k) {
                        if (Coord(i, j, k) == en) return true;
                        w.push_back(s.held[i] ? s.slots[i][(size_t)b.slot_off[j] + k] : '-');
                    }
                if (Coord(i, j, -1) == en) return true;
                w.push_back(s.held[i] ? s.main[i][j] : '-');
            }
        } else {
            int32_t top = j0;
            if (i != b0) {
                top = bl[0].positions() - 1;
                if (top < 0 || top >= n) {
                    std::fprintf(stderr, "unsupported: a reverse-strand walk starts outside block %d\n", i);
                    std::exit(3);
                }
            }
            for (int32_t j = top; j >= 0; --j) {
                if (Coord(i, j, -1) == en) return true;
                w.push_back(s.held[i] ? s.main[i][j] : '-');
                for (int32_t k = (i == b0 && j == j0) ? k0 : b.nslots(j) - 1; k >= 0; --k) {
                    if (Coord(i, j, k) == en) return true;
                    w.push_back(s.held[i] ? s.slots[i][(size_t)b.slot_off[j] + k] : '-');
                }
            }
        }
    }
    return false;
}

Codons codons(const std::string& w) {
    Codons c;
    int cur[3], have = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        const int code = code_of(w[i]);
        if (code >= 0) {
            if (have == 0) c.start.push_back((int64_t)i);
            cur[have++] = code;
        }
        if (have == 3) {
            c.end.push_back((int64_t)i);
            c.aa.push_back(kLetters[16 * cur[0] + 4 * cur[1] + cur[2]]);
            have = 0;
        }
    }
    while (c.start.size() > c.end.size()) c.start.pop_back();
    return c;
}

void put_name(std::string& out, char letter) {
    if (letter == '*') out += '*';
    else out.append(kNames + 3 * (letter - 'A'), 3);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s in.panman START END out.tsv\n", argv[0]);
        return 2;
    }
    pm_panman* file = nullptr;
    char err[512] = {0};
    pm_panmat p;
    if (pm_panman_load(argv[1], &file, err, sizeof err) != PM_OK || pm_panman_tree(file, 0, &p) != PM_OK) {
        std::fprintf(stderr, "cannot load %s: %s\n", argv[1], err);
        return 1;
    }
    const int64_t start = std::atoll(argv[2]), end = std::atoll(argv[3]);
    if (end <= start) return std::fprintf(stderr, "End coordinate must be greater than start\n"), 1;
    const int32_t N = p.num_nodes;
    std::vector<std::string> names(N);
    const char* nm = p.names;
    for (int32_t i = 0; i < N; ++i) {
        names[i] = nm;
        nm += names[i].size() + 1;
    }
    std::vector<int32_t> parent(N, -1);
    for (int32_t i = 0; i < N; ++i)
        for (int32_t e = p.child_offsets[i]; e < p.child_offsets[i + 1]; ++e) parent[p.child_index[e]] = i;
    int32_t M = 0;
    for (int32_t b = 0; b < p.num_blocks; ++b) M = std::max(M, p.block_primary[b] + 1);
    std::vector<Block> bl(M);
    for (int32_t b = 0; b < p.num_blocks; ++b) {
        Block& k = bl[p.block_primary[b]];
        k.is_block = true;
        bool stop = false;
        for (int64_t w = p.block_seq_offsets[b]; w < p.block_seq_offsets[b + 1] && !stop; ++w)
            for (int q = 0; q < 8; ++q) {
                const int code = (p.block_seq[w] >> (4 * (7 - q))) & 15;
                if (code == 0) {
                    stop = true;
                    break;
                }
                k.main.push_back(kNuc[code]);
            }
        k.main.push_back('x');
    }
    {
        std::vector<std::vector<int32_t>> count(M);
        for (int32_t b = 0; b < M; ++b) count[b].assign(bl[b].main.size(), 0);
        for (int32_t g = 0; g < p.num_gaps; ++g)
            for (int64_t k = p.gap_offsets[g]; k < p.gap_offsets[g + 1]; ++k) count[p.gap_primary[g]][p.gap_position[k]] = (int32_t)p.gap_length[k];
        for (int32_t b = 0; b < M; ++b) {
            bl[b].slot_off.assign(bl[b].main.size() + 1, 0);
            for (size_t j = 0; j < bl[b].main.size(); ++j) bl[b].slot_off[j + 1] = bl[b].slot_off[j] + count[b][j];
            bl[b].slots.assign((size_t)bl[b].slot_off.back(), '-');
        }
    }

    auto state = [&](int32_t v) {
        Node s;
        s.main.resize(M);
        s.slots.resize(M);
        s.held.assign(M, 0);
        s.forward.assign(M, 1);
        for (int32_t b = 0; b < M; ++b) {
            s.main[b] = bl[b].main;
            s.slots[b] = bl[b].slots;
        }
        std::vector<int32_t> path;
        for (int32_t u = v; u >= 0; u = parent[u]) path.push_back(u);
        for (size_t q = path.size(); q-- > 0;) {
            const int32_t u = path[q];
            for (int64_t k = p.block_mut_offsets[u]; k < p.block_mut_offsets[u + 1]; ++k) {
                const int32_t b = p.block_mut_primary[k];
                if (p.block_mut_info[k]) s.held[b] = 1, s.forward[b] = !p.block_mut_inversion[k];
                else if (p.block_mut_inversion[k]) s.forward[b] = !s.forward[b];
                else s.held[b] = 0, s.forward[b] = 1;
            }
            for (int64_t k = p.nuc_mut_offsets[u]; k < p.nuc_mut_offsets[u + 1]; ++k) {
                if (p.nuc_mut_secondary[k] != -1) {
                    std::fprintf(stderr, "unsupported: secondary blocks\n");
                    std::exit(3);
                }
                const int32_t b = p.nuc_mut_primary[k], pos = p.nuc_mut_position[k], gap = p.nuc_mut_gap_position[k];
                const int type = p.nuc_mut_info[k] & 7;
                int len = p.nuc_mut_info[k] >> 4;
                if (type > 5) continue;
                if (type >= 3) len = 1;
                for (int j = 0; j < len; ++j) {
                    const char ch = (type == 1 || type == 5) ? '-' : kNuc[(p.nuc_mut_nucs[k] >> (4 * (5 - j))) & 15];
                    if (gap != -1) s.slots[b][(size_t)bl[b].slot_off[pos] + gap + j] = ch;
                    else s.main[b][(size_t)pos + j] = ch;
                }
            }
        }
        for (int32_t b = 0; b < M; ++b)
            if (!s.held[b]) s.forward[b] = 1;   // an absent block counts as forward
        return s;
    };

    double t_seq = 0.0, t_rest = 0.0;
    auto t0 = std::chrono::steady_clock::now();
    const Node root = state(p.root);
    t_seq += since(t0);
    t0 = std::chrono::steady_clock::now();
    Coord S, E;
    if (!locate(bl, root, start, S) || !locate(bl, root, end, E)) return std::fprintf(stderr, "coordinates out of range\n"), 1;
    std::string w;
    if (!window(bl, root, S, E, w)) return std::fprintf(stderr, "the root's window is ERROR\n"), 1;
    const Codons ref = codons(w);
    t_rest += since(t0);
    std::string text;
    int64_t unlocated = 0;
    if (!ref.aa.empty()) {
        text = "node_id\taa_mutations\n";
        for (int32_t v = 0; v < N; ++v) {
            t0 = std::chrono::steady_clock::now();
            const Node s = state(v);
            t_seq += since(t0);
            t0 = std::chrono::steady_clock::now();
            if (!locate(bl, s, start, S) || !locate(bl, s, end, E)) {
                ++unlocated;
                t_rest += since(t0);
                continue;
            }
            Codons alt;
            if (window(bl, s, S, E, w)) alt = codons(w);
            // the two-pointer loop of aaTrans.cpp:259-285
            std::vector<std::pair<size_t, char>> matches, insertions;
            std::vector<size_t> deletions;
            size_t r = 0, a = 0;
            while (a < alt.start.size() && r < ref.start.size()) {
                if (alt.start[a] > ref.end[r]) deletions.push_back(r++);
                else if (alt.start[a] < ref.start[r]) insertions.emplace_back(r, alt.aa[a++]);
                else matches.emplace_back(r++, alt.aa[a++]);
            }
            while (a < alt.start.size()) insertions.emplace_back(r, alt.aa[a++]);
            while (r < ref.start.size()) deletions.push_back(r++);
            std::string line;
            for (const auto& m : matches)
                if (ref.aa[m.first] != m.second) {
                    line += "S:" + std::to_string(m.first) + ":";
                    put_name(line, m.second);
                    line += ';';
                }
            for (const auto& m : insertions) {
                line += "I:" + std::to_string(m.first) + ":";
                put_name(line, m.second);
                line += ';';
            }
            for (size_t d : deletions) line += "D:" + std::to_string(d) + ";";
            if (!line.empty()) text += names[v] + "\t" + line + "\n";
            t_rest += since(t0);
        }
    }
    FILE* f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size() || std::fclose(f) != 0) return std::fprintf(stderr, "cannot write %s\n", argv[4]), 1;
    std::printf("host one thread: ref_codons %zu unlocated %lld text_bytes %zu sequences_s %.4f locate_window_merge_s %.4f\n",
                ref.aa.size(), (long long)unlocated, text.size(), t_seq, t_rest);
    pm_panman_free(file);
    return 0;
}
