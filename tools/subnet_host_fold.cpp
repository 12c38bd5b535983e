// subnet_host_fold.cpp -- the consolidation that pm_subnet runs on the GPU (expand, stable sort, fold per
// coordinate, regroup), single-threaded on the host, to set beside the subnet.* phase times.
// A measurement tool: it links the library only to read the PanMAN and is no part of it.
//
// Build, on one line:
//   g++ -O2 -std=c++17 -Iinclude tools/subnet_host_fold.cpp -o tools/subnet_host_fold
//       -Lpanman_amd -l:libpanman_amd.so -Wl,-rpath,'$ORIGIN/../panman_amd'
//   tools/subnet_host_fold in.panman ids.txt        (ids.txt: the identifiers of tree 0, whitespace separated)
//
// Prints the merged chains, their bases, the records after regrouping and the seconds of the four steps.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "panman_gpu.h"

namespace {

struct Entry {
    uint64_t hi, lo;   // (new node, primary block), (position, gap position + 1): the sort tuple
    uint8_t type, code;
};

double since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.panman ids.txt\n", argv[0]);
        return 2;
    }
    pm_panman* file = nullptr;
    char err[512] = {0};
    pm_panmat p;
    if (pm_panman_load(argv[1], &file, err, sizeof err) != PM_OK || pm_panman_tree(file, 0, &p) != PM_OK) {
        std::fprintf(stderr, "cannot load %s: %s\n", argv[1], err);
        return 1;
    }
    const int32_t N = p.num_nodes;
    std::unordered_map<std::string, int32_t> by_name;
    const char* nm = p.names;
    for (int32_t i = 0; i < N; ++i) {
        const std::string s = nm;
        nm += s.size() + 1;
        by_name.emplace(s, i);
    }
    std::vector<int32_t> parent(N, -1);
    for (int32_t i = 0; i < N; ++i)
        for (int32_t e = p.child_offsets[i]; e < p.child_offsets[i + 1]; ++e) parent[p.child_index[e]] = i;
    std::vector<char> kept(N, 0);
    std::ifstream in(argv[2]);
    std::string id;
    while (in >> id) {
        const auto it = by_name.find(id);
        if (it == by_name.end()) {
            std::fprintf(stderr, "unknown identifier %s\n", id.c_str());
            return 1;
        }
        for (int32_t v = it->second; v >= 0 && !kept[v]; v = parent[v]) kept[v] = 1;
    }
    // the merged chains, as pm_subnet finds them: their records in chain order, top first
    std::vector<int32_t> rec_node;
    std::vector<int64_t> rec_at;
    int64_t chains = 0;
    int32_t new_nodes = 0;
    std::vector<int32_t> st{p.root}, chain, kids;
    while (!st.empty()) {
        int32_t v = st.back();
        st.pop_back();
        chain.clear();
        for (;;) {
            chain.push_back(v);
            kids.clear();
            for (int32_t e = p.child_offsets[v]; e < p.child_offsets[v + 1]; ++e)
                if (kept[p.child_index[e]]) kids.push_back(p.child_index[e]);
            if (kids.size() != 1) break;
            v = kids[0];
        }
        for (size_t j = kids.size(); j-- > 0;) st.push_back(kids[j]);
        if (chain.size() > 1) {
            ++chains;
            for (int32_t c : chain)
                for (int64_t k = p.nuc_mut_offsets[c]; k < p.nuc_mut_offsets[c + 1]; ++k) {
                    rec_node.push_back(new_nodes);
                    rec_at.push_back(k);
                }
        }
        ++new_nodes;
    }

    auto t0 = std::chrono::steady_clock::now();
    std::vector<Entry> ent;
    for (size_t r = 0; r < rec_at.size(); ++r) {
        const int64_t k = rec_at[r];
        const uint32_t info = p.nuc_mut_info[k];
        uint32_t type = info & 7u;
        const int n = type >= 3 ? 1 : (int)(info >> 4);
        type = type == PM_MUT_NS ? 3 : type == PM_MUT_NI ? 4 : type == PM_MUT_ND ? 5 : type;
        const int32_t pos = p.nuc_mut_position[k], gap = p.nuc_mut_gap_position[k];
        for (int j = 0; j < n; ++j) {
            const uint32_t q = gap == -1 ? pos + j : pos, g = gap == -1 ? 0 : gap + j + 1;
            ent.push_back(Entry{(uint64_t)rec_node[r] << 32 | (uint32_t)p.nuc_mut_primary[k], (uint64_t)q << 32 | g, (uint8_t)type,
                                (uint8_t)((p.nuc_mut_nucs[k] >> (4 * (5 - j))) & 15u)});
        }
    }
    const double t_expand = since(t0);
    t0 = std::chrono::steady_clock::now();
    std::stable_sort(ent.begin(), ent.end(), [](const Entry& a, const Entry& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; });
    const double t_sort = since(t0);
    t0 = std::chrono::steady_clock::now();
    size_t live = 0;   // survivors compacted to the front
    for (size_t i = 0; i < ent.size();) {
        bool have = false;
        uint8_t type = 0, code = 0;
        size_t j = i;
        for (; j < ent.size() && ent[j].hi == ent[i].hi && ent[j].lo == ent[i].lo; ++j) {
            const uint8_t t = ent[j].type;
            if (!have || t == type) {
                have = true;
                type = t;
            } else if (type == 3) {
                type = t == 5 ? 5 : 3;
            } else if (type == 4) {
                if (t == 5) have = false;
            } else {
                type = t == 4 ? 3 : 4;
            }
            code = ent[j].code;
        }
        if (have) ent[live++] = Entry{ent[i].hi, ent[i].lo, type, code};
        i = j;
    }
    const double t_fold = since(t0);
    t0 = std::chrono::steady_clock::now();
    int64_t records = 0;
    uint64_t check = 0;
    for (size_t i = 0; i < live;) {
        size_t j = i + 1;
        for (; j < std::min(i + 6, live); ++j) {
            const Entry &a = ent[j - 1], &b = ent[j];
            const bool main = (uint32_t)a.lo == 0;
            if (a.hi != b.hi || a.type != b.type || (main ? b.lo != a.lo + ((uint64_t)1 << 32) : b.lo != a.lo + 1)) break;
        }
        uint32_t nucs = 0;
        for (size_t k = i; k < j; ++k) nucs |= (uint32_t)ent[k].code << (4 * (5 - (k - i)));
        check = check * 1000003u + nucs + (j - i);
        ++records;
        i = j;
    }
    const double t_group = since(t0);
    std::printf("chains %lld bases %zu survivors %zu records %lld check %llx\n", (long long)chains, ent.size(), live,
                (long long)records, (unsigned long long)check);
    std::printf("host.expand=%.4f host.sort=%.4f host.fold=%.4f host.group=%.4f host.total=%.4f\n", t_expand, t_sort, t_fold,
                t_group, t_expand + t_sort + t_fold + t_group);
    pm_panman_free(file);
    return 0;
}
