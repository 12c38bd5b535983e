// panmanUtils-compatible command line for the GPU path (src/panmanUtils.cpp:128-182 option
// table, :1302-1325 PanMAN load, :1409-1465 MSA build, :1326-1362 GFA build, :271-299 writePanMAN, :385-415 and
// :458-490 FASTA / aligned FASTA, :584-652 subnetwork extraction, :699-732 GFA, :741-763 MAF, :766-786 Newick,
// :895-938 amino-acid translation, :1008-1071 mutation printing, :1205-1240 UShER MAT export,
// :328-354 N imputation up to its plan of moves).  Only the commands on the accelerated
// path are implemented; any other reference command is rejected with a message.
#include <fcntl.h>
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "panman_gpu.h"

namespace {

using Clock = std::chrono::high_resolution_clock;

long long ns_since(Clock::time_point t0) {
    return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count();
}

struct Options {
    std::map<std::string, std::string> values;   // long name -> value ("" for flags)
    bool has(const char* k) const { return values.count(k) != 0; }
    const std::string& get(const char* k) const { return values.at(k); }
};

struct Spec {
    const char* name;
    char shortc;
    bool takes_value;
    const char* help;
};

const Spec kSpecs[] = {
    {"help", 'h', false, "Print help messages"},
    {"input-panman", 'I', true, "Input PanMAN file path"},
    {"input-msa", 'M', true, "Input MSA file (FASTA format) to build a PanMAN"},
    {"input-pangraph", 'P', true, "Input PanGraph JSON file to build a PanMAN"},
    {"input-gfa", 'G', true, "Input GFA file to build a PanMAN"},
    {"input-newick", 'N', true, "Input tree topology as Newick string"},
    {"summary", 's', false, "Print PanMAN summary"},
    {"newick", 't', false, "Print newick string of all trees in a PanMAN"},
    {"fasta", 'f', false, "Print tip sequences (FASTA format)"},
    {"fasta-aligned", 'm', false, "Print MSA of sequences for each PanMAT in a PanMAN (FASTA format)"},
    {"maf", 'w', false, "Print m-WGA for each PanMAT in a PanMAN (MAF format)"},
    {"gfa", 'g', false, "Convert any PanMAT in a PanMAN to a GFA file"},
    {"subnet", 'b', false, "Extract subnet of given PanMAN to a new PanMAN file based on the list of nodes provided in the input-file"},
    {"input-file", 'i', true, "Path to the input file, required for --subnet (one line per tree: treeID id id ...)"},
    {"impute", 0, false, "Create new PanMAN with the N substitutions imputed; the moves found for insertions to N are planned in ./info/<output-file>_<tree>.moves, not applied (needs --output-file)"},
    {"max-insertion-impute-distance", 'D', true, "Maximum total branch length to move a node for insertion imputation [default 5]"},
    {"reroot", 'r', false, "Reroot a PanMAT in a PanMAN based on the input sequence id (--reference)"},
    {"printMutations", 'p', false, "Print mutations from root to each node (every node of the tree given by --treeID, default 0)"},
    {"toUsher", 0, false, "Convert a PanMAT in a PanMAN to an UShER MAT (needs --output-file, the file's name as given, and --reference; --treeID, default 0)"},
    {"aa-translation", 0, false, "Extract amino acid translations in TSV file (needs --treeID, --start and --end)"},
    {"start", 'x', true, "Start coordinate of protein translation"},
    {"end", 'y', true, "End coordinate of protein translation"},
    {"treeID", 'd', true, "Tree ID, required for --reroot and --aa-translation; the tree of --maf and --gfa (default 0)"},
    {"protobuf2capnp", 0, false, "Converts a Google Protobuf PanMAN (-I) to a Cap'n Proto PanMAN (-o)"},
    {"low-mem-mode", 0, false, "Build with the Sankoff driver (the reference's batched low-memory mode)"},
    {"reference", 'n', true, "Identifier of reference sequence for PanMAN construction (optional) or reroot (required)"},
    {"output-file", 'o', true, "Prefix of the output file name"},
    {"threads", 0, true, "Accepted for compatibility (the build runs on the GPU)"},
    {"device", 0, true, "First HIP device ordinal (default 0)"},
    {"gpus", 0, true, "Number of GPUs (devices device..device+N-1): MSA columns / FASTA leaves are split across them"},
    {"backend", 0, true, "Compute backend: hip (the only one; there is no CPU product path)"},
};

// Reference commands outside the accelerated path: recognised so the error is explicit.
const char* const kOther[] = {"create-network", "printTips",
                              "vcf", "annotate",
                              "extended-newick", "acr", "index"};

void usage(std::ostream& os) {
    os << "Allowed options:\n";
    for (const Spec& s : kSpecs) {
        std::string flag = "  --" + std::string(s.name);
        if (s.shortc) flag += std::string(" [ -") + s.shortc + " ]";
        if (s.takes_value) flag += " arg";
        os << flag << std::string(flag.size() < 36 ? 36 - flag.size() : 1, ' ') << s.help << "\n";
    }
}

const Spec* find_long(const std::string& n) {
    for (const Spec& s : kSpecs)
        if (n == s.name) return &s;
    return nullptr;
}

const Spec* find_short(char c) {
    for (const Spec& s : kSpecs)
        if (s.shortc == c) return &s;
    return nullptr;
}

bool parse(int argc, char** argv, Options& o, std::string& err) {
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        const Spec* s = nullptr;
        std::string inline_value;
        bool has_inline = false;
        if (a.rfind("--", 0) == 0) {
            std::string n = a.substr(2);
            const size_t eq = n.find('=');
            if (eq != std::string::npos) {
                inline_value = n.substr(eq + 1);
                n.resize(eq);
                has_inline = true;
            }
            s = find_long(n);
            if (!s) {
                for (const char* other : kOther)
                    if (n == other) {
                        err = "--" + n + " is not part of the GPU path of this build";
                        return false;
                    }
                err = "unrecognised option '" + a + "'";
                return false;
            }
        } else if (a.size() >= 2 && a[0] == '-') {
            s = find_short(a[1]);
            if (!s) {
                err = "unrecognised option '" + a + "'";
                return false;
            }
            if (a.size() > 2) {
                inline_value = a.substr(2);
                has_inline = true;
            }
        } else {
            o.values["input-panman"] = a;   // positional argument (src/panmanUtils.cpp:183)
            continue;
        }
        if (s->takes_value) {
            if (has_inline) {
                o.values[s->name] = inline_value;
            } else if (i + 1 < argc) {
                o.values[s->name] = argv[++i];
            } else {
                err = std::string("the required argument for option '--") + s->name + "' is missing";
                return false;
            }
        } else {
            o.values[s->name] = "";
        }
    }
    return true;
}

bool read_file(const std::string& path, std::string& out) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    std::ostringstream ss;
    ss << in.rdbuf();
    out = ss.str();
    return true;
}

// a CLI phase in the same log as the library's (PANMAN_PHASES)
void cli_phase(const char* name, Clock::time_point t0) {
    if (const char* ph = std::getenv("PANMAN_PHASES"); ph && ph[0] == '1')
        std::cerr << name << "\t" << ns_since(t0) * 1e-9 << "\n";
}

void print_error(const std::string& e) { std::cerr << "\033[1;31mError: " << e << "\033[0m\n"; }

int build_from_msa(const Options& o, const std::vector<int>& devices) {
    if (!o.has("input-newick")) {
        print_error("File containing newick string not provided!");
        return 1;
    }
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        usage(std::cout);
        return 1;
    }
    std::string msa, newick;
    const auto r0 = Clock::now();
    if (!read_file(o.get("input-msa"), msa)) {
        print_error("cannot read " + o.get("input-msa"));
        return 1;
    }
    if (!read_file(o.get("input-newick"), newick)) {
        print_error("cannot read " + o.get("input-newick"));
        return 1;
    }
    cli_phase("cli.read_inputs", r0);
    const std::string ref = o.has("reference") ? o.get("reference") : "";
    const int mode = o.has("low-mem-mode") ? PM_MODE_SANKOFF : PM_MODE_FITCH;
    std::cout << "Creating PanMAN from MSA and Newick" << std::endl;
    ::mkdir("./panman", 0777);
    const std::string out = "./panman/" + o.get("output-file") + ".panman";
    const auto t0 = Clock::now();
    char err[512] = {0};
    const int rc = pm_msa_to_panman_multi(newick.c_str(), msa.c_str(), ref.c_str(), mode, devices.data(),
                                          (int)devices.size(), out.c_str(), err, sizeof err);
    if (rc != PM_OK) {
        print_error(err[0] ? err : "PanMAN construction failed");
        return 1;
    }
    // Construction and the xz write are one call here; both lines report its time.
    const long long t = ns_since(t0);
    std::cout << "Data load time: " << t << " nanoseconds \n";
    std::cout << "Writing PanMAN" << std::endl;
    std::cout << "\nNetwork Write execution time: " << t << " nanoseconds\n";
    return 0;
}

int reroot(const Options& o, const pm_panman* file, int device) {
    if (!o.has("treeID")) {
        print_error("TreeID not provided!");
        usage(std::cout);
        return 1;
    }
    const int tree_id = std::atoi(o.get("treeID").c_str());
    if (tree_id < 0 || tree_id >= pm_panman_tree_count(file)) {
        print_error("TreeID out of range");
        return 1;
    }
    if (!o.has("reference")) {
        print_error("Refence ID not provided!");
        usage(std::cout);
        return 1;
    }
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        return 1;
    }
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    pm_panmat view;
    pm_panman* res = nullptr;
    const auto t0 = Clock::now();
    int rc = pm_panman_tree(file, tree_id, &view);
    if (rc == PM_OK) rc = pm_reroot(ctx, &view, o.get("reference").c_str(), &res);
    if (rc != PM_OK) {
        print_error(pm_last_error(ctx));
        pm_destroy(ctx);
        return 1;
    }
    std::cout << "\nReroot execution time: " << ns_since(t0) << " nanoseconds\n";
    std::vector<pm_panmat> views(pm_panman_tree_count(file));
    std::vector<const pm_panmat*> list;
    for (int i = 0; i < (int)views.size(); ++i) {
        if (i == tree_id) pm_panman_tree(res, 0, &views[i]);
        else pm_panman_tree(file, i, &views[i]);
        list.push_back(&views[i]);
    }
    std::cout << "Writing PanMAN" << std::endl;
    ::mkdir("./panman", 0777);
    const std::string out = "./panman/" + o.get("output-file") + ".panman";
    const auto w0 = Clock::now();
    rc = pm_panman_write(out.c_str(), list.data(), (int)list.size(), 1);
    std::cout << "\nNetwork Write execution time: " << ns_since(w0) << " nanoseconds\n";
    pm_panman_free(res);
    pm_destroy(ctx);
    if (rc != PM_OK) {
        print_error("cannot write " + out);
        return 1;
    }
    return 0;
}

// -I in.panman --subnet -i ids.txt -o out (src/panmanUtils.cpp:584-652): every tree cut down to the nodes its
// line of the input file names ("treeID id id ..."), written as ./panman/<out>.panman.
int subnet(const Options& o, const pm_panman* file, int device) {
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        usage(std::cout);
        return 1;
    }
    if (!o.has("input-file")) {
        print_error("Input file not provided!");
        usage(std::cout);
        return 1;
    }
    std::ifstream in(o.get("input-file"));
    if (!in) {
        print_error("cannot read " + o.get("input-file"));
        return 1;
    }
    const int trees = pm_panman_tree_count(file);
    std::map<int, std::vector<std::string>> ids;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream words(line);
        std::string word;
        if (!(words >> word)) continue;
        std::vector<std::string>& list = ids[std::atoi(word.c_str())];
        while (words >> word) list.push_back(word);
    }
    // (the reference would dereference a null root for a tree without a line)
    for (int i = 0; i < trees; ++i)
        if (!ids.count(i) || ids[i].empty()) {
            print_error("no node identifiers for tree " + std::to_string(i) + " in " + o.get("input-file"));
            return 1;
        }
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    std::vector<pm_panman*> results(trees, nullptr);
    std::vector<pm_panmat> views(trees);
    std::vector<const pm_panmat*> list;
    int status = 0;
    const auto t0 = Clock::now();
    for (int i = 0; i < trees && status == 0; ++i) {
        pm_panmat view;
        std::vector<const char*> names;
        for (const std::string& id : ids[i]) names.push_back(id.c_str());
        if (pm_panman_tree(file, i, &view) != PM_OK ||
            pm_subnet(ctx, &view, names.data(), (int64_t)names.size(), &results[i]) != PM_OK) {
            print_error(pm_last_error(ctx));
            status = 1;
            break;
        }
        pm_panman_tree(results[i], 0, &views[i]);
        list.push_back(&views[i]);
    }
    if (status == 0) {   // (the reference's time covers the extraction and the write)
        ::mkdir("./panman", 0777);
        const std::string out = "./panman/" + o.get("output-file") + ".panman";
        if (pm_panman_write(out.c_str(), list.data(), (int)list.size(), 1) != PM_OK) {
            print_error("cannot write " + out);
            status = 1;
        } else {
            std::cout << "\nParallel Subnetwork Extract execution time: " << ns_since(t0) << " nanoseconds\n";
        }
    }
    for (pm_panman* r : results) pm_panman_free(r);
    pm_destroy(ctx);
    return status;
}

// -I in.panman --impute [-D distance] -o out (src/panmanUtils.cpp:328-354): Tree::imputeNs of every tree up to the
// plan of moves (pm_impute), written as ./panman/<out>.panman; tree i's plan goes to ./info/<out>_<i>.moves.
int impute(const Options& o, const pm_panman* file, int device) {
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        usage(std::cout);
        return 1;
    }
    int distance = 5;
    if (o.has("max-insertion-impute-distance")) {
        char* end = nullptr;
        const std::string& text = o.get("max-insertion-impute-distance");
        const long long v = std::strtoll(text.c_str(), &end, 10);
        if (text.empty() || *end || v < -2147483647LL || v > 2147483647LL) {
            print_error("the argument ('" + text + "') for option '--max-insertion-impute-distance' is invalid");
            return 1;
        }
        distance = (int)v;
    }
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    const int trees = pm_panman_tree_count(file);
    std::vector<pm_panman*> results(trees, nullptr);
    std::vector<pm_panmat> views(trees);
    std::vector<const pm_panmat*> list;
    std::vector<std::string> plans(trees);
    int status = 0;
    const auto t0 = Clock::now();
    for (int i = 0; i < trees && status == 0; ++i) {
        pm_panmat view;
        pm_impute_stats stats;
        char* plan = nullptr;
        int64_t length = 0;
        if (pm_panman_tree(file, i, &view) != PM_OK ||
            pm_impute(ctx, &view, distance, &results[i], &plan, &length, &stats) != PM_OK) {
            print_error(pm_last_error(ctx));
            status = 1;
            break;
        }
        plans[i].assign(plan, (size_t)length);
        pm_free(plan);
        std::cout << "Imputed " << stats.imputed_bases << "/" << stats.imputed_bases << " SNPs/MNPs to N" << std::endl;
        std::cout << "Moved 0/" << stats.insertion_nodes << " nodes with insertions to N (" << stats.moves_found
                  << " moves found, not applied)" << std::endl;
        pm_panman_tree(results[i], 0, &views[i]);
        list.push_back(&views[i]);
    }
    if (status == 0) {
        std::cout << "\nImputation time: " << ns_since(t0) << " nanoseconds\n";
        ::mkdir("./panman", 0777);
        ::mkdir("./info", 0777);
        const std::string out = "./panman/" + o.get("output-file") + ".panman";
        std::cout << "Writing PanMAN" << std::endl;
        const auto w0 = Clock::now();
        if (pm_panman_write(out.c_str(), list.data(), (int)list.size(), 1) != PM_OK) {
            print_error("cannot write " + out);
            status = 1;
        }
        std::cout << "\nNetwork Write execution time: " << ns_since(w0) << " nanoseconds\n";
        for (int i = 0; i < trees && status == 0; ++i) {
            const std::string p = "./info/" + o.get("output-file") + "_" + std::to_string(i) + ".moves";
            std::ofstream f(p, std::ios::binary);
            f.write(plans[i].data(), (std::streamsize)plans[i].size());
            if (!f) {
                print_error("cannot write " + p);
                status = 1;
            }
        }
    }
    for (pm_panman* r : results) pm_panman_free(r);
    pm_destroy(ctx);
    return status;
}

// -I in.panman --maf [--treeID k] [-o out] (src/panmanUtils.cpp:741-763): Tree::printMAF of one
// tree to stdout or ./info/<out>.maf, streamed from the device (pm_maf_fd).
// -I in.panman --gfa [--treeID k] [-o out] (src/panmanUtils.cpp:699-732): Tree::convertToGFA of
// one tree to stdout or ./info/<out>.gfa (pm_gfa_fd).
int one_tree_text(const Options& o, const pm_panman* file, int device, const char* ext,
                  int (*extract)(pm_ctx*, const pm_panmat*, int, int64_t*), const char* time_line) {
    const int tree_id = o.has("treeID") ? std::atoi(o.get("treeID").c_str()) : 0;
    if (tree_id < 0 || tree_id >= pm_panman_tree_count(file)) {
        print_error("TreeID out of range");
        return 1;
    }
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    int fd = 1;
    const bool to_file = o.has("output-file");
    if (to_file) {
        const std::string p = "./info/" + o.get("output-file") + ext;
        fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) {
            print_error("cannot write " + p);
            pm_destroy(ctx);
            return 1;
        }
    } else {
        std::cout.flush();
        std::fflush(stdout);
    }
    int status = 0;
    pm_panmat view;
    int64_t len = 0;
    const auto t0 = Clock::now();
    if (pm_panman_tree(file, tree_id, &view) != PM_OK || extract(ctx, &view, fd, &len) != PM_OK) {
        print_error(pm_last_error(ctx));
        status = 1;
    }
    const long long t = ns_since(t0);
    if (to_file && ::close(fd) != 0) status = 1;
    pm_destroy(ctx);
    if (status == 0) std::cout << time_line << t << " nanoseconds\n";
    return status;
}

// -I in.panman --printMutations [--treeID k] [-o out] (src/panmanUtils.cpp:1008-1071):
// Tree::printMutationsNew(std::ostream&) of one tree to stdout or ./info/<out>.mutations
// (pm_print_mutations_fd).  The forms with a node list (--input-file) or a reference string
// (--refFile) are not built.
int print_mutations_fd(pm_ctx* ctx, const pm_panmat* view, int fd, int64_t* length) {
    return pm_print_mutations_fd(ctx, view, fd, length, nullptr);
}

int print_mutations(const Options& o, const pm_panman* file, int device) {
    if (o.has("input-file")) {
        print_error("--printMutations with --input-file: the node-list and --refFile forms are not built");
        return 1;
    }
    return one_tree_text(o, file, device, ".mutations", print_mutations_fd, "\nMutation extract execution time: ");
}

// -I in.panman --toUsher -o NAME -n REF [--treeID k] (src/panmanUtils.cpp:1205-1240): panmanToUsher of
// one tree into the file NAME exactly as given -- no ./info/ prefix and no extension, as in the
// reference (pm_to_usher_fd).  -n is required as there, though panmanToUsher never reads it.  The
// reference converts every tree into the same file, so the last one survives; here the tree is
// --treeID, default 0.  A missing -o or -n prints the reference's message and ends with status 1 (the
// reference returns silently with status 0).  A NAME containing ".gz" is refused: the reference
// gzips such a file, this build links no gzip.
int to_usher(const Options& o, const pm_panman* file, int device) {
    if (!o.has("output-file")) {
        std::cout << "Output File not provided" << std::endl;
        return 1;
    }
    if (!o.has("reference")) {
        std::cout << "Reference not provided" << std::endl;
        return 1;
    }
    const std::string p = o.get("output-file");
    if (p.find(".gz") != std::string::npos) {
        print_error("--toUsher: gzip output (a name containing .gz) is not built; give a plain name and compress the file");
        return 1;
    }
    const int tree_id = o.has("treeID") ? std::atoi(o.get("treeID").c_str()) : 0;
    if (tree_id < 0 || tree_id >= pm_panman_tree_count(file)) {
        print_error("TreeID out of range");
        return 1;
    }
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    const int fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) {
        print_error("cannot write " + p);
        pm_destroy(ctx);
        return 1;
    }
    int status = 0;
    pm_panmat view;
    int64_t len = 0;
    const auto t0 = Clock::now();
    if (pm_panman_tree(file, tree_id, &view) != PM_OK || pm_to_usher_fd(ctx, &view, fd, &len, nullptr) != PM_OK) {
        print_error(pm_last_error(ctx));
        status = 1;
    }
    const long long t = ns_since(t0);
    if (::close(fd) != 0) status = 1;
    pm_destroy(ctx);
    if (status == 0) std::cout << "\nUsher Conversion time: " << t << " nanoseconds\n";
    return status;
}

// -I in.panman --aa-translation --treeID k -x start -y end [-o out] (src/panmanUtils.cpp:895-938):
// Tree::extractAminoAcidTranslations of one tree to stdout or ./info/<out>.tsv (pm_aa / pm_aa_fd).
// stdout receives the reference's "<n> <n> <n>" line (the sizes of the root's three codon lists)
// before the text and the timing line after it.
int aa_translation(const Options& o, const pm_panman* file, int device) {
    if (!o.has("treeID")) {
        print_error("TreeID not provided!");
        usage(std::cout);
        return 1;
    }
    const int tree_id = std::atoi(o.get("treeID").c_str());
    if (tree_id < 0 || tree_id >= pm_panman_tree_count(file)) {
        print_error("TreeID out of range");
        return 1;
    }
    if (!o.has("start") || !o.has("end")) {
        std::cout << "Start/End Coordinate not provided" << std::endl;
        return 1;
    }
    const int64_t start = std::strtoll(o.get("start").c_str(), nullptr, 10), end = std::strtoll(o.get("end").c_str(), nullptr, 10);
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    int fd = -1;
    const bool to_file = o.has("output-file");
    if (to_file) {
        const std::string p = "./info/" + o.get("output-file") + ".tsv";
        fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) {
            print_error("cannot write " + p);
            pm_destroy(ctx);
            return 1;
        }
    }
    int status = 0;
    pm_panmat view;
    char* text = nullptr;
    int64_t len = 0, codons = 0, unlocated = 0;
    const auto t0 = Clock::now();
    int rc = pm_panman_tree(file, tree_id, &view);
    if (rc == PM_OK)
        rc = to_file ? pm_aa_fd(ctx, &view, start, end, fd, &len, &codons, &unlocated)
                     : pm_aa(ctx, &view, start, end, &text, &len, &codons, &unlocated);
    if (rc != PM_OK) {
        print_error(pm_last_error(ctx));
        status = 1;
    } else {
        std::cout << codons << " " << codons << " " << codons << std::endl;
        if (!to_file) {
            std::cout.flush();
            if (std::fwrite(text, 1, (size_t)len, stdout) != (size_t)len || std::fflush(stdout) != 0) status = 1;
        }
        if (unlocated) std::cerr << unlocated << " nodes: coordinates out of range, no line\n";
    }
    const long long t = ns_since(t0);
    pm_free(text);
    if (to_file && ::close(fd) != 0) status = 1;
    pm_destroy(ctx);
    if (status == 0) std::cout << "\nAmino Acid translate execution time: " << t << " nanoseconds\n";
    return status;
}

// -P pangraph.json -N tree.nwk -o out [-n ref] (src/panmanUtils.cpp:1364-1407)
int build_from_pangraph(const Options& o, int device) {
    if (!o.has("input-newick")) {
        print_error("File containing newick string not provided!");
        return 1;
    }
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        usage(std::cout);
        return 1;
    }
    std::string json, newick;
    if (!read_file(o.get("input-pangraph"), json)) {
        print_error("cannot read " + o.get("input-pangraph"));
        return 1;
    }
    if (!read_file(o.get("input-newick"), newick)) {
        print_error("cannot read " + o.get("input-newick"));
        return 1;
    }
    std::cout << "Creating PanMAN from PanGraph and Newick" << std::endl;
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    const auto t0 = Clock::now();
    pm_panman* res = nullptr;
    const std::string ref = o.has("reference") ? o.get("reference") : "";
    if (pm_pangraph_build(ctx, json.c_str(), newick.c_str(), ref.c_str(), &res) != PM_OK) {
        print_error(pm_last_error(ctx));
        pm_destroy(ctx);
        return 1;
    }
    std::cout << "Data load time: " << ns_since(t0) << " nanoseconds \n";
    std::cout << "Writing PanMAN" << std::endl;
    ::mkdir("./panman", 0777);
    const std::string out = "./panman/" + o.get("output-file") + ".panman";
    pm_panmat view;
    pm_panman_tree(res, 0, &view);
    const pm_panmat* list[1] = {&view};
    const auto w0 = Clock::now();
    const int rc = pm_panman_write(out.c_str(), list, 1, 1);
    std::cout << "\nNetwork Write execution time: " << ns_since(w0) << " nanoseconds\n";
    pm_panman_free(res);
    pm_destroy(ctx);
    if (rc != PM_OK) {
        print_error("cannot write " + out);
        return 1;
    }
    return 0;
}

// -G graph.gfa -N tree.nwk -o out (src/panmanUtils.cpp:1326-1362)
int build_from_gfa(const Options& o, int device) {
    if (!o.has("input-newick")) {
        print_error("File containing newick string not provided!");
        return 1;
    }
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        usage(std::cout);
        return 1;
    }
    std::string text, newick;
    if (!read_file(o.get("input-gfa"), text)) {
        print_error("cannot read " + o.get("input-gfa"));
        return 1;
    }
    if (!read_file(o.get("input-newick"), newick)) {
        print_error("cannot read " + o.get("input-newick"));
        return 1;
    }
    std::cout << "Creating PanMAN from GFA and Newick" << std::endl;
    pm_ctx* ctx = nullptr;
    if (pm_create(device, &ctx) != PM_OK) {
        print_error("no HIP device");
        return 1;
    }
    const auto t0 = Clock::now();
    pm_panman* res = nullptr;
    if (pm_gfa_build(ctx, text.c_str(), newick.c_str(), &res) != PM_OK) {
        print_error(pm_last_error(ctx));
        pm_destroy(ctx);
        return 1;
    }
    std::cout << "Data load time: " << ns_since(t0) << " nanoseconds \n";
    std::cout << "Writing PanMAN" << std::endl;
    ::mkdir("./panman", 0777);
    const std::string out = "./panman/" + o.get("output-file") + ".panman";
    pm_panmat view;
    pm_panman_tree(res, 0, &view);
    const pm_panmat* list[1] = {&view};
    const auto w0 = Clock::now();
    const int rc = pm_panman_write(out.c_str(), list, 1, 1);
    std::cout << "\nNetwork Write execution time: " << ns_since(w0) << " nanoseconds\n";
    pm_panman_free(res);
    pm_destroy(ctx);
    if (rc != PM_OK) {
        print_error("cannot write " + out);
        return 1;
    }
    return 0;
}

// --protobuf2capnp -I old.panman -o out (src/panmanUtils.cpp:939-952, 1267-1268): the older
// Protobuf PanMAN read and written back as ./panman/<out>.panman (writePanMAN, :271-299).
int protobuf2capnp(const Options& o) {
    if (!o.has("output-file")) {
        print_error("Output file not provided!");
        usage(std::cout);
        return 1;
    }
    const std::string path = o.get("input-panman");
    std::cout << "starting reading panman" << std::endl;
    pm_panman* file = nullptr;
    char err[512] = {0};
    if (pm_panman_load_old(path.c_str(), &file, err, sizeof err) != PM_OK) {
        print_error(err[0] ? err : ("cannot load " + path));
        return 1;
    }
    std::vector<pm_panmat> views(pm_panman_tree_count(file));
    std::vector<const pm_panmat*> list;
    for (int i = 0; i < (int)views.size(); ++i) {
        pm_panman_tree(file, i, &views[i]);
        list.push_back(&views[i]);
    }
    std::cout << "Writing PanMAN" << std::endl;
    ::mkdir("./panman", 0777);
    const std::string out = "./panman/" + o.get("output-file") + ".panman";
    const auto w0 = Clock::now();
    const int rc = pm_panman_write(out.c_str(), list.data(), (int)list.size(), 1);
    std::cout << "\nNetwork Write execution time: " << ns_since(w0) << " nanoseconds\n";
    pm_panman_free(file);
    if (rc != PM_OK) {
        print_error("cannot write " + out);
        return 1;
    }
    return 0;
}

int from_panman(const Options& o, const std::vector<int>& devices) {
    const int device = devices[0];
    const std::string path = o.get("input-panman");
    if (o.has("protobuf2capnp")) return protobuf2capnp(o);
    std::cout << "starting reading panman" << std::endl;
    const auto t0 = Clock::now();
    pm_panman* file = nullptr;
    char err[512] = {0};
    if (pm_panman_load(path.c_str(), &file, err, sizeof err) != PM_OK) {
        print_error(err[0] ? err : ("cannot load " + path));
        return 1;
    }
    std::cout << "Data load time: " << ns_since(t0) << " nanoseconds \n";
    ::mkdir("./info", 0777);
    const int trees = pm_panman_tree_count(file);
    const bool to_file = o.has("output-file");
    auto sink = [&](const char* ext, int i, const char* data, size_t n) -> bool {
        if (!to_file) {   // (stdio straight to fd 1: a 5 GB FASTA text through iostream costs seconds)
            std::cout.flush();
            return std::fwrite(data, 1, n, stdout) == n && std::fflush(stdout) == 0;
        }
        const std::string p = "./info/" + o.get("output-file") + "_" + std::to_string(i) + ext;
        std::ofstream f(p, std::ios::binary);
        f.write(data, (std::streamsize)n);
        return (bool)f;
    };
    int status = 0;
    if (o.has("reroot")) {   // src/panmanUtils.cpp:855-892, then writePanMAN
        status = reroot(o, file, device);
        pm_panman_free(file);
        return status;
    }
    if (o.has("impute")) {
        status = impute(o, file, device);
        pm_panman_free(file);
        return status;
    }
    if (o.has("subnet")) {
        status = subnet(o, file, device);
        pm_panman_free(file);
        return status;
    }
    if (o.has("maf")) {
        status = one_tree_text(o, file, device, ".maf", pm_maf_fd, "\nMAF execution time: ");
        pm_panman_free(file);
        return status;
    }
    if (o.has("gfa")) {
        status = one_tree_text(o, file, device, ".gfa", pm_gfa_fd, "GFA generation time: ");
        pm_panman_free(file);
        return status;
    }
    if (o.has("printMutations")) {
        status = print_mutations(o, file, device);
        pm_panman_free(file);
        return status;
    }
    if (o.has("toUsher")) {
        status = to_usher(o, file, device);
        pm_panman_free(file);
        return status;
    }
    if (o.has("aa-translation")) {
        status = aa_translation(o, file, device);
        pm_panman_free(file);
        return status;
    }
    if (o.has("summary")) {   // src/panmanUtils.cpp:356-384, Tree::printSummary (src/summary.cpp:257-273)
        pm_ctx* ctx = nullptr;
        if (pm_create(device, &ctx) != PM_OK) {
            print_error("no HIP device");
            pm_panman_free(file);
            return 1;
        }
        const auto s0 = Clock::now();
        for (int i = 0; i < trees && status == 0; ++i) {
            pm_panmat view;
            pm_summary sm;
            if (pm_panman_tree(file, i, &view) != PM_OK || pm_summary_compute(ctx, &view, &sm) != PM_OK) {
                print_error(pm_last_error(ctx));
                status = 1;
                break;
            }
            std::ostringstream out;
            out << "Total Nodes in Tree: " << sm.nodes << std::endl;
            out << "Total Samples in Tree: " << sm.samples << std::endl;
            out << "Total Substitutions: " << sm.substitutions << std::endl;
            out << "Total Insertions: " << sm.insertions << std::endl;
            out << "Total Deletions: " << sm.deletions << std::endl;
            out << "Total Inversions: " << sm.inversions << std::endl;
            out << "Max Tree Depth: " << sm.max_depth << std::endl;
            out << "Mean Tree Depth: " << sm.mean_depth << std::endl;
            const std::string text = out.str();
            if (!sink(".summary", i, text.data(), text.size())) status = 1;
            // getBlockMutationsParallel prints to std::cout whatever the output file (:203-250)
            std::cout << "Total Block Insertions: " << sm.block_insertions << std::endl;
            std::cout << "Total Block Deletions: " << sm.block_deletions << std::endl;
            std::cout << "Total Block Inversion: " << sm.block_inversions << std::endl;
            std::cout << "Total Block Duplications: " << sm.block_duplications << std::endl;
            std::cout << "Total Block Translocation: " << sm.block_translocations << std::endl;
        }
        std::cout << "\nSummary creation time: " << ns_since(s0) << " nanoseconds\n";
        pm_destroy(ctx);
    }
    if (o.has("newick")) {
        for (int i = 0; i < trees; ++i) {
            std::string s = pm_panman_newick(file, i);
            s += "\n";
            if (!sink(".newick", i, s.data(), s.size())) status = 1;
        }
    }
    for (int aligned = 0; aligned < 2 && status == 0; ++aligned) {
        if (!o.has(aligned ? "fasta-aligned" : "fasta")) continue;
        const auto f0 = Clock::now();
        for (int i = 0; i < trees && status == 0; ++i) {
            pm_panmat view;
            int64_t len = 0;
            char err[512] = {0};
            // the text streams from the device(s) straight to stdout or the output file
            // (pm_fasta_multi_fd): no host copy of the whole text, the write overlaps the download
            int fd = 1;
            if (to_file) {
                const std::string p = "./info/" + o.get("output-file") + "_" + std::to_string(i) + (aligned ? ".msa" : ".fasta");
                fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
                if (fd < 0) {
                    print_error("cannot write " + p);
                    status = 1;
                    break;
                }
            } else {
                std::cout.flush();
                std::fflush(stdout);
            }
            const auto w0 = Clock::now();
            if (pm_panman_tree(file, i, &view) != PM_OK ||
                pm_fasta_multi_fd(&view, aligned, devices.data(), (int)devices.size(), fd, &len, err, sizeof err) != PM_OK) {
                print_error(err[0] ? err : "FASTA extraction failed");
                status = 1;
            }
            if (to_file && ::close(fd) != 0) status = 1;
            cli_phase("cli.fasta_stream", w0);
            if (status) break;
        }
        std::cout << "\nFASTA execution time: " << ns_since(f0) << " nanoseconds\n";
    }
    pm_panman_free(file);
    return status;
}

int run(int argc, char** argv);

}  // namespace

// Builds whose tools write their results at exit always take the normal exit: sanitizers
// (LeakSanitizer's report) are detected; a coverage build (gcc defines no macro for
// --coverage) adds -DPM_CLI_NORMAL_EXIT.
#if defined(__SANITIZE_ADDRESS__) || defined(__SANITIZE_THREAD__) || defined(PM_CLI_NORMAL_EXIT)
constexpr bool kFastExitAllowed = false;
#elif defined(__has_feature)
#if __has_feature(address_sanitizer) || __has_feature(thread_sanitizer) || __has_feature(memory_sanitizer)
constexpr bool kFastExitAllowed = false;
#else
constexpr bool kFastExitAllowed = true;
#endif
#else
constexpr bool kFastExitAllowed = true;
#endif

// PANMAN_PHASES=1: the library's phase log (pm_phase_report: HIP init, parse, upload, GPU
// run, grouping, capnp, xz, download ...) and the CLI's own wall time, on stderr.
int main(int argc, char** argv) {
    pm_phase_reset();
    const auto t0 = Clock::now();
    const int rc = run(argc, argv);
    const char* ph = std::getenv("PANMAN_PHASES");
    if (ph && ph[0] == '1') {
        std::vector<char> buf((size_t)pm_phase_report(nullptr, 0));
        pm_phase_report(buf.data(), (int64_t)buf.size());
        std::cerr << "#phases\n" << buf.data() << "cli.total\t" << ns_since(t0) * 1e-9 << "\n";
    }
    // Every output file is closed and every context destroyed by now; what a normal exit adds
    // is the HIP / HSA runtime's own teardown in static destructors, which the kernel driver
    // does anyway when the process ends.  Skipped, unless a profiler whose results are written
    // at exit is preloaded, the build carries a sanitizer or coverage (kFastExitAllowed), or
    // PM_CLI_FULL_EXIT=1.
    const char* pre = std::getenv("LD_PRELOAD");
    const char* full = std::getenv("PM_CLI_FULL_EXIT");
    if (kFastExitAllowed && !(full && full[0] == '1') && !(pre && std::strstr(pre, "rocprof"))) {
        std::cout.flush();
        std::cerr.flush();
        std::fflush(nullptr);
        _exit(rc);
    }
    return rc;
}

namespace {

int run(int argc, char** argv) {
    Options o;
    std::string err;
    if (!parse(argc, argv, o, err)) {
        print_error(err);
        usage(std::cerr);
        return 1;
    }
    if (o.has("help") || argc == 1) {
        usage(std::cout);
        return 0;
    }
    if (o.has("backend") && o.get("backend") != "hip") {
        print_error("--backend " + o.get("backend") + ": this build computes on the GPU only (use --backend hip)");
        return 1;
    }
    const int device = o.has("device") ? std::atoi(o.get("device").c_str()) : 0;
    const int gpus = o.has("gpus") ? std::atoi(o.get("gpus").c_str()) : 1;
    if (gpus < 1 || gpus > 64) {
        print_error("--gpus must be between 1 and 64");
        return 1;
    }
    std::vector<int> devices;
    for (int g = 0; g < gpus; ++g) devices.push_back(device + g);
    // -I: HIP initialisation and the code objects' load (~0.1 s) on a thread of their own,
    // while this one reads and xz-decodes the PanMAN (C5: 0.3 s; measured 0.06-0.08 s off the
    // command).  Not for -M, whose input is parsed in ~10 ms: there the extra code-object
    // loads only delayed the build (PM_CLI_NO_WARMUP=1: never).
    struct Warm {
        std::thread t;
        ~Warm() {
            if (t.joinable()) t.join();
        }
    } warm;
    if (const char* nw = std::getenv("PM_CLI_NO_WARMUP");
        !(nw && nw[0] == '1') && o.has("input-panman") && !o.has("input-msa") && !o.has("input-pangraph") && !o.has("input-gfa"))
        warm.t = std::thread([device] { (void)pm_warmup(device); });
    if (o.has("input-gfa")) return build_from_gfa(o, device);
    if (o.has("input-pangraph")) return build_from_pangraph(o, device);
    if (o.has("input-msa")) return build_from_msa(o, devices);
    if (o.has("input-panman")) return from_panman(o, devices);
    print_error("no input: give -I <file.panman>, or -M <msa>, -P <pangraph.json> or -G <graph.gfa> with -N <newick>");
    usage(std::cerr);
    return 1;
}

}  // namespace
