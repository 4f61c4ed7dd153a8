// metafast_main.cpp -- metafast.sh-compatible command line driver for the MI355X hot path.
//
// Host-side mirror (C++; the image has no JDK) of the reference's tool shells for this path, on top of the C-ABI only
// (include/metafast_hip.h):
//   src/Runner.java:27-30 + itmo!/Runner.java:108-182          tool registry, -t/--tool, -ts/--tools, --version, default matrix-builder
//   itmo!/utils/tool/Tool.java:61-143, 212-214, 318-392        launch options (-w -p -c --force -s -f -v -h), <workDir>/<tool>/, SUCCESS
//   src/tools/KmersCounterMain.java, KmersCounterForManyFilesMain.java, SeqBuilderMain.java, SeqBuilderForManyFilesMain.java,
//   ComponentCutterMain.java, FeaturesCalculatorMain.java, DistanceMatrixCalculatorMain.java, DistanceMatrixBuilderMain.java
// Parameter names, defaults, output file names and the workDir layout are the reference's, and so is the
// step bookkeeping of the Tool framework (in.properties / out.properties / SUCCESS per step, -c/--force/-s/-f, the
// "rewrite them?" prompt, log + logs/log_<ts>, output_description.txt), so that a Java run can continue a workDir this
// program wrote and the other way round.  Errors: message on stderr, exit 1.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>
#include "../../include/metafast_hip.h"

// the group-comparison entry points are reached through weak references: a build of this driver against a library without them (the
// sanitizer build links a stub of the older entry points) still links, and the tools stop with a message
extern "C" int mf_stats_kmers(mf_ctx *, const char *const *, int, const char *const *, int, int, double, double, const char *, uint64_t *)
    __attribute__((weak));
extern "C" int mf_kmers_samples_count(mf_ctx *, const char *const *, int, int, int, const char *, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_unique_kmers_multi(mf_ctx *, const char *const *, int, const char *const *, int, int, int, int, int, const char *, int *, uint64_t *,
                                     uint64_t *) __attribute__((weak));
extern "C" int mf_kmers_multiple_filters(mf_ctx *, const char *const *, int, const char *const *, int, const char *const *, int, const char *const *, int,
                                         int, int, const char *const *, const char *const *, uint64_t *) __attribute__((weak));
extern "C" int mf_stats_kmers3(mf_ctx *, const char *const *, int, const char *const *, int, const char *const *, int, int, double, double, const char *,
                               uint64_t *) __attribute__((weak));
extern "C" int mf_specific_kmers(mf_ctx *, const char *const *, int, const char *const *, int, double, double, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_specific_kmers3(mf_ctx *, const char *const *, int, const char *const *, int, const char *const *, int, double, double, const char *,
                                  uint64_t *) __attribute__((weak));
extern "C" int mf_unique_kmers(mf_ctx *, const char *const *, int, const char *const *, int, int, int, const char *, const char *, uint64_t *, uint64_t *)
    __attribute__((weak));
extern "C" int mf_kmers_grouped_count(mf_ctx *, const char *const *, int, const char *const *, int, const char *const *, int, const char *const *, int, int,
                                      int, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_kmers_per_sample(mf_ctx *, const char *const *, int, int, int, int, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_kmers_color(mf_ctx *, const char *const *, const int *, int, int, int, int, const char *, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_colored_components(mf_ctx *, const char *const *, int, int, int64_t, int, int, double, const char *, const char *, uint64_t *)
    __attribute__((weak));
extern "C" int mf_comp2seq(mf_ctx *, const char *, int, int, const char *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_comp2graph(mf_ctx *, const char *, int, const char *const *, int, int, const char *, uint64_t *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_seq2comp(mf_ctx *, const char *const *, int, int, const char *, const char *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_paths_create(mf_ctx *, mf_comps *, const uint32_t *, uint64_t, int, uint64_t, mf_paths **) __attribute__((weak));
extern "C" int mf_paths_add(mf_paths *, const void *, const void *, uint64_t, uint64_t) __attribute__((weak));
extern "C" int mf_paths_finish(mf_paths *) __attribute__((weak));
extern "C" void mf_paths_destroy(mf_paths *) __attribute__((weak));
extern "C" int mf_paths_slots(const mf_paths *, uint32_t *, uint64_t *, uint64_t *, uint8_t *) __attribute__((weak));
extern "C" int mf_paths_write(const mf_paths *, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_paths_stats(const mf_paths *, uint64_t *, uint64_t *, uint64_t *, uint64_t *) __attribute__((weak));
// (component-paths drives the library step by step, to log as the reference does: these older entry points are weak for it too)
extern "C" int mf_comps_load(mf_ctx *, const char *, mf_comps **) __attribute__((weak));
extern "C" int mf_comps_set_k(mf_comps *, int) __attribute__((weak));
extern "C" int mf_comps_stats(const mf_comps *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" void mf_comps_destroy(mf_comps *) __attribute__((weak));
extern "C" int mf_reads_load(mf_ctx *, const char *const *, int, mf_reads **) __attribute__((weak));
extern "C" int mf_reads_stats(const mf_reads *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_reads_device_view(const mf_reads *, const void **, const void **) __attribute__((weak));
extern "C" void mf_reads_destroy(mf_reads *) __attribute__((weak));

// (the k = 32 ... 63 path behind --wide-kmers: weak for the same reason)
extern "C" int mf_count_reads_wide(mf_ctx *, const char *const *, int, int, int, mf_wtable **) __attribute__((weak));
extern "C" int mf_wtable_write_kmers(mf_wtable *, int, const char *, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_wtable_load_kmers(mf_ctx *, const char *const *, int, int, int, mf_wtable **) __attribute__((weak));
extern "C" int mf_wtable_stats(const mf_wtable *, uint64_t *, uint64_t *, int *) __attribute__((weak));
extern "C" int mf_wtable_export(const mf_wtable *, uint64_t *, uint64_t *, uint16_t *, uint64_t, uint64_t *) __attribute__((weak));
extern "C" void mf_wtable_destroy(mf_wtable *) __attribute__((weak));
extern "C" int mf_build_unitigs_wide_device(mf_ctx *, mf_wtable *, int, int, mf_seqs **) __attribute__((weak));
extern "C" int mf_seqs_write_fasta(const mf_seqs *, const char *) __attribute__((weak));
extern "C" int mf_seqs_stats(const mf_seqs *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" void mf_seqs_destroy(mf_seqs *) __attribute__((weak));
extern "C" int mf_cut_components_wide_device(mf_ctx *, mf_wtable *, int, int, mf_wcomps **) __attribute__((weak));
extern "C" int mf_wcomps_write(const mf_wcomps *, const char *, const char *) __attribute__((weak));
extern "C" int mf_wcomps_load(mf_ctx *, const char *, int, mf_wcomps **) __attribute__((weak));
extern "C" int mf_wcomps_stats(const mf_wcomps *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" void mf_wcomps_destroy(mf_wcomps *) __attribute__((weak));
extern "C" int mf_features_wide(mf_ctx *, const char *, const char *, int, int, const char *, const char *) __attribute__((weak));
extern "C" int mf_features_wide_selected(mf_ctx *, const char *, const char *, int, int, mf_wtable *, const char *, const char *) __attribute__((weak));
extern "C" int mf_features_reads_wide_selected(mf_ctx *, const char *, const char *const *, int, int, int, mf_wtable *, const char *, const char *) __attribute__((weak));
extern "C" int mf_comp2seq_wide(mf_ctx *, const char *, int, int, const char *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_seq2comp_wide(mf_ctx *, const char *const *, int, int, const char *, const char *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_comp2graph_wide(mf_ctx *, const char *, int, const char *const *, int, int, const char *, uint64_t *, uint64_t *, uint64_t *) __attribute__((weak));
extern "C" int mf_paths_create_wide(mf_ctx *, mf_wcomps *, const uint32_t *, uint64_t, int, uint64_t, mf_paths **) __attribute__((weak));
extern "C" int mf_unique_kmers_multi_wide(mf_ctx *, const char *const *, int, const char *const *, int, int, int, int, int, const char *, int *, uint64_t *, uint64_t *)
    __attribute__((weak));
extern "C" int mf_wtable_write_kmers_filtered(mf_wtable *, int, mf_wtable *, int, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_kmers_per_sample_wide(mf_ctx *, const char *const *, int, int, int, int, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_stats_kmers_wide(mf_ctx *, const char *const *, int, const char *const *, int, int, int, double, double, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_kmers_grouped_count_wide(mf_ctx *, const char *const *, int, const char *const *, int, const char *const *, int, const char *const *, int, int,
                                           int, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_kmers_color_wide(mf_ctx *, const char *const *, const int *, int, int, int, int, const char *, const char *, uint64_t *) __attribute__((weak));
extern "C" int mf_colored_components_wide(mf_ctx *, const char *const *, int, int, int64_t, int, int, double, const char *, const char *, uint64_t *)
    __attribute__((weak));

using std::string;
using std::vector;

// ------------------------------------------------------------------------------------------------ utilities
static bool g_verbose = false;
static FILE *g_logfile = nullptr, *g_logfile2 = nullptr;      // <workDir>/log and <workDir>/logs/log_<ts> (identical)
static std::mutex g_log_mutex;                                // (the per-device workers of a step log too)
static std::atomic<bool> g_workers_active{false};                         // other threads are inside library calls: die() must not run static destructors under them
static void logmsg(const char *level, const char *fmt, ...) {
    char buf[4096];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    std::lock_guard<std::mutex> lock(g_log_mutex);
    bool debug = !strcmp(level, "DEBUG");
    if (!debug || g_verbose) fprintf(stderr, "%s: %s\n", level, buf);
    if (g_logfile || g_logfile2) {                          // "%d{dd-MMM-yy  HH:mm:ss,SSS}  %-5p  %m%n" (Tool.java:700)
        struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts);
        struct tm tmv; localtime_r(&ts.tv_sec, &tmv);
        char d[64]; strftime(d, sizeof d, "%d-%b-%y  %H:%M:%S", &tmv);
        for (FILE *f : {g_logfile, g_logfile2}) if (f) { fprintf(f, "%s,%03ld  %-5s  %s\n", d, ts.tv_nsec / 1000000, level, buf); fflush(f); }
    }
}
[[noreturn]] static void die(const char *fmt, ...) {
    char buf[4096];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    logmsg("ERROR", "%s", buf);
    if (g_workers_active) { fflush(nullptr); _exit(1); }
    exit(1);                                            // Tool.java:450-463: ExecutionFailedException -> exit code 1
}
static void check(int rc) { if (rc < 0) die("%s", mf_last_error()); }
static bool exists(const string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }
static bool is_dir(const string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }
static void mkdirs(const string &p) {
    string cur;
    for (size_t i = 0; i <= p.size(); i++) {
        if (i == p.size() || p[i] == '/') { if (!cur.empty() && !is_dir(cur) && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST) die("can't create directory %s", cur.c_str()); }
        if (i < p.size()) cur.push_back(p[i]);
    }
}
static string basename_of(const string &p) { size_t s = p.find_last_of('/'); return s == string::npos ? p : p.substr(s + 1); }
static bool ends_with_ci(const string &s, const string &suf) {
    if (suf.size() > s.size()) return false;
    for (size_t i = 0; i < suf.size(); i++) if (tolower((unsigned char)s[s.size() - suf.size() + i]) != tolower((unsigned char)suf[i])) return false;
    return true;
}
// FileUtils.removeExtension (itmo!/utils/FileUtils.java:199-210): first matching extension only
static string remove_ext(const string &s, std::initializer_list<const char *> exts) {
    for (const char *e : exts) { string x = e[0] == '.' ? e : string(".") + e; if (ends_with_ci(s, x)) return s.substr(0, s.size() - x.size()); }
    return s;
}
// NamedSource.name(): FastaReader.java:22 / FastqReader.java:25
static string library_name(const string &path) {
    string b = basename_of(path);
    if (ends_with_ci(b, ".gz")) b = b.substr(0, b.size() - 3);          // FastaGZReader.java:17, FastqGZReader.java:21
    else if (ends_with_ci(b, ".bz2")) b = b.substr(0, b.size() - 4);    // FastaBZ2Reader.java:20
    if (ends_with_ci(b, ".binq")) return remove_ext(b, {".binq"});         // BinqReader.java:19
    if (ends_with_ci(b, ".fastq") || ends_with_ci(b, ".fq")) return remove_ext(b, {".fastq", ".fq"});
    return remove_ext(b, {".fasta", ".fa", ".fn", ".fna"});
}
static string timestamp() {                                 // Tool.java:664 "yyyy.MM.dd_HH.mm.ss"
    time_t t = time(nullptr); struct tm tmv; localtime_r(&t, &tmv);
    char b[64]; strftime(b, sizeof b, "%Y.%m.%d_%H.%M.%S", &tmv);
    return b;
}
static void mkparent(const string &path) { const size_t s = path.find_last_of('/'); if (s != string::npos) mkdirs(path.substr(0, s)); }
static string with_dt(string p, const string &ts) { const size_t q = p.find("$DT"); if (q != string::npos) p.replace(q, 3, ts); return p; }
static string percent_or_nan(uint64_t part, uint64_t whole) {       // Java's "%.1f" of part * 100.0 / whole: 0 / 0 prints NaN
    char b[64]; if (whole) snprintf(b, sizeof b, "%.1f", part * 100.0 / whole); else snprintf(b, sizeof b, "NaN");
    return b;
}
static void touch(const string &p) { FILE *f = fopen(p.c_str(), "w"); if (f) fclose(f); }
static string abspath(const string &p) {                    // File.getAbsolutePath: no normalisation
    if (!p.empty() && p[0] == '/') return p;
    char cwd[4096]; if (!getcwd(cwd, sizeof cwd)) return p;
    return string(cwd) + "/" + p;
}
static string group_digits(uint64_t v) {                    // NumUtils.groupDigits: 1'234'567
    string s = std::to_string(v), o;
    for (size_t i = 0; i < s.size(); i++) { o.push_back(s[i]); size_t r = s.size() - 1 - i; if (r && r % 3 == 0) o.push_back('\''); }
    return o;
}

// ------------------------------------------------------------------------------------------------ argument parsing
struct Args {
    std::map<string, vector<string>> opt;      // canonical long name -> values
    bool has(const string &k) const { return opt.count(k) > 0; }
    string get(const string &k, const string &def = "") const { auto it = opt.find(k); return it == opt.end() || it->second.empty() ? def : it->second[0]; }
    int geti(const string &k, int def) const {
        auto it = opt.find(k); if (it == opt.end() || it->second.empty()) return def;
        char *e; long v = strtol(it->second[0].c_str(), &e, 10); if (*e) die("Can't parse integer value '%s' of option --%s", it->second[0].c_str(), k.c_str());
        return (int)v;
    }
    double getd(const string &k, double def) const {
        auto it = opt.find(k); if (it == opt.end() || it->second.empty()) return def;
        char *e; double v = strtod(it->second[0].c_str(), &e); if (*e || it->second[0].empty()) die("Can't parse double value '%s' of option --%s", it->second[0].c_str(), k.c_str());
        return v;
    }
    bool flag(const string &k) const { return get(k, "false") == "true"; }
    vector<string> list(const string &k) const { auto it = opt.find(k); return it == opt.end() ? vector<string>() : it->second; }
};
// ------------------------------------------------------------------------------------------------ a tool, as the table at the end declares it
// (the reference's Tool with its Parameter fields, itmo!/utils/tool/Tool.java + Parameter.java): one row of TOOLS and one run function
enum Kind { VAL, FILE1, FILES, FLAG, LIST, DTFILE };      // plain value, file, list of files, boolean, list of plain values, file with $DT = the run's time stamp
struct Param { const char *name; Kind kind; const char *dflt; };          // dflt == nullptr: none, the parameter is null unless given; "$WD/x": x in the work directory
struct Short { const char *sht, *lng; };                                  // what an overloaded short option means for this tool, where OPTS' first match is not it
struct Need { const char *name, *sht; };                                  // a mandatory argument; sht == nullptr: the message names no short option
struct PV;
struct Run;
struct Tool {
    const char *name, *desc;
    vector<PV> (*run)(Run &);                                             // does the work, returns the entries of out.properties
    Short shorts[4]; Need needs[6]; Param params[18];                     // each ends at its first empty entry; params in the reference's declaration order
    const Param *param(const string &n) const { for (auto &p : params) if (p.name && n == p.name) return &p; return nullptr; }
};
static const Tool *find_tool(const string &name);
struct OptDef { const char *lng; const char *sht; bool multi; bool flag; };
// every option of the tools on the path (short names as in the reference; note --maximal-bad-frequence in the counters,
// KmersCounterMain.java:40, vs --maximal-bad-frequency elsewhere).  A short name that several options share means the FIRST of them
// unless the tool's row says otherwise.
static const OptDef OPTS[] = {
    {"tool", "t", false, false}, {"tools", "ts", false, true}, {"version", "", false, true}, {"work-dir", "w", false, false},
    {"available-processors", "p", false, false}, {"continue", "c", false, true}, {"force", "", false, true},
    {"start", "s", false, false}, {"finish", "f", false, false}, {"verbose", "v", false, true}, {"help", "h", false, true},
    {"help-all", "ha", false, true}, {"memory", "m", false, false},
    {"k", "k", false, false}, {"reads", "i", true, false}, {"k-mers", "i", true, false}, {"sequences", "i", true, false},
    {"maximal-bad-frequency", "b", false, false}, {"maximal-bad-frequence", "b", false, false},
    {"bottom-cut-percent", "bp", false, false}, {"min-seq-len", "l", false, false}, {"sequence-len", "l", false, false},
    {"output-dir", "o", false, false}, {"stats-dir", "", false, false},
    {"min-component-size", "b1", false, false}, {"max-component-size", "b2", false, false}, {"components-file", "cm", false, false},
    {"kmers", "ka", true, false}, {"selected", "", true, false}, {"threshold", "", false, false},
    {"features", "", true, false}, {"without-names", "wn", false, true}, {"matrix-file", "", false, false},
    {"output-format", "", false, false}, {"heatmap-file", "", false, false}, {"newMatrix-file", "", false, false},
    {"without-renumbering", "wr", false, true}, {"colors-file", "col", false, false}, {"invert-colors", "", false, true},
    {"kmers-file", "kf", false, false}, {"output-file", "o", false, false}, {"split", "", false, true}, {"long", "", false, true},
    {"use-reads-for-calculating-features", "", false, true}, {"device", "", false, false}, {"devices", "", false, false},
    {"positiveReads", "pos", true, false}, {"negativeReads", "neg", true, false}, {"filter-kmers", "", true, false}, {"max-thresh", "", false, false},
    {"a-kmers", "A", true, false}, {"b-kmers", "B", true, false}, {"p-value-chi2", "pchi2", false, false}, {"p-value-mw", "pmw", false, false},
    {"min-samples", "", false, false}, {"max-samples", "", false, false}, {"cd-filter-kmers", "cd", true, false}, {"uc-filter-kmers", "uc", true, false},
    {"nonibd-filter-kmers", "nonibd", true, false}, {"c-kmers", "C", true, false},
    {"cd-kmers", "cd", true, false}, {"uc-kmers", "uc", true, false}, {"nonibd-kmers", "nonibd", true, false},
    {"class", "", false, false}, {"val", "val", false, true}, {"n_groups", "group", false, false}, {"separate", "", false, true},
    {"linear", "", false, true}, {"n_comps", "comp", false, false}, {"perc", "", false, false}, {"percent-present", "", false, false},
    {"coverage", "cov", false, true}, {"graph-file", "", false, false},
    {"seq", "", true, false}, {"components", "", true, false}, {"all-components", "a", false, true}, {"min-length", "", false, false},
    {"wide-kmers", "", false, true},
};
static Args parse_args(int argc, char **argv, string *tool_out) {
    // first pass: find the tool (needed to resolve the overloaded short options)
    string tool = "matrix-builder";                                         // src/Runner.java:29
    for (int i = 1; i + 1 < argc; i++) if (!strcmp(argv[i], "-t") || !strcmp(argv[i], "--tool")) tool = argv[i + 1];
    *tool_out = tool;
    const Tool *row = find_tool(tool);
    auto long_of_short = [&](const string &s) -> string {
        if (row) for (auto &o : row->shorts) if (o.sht && s == o.sht) return o.lng;
        if (s == "cf") return "components-file";                           // ViewMain.java:45, BinaryToFasta.java:47
        for (auto &o : OPTS) if (o.sht[0] && s == o.sht) return o.lng;
        return "";
    };
    Args a;
    for (int i = 1; i < argc;) {
        string tok = argv[i];
        // launcher-level options handled by stub.sh in the reference (src/stub.sh:6-19): accepted and ignored
        if (tok == "-ea" || tok.rfind("-X", 0) == 0 || tok.rfind("-agentlib:", 0) == 0) { i++; continue; }
        string name;
        if (tok.rfind("--", 0) == 0) { name = tok.substr(2); if (name == "new-matrix-file") name = "newMatrix-file"; }
        else if (tok.size() > 1 && tok[0] == '-') name = long_of_short(tok.substr(1));
        else die("Unknown argument '%s'", tok.c_str());
        const OptDef *def = nullptr;
        for (auto &o : OPTS) if (name == o.lng) def = &o;
        if (!def) die("Unrecognized option: %s", tok.c_str());
        i++;
        auto &vals = a.opt[name];
        if (def->flag) {                                                    // booleans take an optional true/false (Parameter.java:51-58)
            if (i < argc && (!strcmp(argv[i], "true") || !strcmp(argv[i], "false"))) { vals.push_back(argv[i]); i++; }
            else vals.push_back("true");
            continue;
        }
        if (i >= argc) die("Missing argument for option: %s", tok.c_str());
        // (a list where the tool declares one: --kmers-file in kmers-grouped-counter, KmersGroupedSamplesCounter.java:38-42, one file in view and bin2fasta)
        const Param *decl = row ? row->param(name) : nullptr;
        if (def->multi || (decl && (decl->kind == FILES || decl->kind == LIST))) { while (i < argc && !(argv[i][0] == '-' && strlen(argv[i]) > 1 && !isdigit((unsigned char)argv[i][1]))) vals.push_back(argv[i++]); }
        else vals.push_back(argv[i++]);
    }
    return a;
}

// ------------------------------------------------------------------------------------------------ tools
// Devices.  The reference's drivers loop over all libraries in one process (KmersCounterForManyFilesMain.java:80-108,
// SeqBuilderForManyFilesMain.java:82-94, FeaturesCalculatorMain.java:137-162): here `--devices a,b,...` (default: every device the process
// sees; `--device n` = one) names the GPUs, every entry gets a context of its own, and the three per-library steps deal their libraries
// round-robin to one worker thread per entry (library i -> entry i mod D, in every step: what entry d wrote in kmer-counter-many is
// still in ITS HBM when seq-builder-many and features-calculator ask for the file, `file_cache`).  The steps need no exchange -- the
// files are the interchange --, component-cutter joins all libraries (ComponentCutterMain.java:78-114) on entry 0 from the .seq.fasta
// files.  An entry may name a device twice (--devices 0,0: two contexts, two streams on one GPU).
struct Env {
    vector<int> devs;                           // --devices
    vector<mf_ctx *> ctxs;                      // one per entry, made by the first thread that needs it
    string work_dir;
    bool cont = false;
    string start_ts;
};
static thread_local int t_slot = 0;             // the entry of Env::devs the calling thread works for
static void parse_devices(Env &e, const Args &a) {
    if (!e.devs.empty()) return;
    if (a.has("devices")) {
        const string v = a.get("devices");
        size_t i = 0;
        while (i <= v.size()) {
            size_t j = v.find(',', i); if (j == string::npos) j = v.size();
            const string tok = v.substr(i, j - i);
            char *end = nullptr; const long d = strtol(tok.c_str(), &end, 10);
            if (tok.empty() || *end || d < 0) die("Can't parse --devices '%s' (a comma-separated list of device numbers)", v.c_str());
            e.devs.push_back((int)d);
            i = j + 1;
        }
    } else if (a.has("device")) e.devs.push_back(a.geti("device", 0));
    else {
        const int n = std::max(1, mf_device_count());
        for (int d = 0; d < n; d++) e.devs.push_back(d);
        // Two contexts per device where the libraries are small next to its memory: while one library's files are read and written (the page
        // cache takes 9 GB/s, a sample's .kmers.bin is as large as a third of its reads) the device counts the other one's.  A library needs
        // about 8 x its read file in HBM at the peak of its count (reads + two record buffers + lists + table + index); two of the largest
        // must fit in 0.8 of the device.  MF_CONTEXTS_PER_DEVICE=1 (or an explicit --devices / --device) switches it off.
        size_t largest = 0, nlib = 0;
        for (const char *opt : {"reads", "k-mers", "kmers"})
            for (auto &f : a.list(opt)) {
                struct stat st;
                if (stat(f.c_str(), &st) != 0) continue;
                const size_t packed = ends_with_ci(f, ".gz") || ends_with_ci(f, ".bz2") ? 5 : 1;      // (compressed reads: about five times their size once inflated)
                largest = std::max(largest, (size_t)st.st_size * packed); nlib++;
            }
        const char *cpd = getenv("MF_CONTEXTS_PER_DEVICE");
        uint64_t hbm = 0;
        bool two = cpd ? atoi(cpd) >= 2 : false;
        if (!cpd && nlib >= 2 * (size_t)n && mf_device_memory(0, &hbm) == MF_OK && hbm > 0 && (double)largest * 8.0 * 2.0 < 0.8 * (double)hbm) two = true;
        if (two) for (int d = 0; d < n; d++) e.devs.push_back(d);
    }
    e.ctxs.assign(e.devs.size(), nullptr);
}
static mf_ctx *ctx_of(Env &e, const Args &a) {
    parse_devices(e, a);
    mf_ctx *&ctx = e.ctxs[(size_t)t_slot];
    if (!ctx) {
        // (-p/--available-processors: the host-side parsers' threads, shared out over the entries that work side by side)
        const int procs = a.geti("available-processors", (int)sysconf(_SC_NPROCESSORS_ONLN));
        check(mf_ctx_create(e.devs[(size_t)t_slot], std::max(1, procs / (int)e.devs.size()), &ctx));
        // the steps of one run hand their results on through the reference's files; what a step has just written stays in HBM for the
        // step that loads it next (a quarter of the device's memory at most -- shared out over the entries that name the same device;
        // MF_FILE_CACHE=0 switches it off)
        const char *fc = getenv("MF_FILE_CACHE");
        int same = 0; for (int d : e.devs) same += d == e.devs[(size_t)t_slot];
        check(mf_ctx_set_option(ctx, "file_cache", fc ? atoll(fc) : -(int64_t)same));
        if (const char *mo = getenv("MF_OPTIONS")) {                      // library options for A/B runs: MF_OPTIONS=name=value,name=value
            string all(mo); size_t i = 0;
            while (i < all.size()) {
                size_t j = all.find(',', i); if (j == string::npos) j = all.size();
                const string kv = all.substr(i, j - i); const size_t q = kv.find('=');
                if (q != string::npos) check(mf_ctx_set_option(ctx, kv.substr(0, q).c_str(), atoll(kv.c_str() + q + 1)));
                i = j + 1;
            }
        }
    }
    return ctx;
}
// a per-library step: item i is done by the worker of entry i mod D (entry 0 = the calling thread)
static void for_each_library(Env &e, const Args &a, size_t n, const std::function<void(size_t)> &fn) {
    parse_devices(e, a);
    const size_t D = std::min(e.devs.size(), n);
    if (D <= 1) { for (size_t i = 0; i < n; i++) fn(i); return; }
    logmsg("DEBUG", "%zu libraries on %zu device contexts", n, D);
    g_workers_active = true;
    vector<std::thread> th;
    for (size_t d = 1; d < D; d++)
        th.emplace_back([&, d]() {
            t_slot = (int)d;
            if (e.ctxs[d]) check(mf_ctx_bind_thread(e.ctxs[d]));           // (made by the worker of an earlier step: HIP's device is per thread)
            for (size_t i = d; i < n; i += D) fn(i);
            if (e.ctxs[d]) mf_ctx_synchronize(e.ctxs[d]);
        });
    for (size_t i = 0; i < n; i += D) fn(i);
    for (auto &t : th) t.join();
    g_workers_active = false;
}
static vector<const char *> cptrs(const vector<string> &v) { vector<const char *> p; for (auto &s : v) p.push_back(s.c_str()); return p; }
static void check_k(int k) {                                                 // KmersCounterMain.java:66-73
    if (k <= 0) die("The size of k-mer must be at least 1.");
    if (k > 31) die("The size of k-mer must be no more than 31.");
}
// --wide-kmers (a launch option of this driver; the reference has none): the tools from files to the matrix take 32 <= k <= 63 on 2k-bit
// k-mers -- wide .kmers.bin / components.bin files, everything else as for k <= 31.  With k <= 31 the flag changes nothing,
// and every other tool keeps check_k.  true: this run is wide (k has been checked); false: the caller goes on as ever, check_k first.
static bool g_wide = false;
static bool wide_k(int k) {
    if (!g_wide || k <= 31) return false;
    if (k > 63) die("The size of k-mer must be no more than 63.");
    if (!mf_count_reads_wide || !mf_wtable_write_kmers || !mf_wtable_load_kmers || !mf_wcomps_write || !mf_features_wide || !mf_seqs_write_fasta)
        die("--wide-kmers: this build of the library has no file level for k > 31 (mf_count_reads_wide ...)");
    return true;
}
// view and bin2fasta read wide files on the host and call no library function: wide without a look at the library's symbols
// (comp2graph and seq2comp call ONE entry point each -- on wide files somebody else wrote, or writing them itself -- and report it by name themselves)
static bool wide_host_k(int k) {
    if (!g_wide || k <= 31) return false;
    if (k > 63) die("The size of k-mer must be no more than 63.");
    return true;
}
static void no_wide(bool given, const char *option) {
    if (given) die("Option --%s is not supported with --wide-kmers and k > 31", option);
}

// kmer-counter (src/tools/KmersCounterMain.java:65-137)
static string run_kmer_counter(Env &e, const Args &a, const vector<string> &files, int k, int b, const string &out_dir, const string &stats_dir) {
    const bool wide = wide_k(k);
    if (!wide) check_k(k);
    if (files.empty()) die("Mandatory option --reads is not set");
    mf_ctx *ctx = ctx_of(e, a);
    for (auto &f : files) logmsg("INFO", "Loading file %s...", basename_of(f).c_str());
    mf_table *t = nullptr;
    mf_wtable *wt = nullptr;
    auto fp = cptrs(files);
    // loadReads + printKmers(hm, b, ...) (KmersCounterMain.java:77-99): only the entries with value > b are handed on, so the
    // cut is made inside the counting kernels and the uncut table (> 2^32 entries for a large sample) never exists; the
    // .stat.txt histogram still covers every counted k-mer (the table remembers what the cut dropped)
    uint64_t size = 0;
    // (wide: the count is uncut -- a wide table does not remember what a cut drops, and .stat.txt lists it --, the writer makes the cut)
    if (wide) { check(mf_count_reads_wide(ctx, fp.data(), (int)fp.size(), k, 0, &wt)); check(mf_wtable_stats(wt, &size, nullptr, nullptr)); }
    else check(mf_count_reads_above(ctx, fp.data(), (int)fp.size(), k, 0, b, &t, &size));
    mkdirs(out_dir); mkdirs(stats_dir);
    string name;                                                             // getName :122-137
    if (files.size() == 2) {
        string n1 = library_name(files[0]), n2 = library_name(files[1]);
        auto ends = [](const string &s, const char *x) { return s.size() >= 3 && s.compare(s.size() - 3, 3, x) == 0; };
        if ((ends(n1, "_r1") && ends(n2, "_r2")) || (ends(n1, "_R1") && ends(n2, "_R2"))) name = n1.substr(0, n1.size() - 3);
        else name = n1 + "+";
    } else name = library_name(files[0]) + (files.size() > 1 ? "+" : "");
    string out = out_dir + "/" + name + ".kmers.bin", st = stats_dir + "/" + name + ".stat.txt";
    uint64_t good = 0;
    if (wide) check(mf_wtable_write_kmers(wt, b, out.c_str(), st.c_str(), &good));
    else check(mf_table_write_kmers(t, b, out.c_str(), st.c_str(), &good));
    logmsg("INFO", "%s k-mers found, %s (%.1f%%) of them is good (not erroneous)", group_digits(size).c_str(), group_digits(good).c_str(),
           size ? good * 100.0 / size : 0.0);
    if (size == 0) logmsg("WARN", "No k-mers found in reads! Perhaps you reads file is empty or k-mer size is too big");
    else if (good == 0 || good < (uint64_t)(size * 0.03)) logmsg("WARN", "Too few good k-mers were found! Perhaps you should decrease k-mer size or --maximal-bad-frequency value");
    logmsg("INFO", "Good k-mers printed to %s", out.c_str());
    if (wide) mf_wtable_destroy(wt); else mf_table_destroy(t);
    return out;
}
// kmer-counter-many (src/tools/KmersCounterForManyFilesMain.java:66-108): sort, pair _r1/_r2, one counter per sample
static vector<string> run_kmer_counter_many(Env &e, const Args &a, vector<string> files, int k, int b, const string &wd, const string &out_dir, const string &stats_dir) {
    if (files.empty()) die("Mandatory option --reads is not set");
    std::sort(files.begin(), files.end());
    mkdirs(wd + "/sub-counter");
    auto ends = [](const string &s, const char *x) { return s.size() >= 3 && s.compare(s.size() - 3, 3, x) == 0; };
    vector<vector<string>> libs;                                             // :80-108, one entry per library
    for (size_t i = 0; i < files.size();) {
        string n = library_name(files[i]);
        bool pair = i + 1 < files.size() && ((ends(n, "_r1") && ends(library_name(files[i + 1]), "_r2")) || (ends(n, "_R1") && ends(library_name(files[i + 1]), "_R2")));
        libs.emplace_back(files.begin() + i, files.begin() + i + (pair ? 2 : 1));
        i += pair ? 2 : 1;
    }
    vector<string> outs(libs.size());
    for_each_library(e, a, libs.size(), [&](size_t i) { outs[i] = run_kmer_counter(e, a, libs[i], k, b, out_dir, stats_dir); });
    return outs;
}
// seq-builder (src/tools/SeqBuilderMain.java:78-160)
static string run_seq_builder(Env &e, const Args &a, const vector<string> &files, int k, int b, int bp, int l, const string &wd, const string &out_dir,
                              bool write_distribution = true) {
    if (files.empty()) die("Mandatory option --k-mers is not set");
    mf_ctx *ctx = ctx_of(e, a);
    mf_table *t = nullptr;
    mf_wtable *wt = nullptr;
    const bool wide = wide_k(k);
    auto fp = cptrs(files);
    // (wide: a table loaded from files is ascending, whatever order the count that wrote them left -- the unitigs are a function of the files)
    if (wide) check(mf_wtable_load_kmers(ctx, fp.data(), (int)fp.size(), b, k, &wt));
    else check(mf_table_load_kmers(ctx, fp.data(), (int)fp.size(), b, k, &t));
    vector<uint16_t> wcnts;                                                  // wide: the counts of the table, for -bp and the distribution file
    if (wide && (bp >= 0 || write_distribution)) {
        uint64_t n = 0; check(mf_wtable_export(wt, nullptr, nullptr, nullptr, 0, &n));
        wcnts.resize(n);
        if (n) check(mf_wtable_export(wt, nullptr, nullptr, wcnts.data(), n, &n));
    }
    if (bp >= 0) {                                                           // bottom-cut-percent :103-115
        uint64_t n = 0; if (!wide) check(mf_table_export(t, -1, nullptr, nullptr, 0, &n));
        vector<uint64_t> keys(n); vector<uint16_t> cnts(n);
        if (n) check(mf_table_export(t, -1, keys.data(), cnts.data(), n, &n));
        if (wide) cnts.swap(wcnts);
        vector<uint64_t> stat(1024, 0); uint64_t total = 0;
        for (uint16_t c : cnts) { total += c; stat[c >= 1024 ? 1023 : c]++; }
        uint64_t to_cut = total * (uint64_t)bp / 100, cur = 0;
        logmsg("INFO", "Using bottom cut percent = %d", bp);
        for (int i = 0; i < 1023; i++) { if (cur >= to_cut) { b = i; break; } cur += (uint64_t)i * stat[i]; }
    }
    logmsg("INFO", "Using maximal bad frequency = %d", b);
    mkdirs(wd); mkdirs(out_dir);
    string base = remove_ext(basename_of(files[0]), {".kmers.bin"});
    string fasta = out_dir + "/" + base + (files.size() > 1 ? "+" : "") + ".seq.fasta";
    string distr = wd + "/distribution";
    uint64_t nseq = 0;
    if (wide) {
        if (write_distribution) {                                            // stat[min(value, 1023)]++, lines "i stat[i]" (SeqBuilderMain.java:84-98, 170-176)
            if (bp >= 0) { uint64_t n = 0; check(mf_wtable_export(wt, nullptr, nullptr, nullptr, 0, &n)); wcnts.resize(n); if (n) check(mf_wtable_export(wt, nullptr, nullptr, wcnts.data(), n, &n)); }
            vector<uint64_t> stat(1024, 0);
            for (uint16_t c : wcnts) stat[c >= 1024 ? 1023 : c]++;
            FILE *f = fopen(distr.c_str(), "w");
            if (!f) die("can't write '%s'", distr.c_str());
            for (int i = 1; i < 1024; i++) fprintf(f, "%d %llu\n", i, (unsigned long long)stat[i]);
            fclose(f);
        }
        mf_seqs *sq = nullptr;
        check(mf_build_unitigs_wide_device(ctx, wt, b, l, &sq));
        check(mf_seqs_write_fasta(sq, fasta.c_str()));
        check(mf_seqs_stats(sq, &nseq, nullptr));
        mf_seqs_destroy(sq);
    } else check(mf_build_unitigs(ctx, t, k, b, l, fasta.c_str(), write_distribution ? distr.c_str() : nullptr, &nseq));
    logmsg("INFO", "%s sequences found", group_digits(nseq).c_str());
    if (nseq == 0) logmsg("WARN", "No sequences were found! Perhaps you should decrease --min-seq-len or --maximal-bad-frequency values");
    logmsg("INFO", "Sequences printed to %s", fasta.c_str());
    if (wide) mf_wtable_destroy(wt); else mf_table_destroy(t);
    return fasta;
}
// seq-builder-many (src/tools/SeqBuilderForManyFilesMain.java:82-94): one seq-builder per k-mers file, all in <wd>/sub-builder.  Every one of
// them writes sub-builder/distribution (SeqBuilderMain.java:98), so the file a run leaves behind is the LAST library's; with several
// device contexts at work only that one writes it.
static vector<string> run_seq_builder_many(Env &e, const Args &a, const vector<string> &kmers, int k, int b, int bp, int l, const string &wd, const string &out_dir) {
    vector<string> fs(kmers.size());
    parse_devices(e, a);
    const bool par = std::min(e.devs.size(), kmers.size()) > 1;
    for_each_library(e, a, kmers.size(), [&](size_t i) { fs[i] = run_seq_builder(e, a, {kmers[i]}, k, b, bp, l, wd + "/sub-builder", out_dir, !par || i + 1 == kmers.size()); });
    return fs;
}
// component-cutter (src/tools/ComponentCutterMain.java:78-114)
// ... with several device contexts (round 6): every entry reads the .seq.fasta files of ITS libraries (library i -> entry i mod W, as in the
// per-library steps: the device that built them), the entries cut the components together -- every entry owns a shard of the cutter table,
// the exchanges run inside the library over a communicator of this process's threads (mf_comm_create_local: slices copied straight into the
// peers' buffers, over xGMI between devices) -- and entry 0 writes components.bin; every entry keeps the components for the features of
// its libraries.  W = the largest power of two <= the entries; MF_REPLICATED_CUTTER=1, k < 20 or a single entry: entry 0 alone, as before.
// Returns false when the entries gave up together (the caller then takes entry 0 alone).
static bool run_component_cutter_sharded(Env &e, const Args &a, const vector<string> &files, int k, int l, int b1, int b2, const string &comp_file, const string &stat, uint64_t *nc) {
    parse_devices(e, a);
    size_t W = 1;
    while (2 * W <= e.devs.size() && 2 * W <= 64) W *= 2;
    if (W < 2 || k < 20 || getenv("MF_REPLICATED_CUTTER")) return false;
    // (entries that share ONE device gain nothing from shards -- two contexts on a GPU: 0.17 s against 0.13 on the benchmark's two libraries --:
    // the cutter is sharded when the entries name at least two devices; MF_SHARDED_CUTTER=1 shards whatever they name: tests on a one-GPU box)
    { bool two = false; for (size_t d = 1; d < W; d++) two |= e.devs[d] != e.devs[0]; if (!two && !getenv("MF_SHARDED_CUTTER")) return false; }
    const int keep_slot = t_slot;
    for (size_t d = 0; d < W; d++) { t_slot = (int)d; ctx_of(e, a); }           // (a context is made by whoever needs it first; its worker binds it below)
    t_slot = keep_slot;
    vector<mf_comm *> comms(W, nullptr);
    check(mf_comm_create_local(e.ctxs.data(), (int)W, comms.data()));
    logmsg("DEBUG", "Cutting components on %zu device contexts (sharded cutter table)", W);
    vector<int> rcs(W, MF_OK); vector<string> errs(W); vector<uint64_t> ncs(W, 0);
    auto work = [&](size_t d) {
        vector<string> mine;
        for (size_t i = d; i < files.size(); i += W) mine.push_back(files[i]);
        auto fp = cptrs(mine);
        rcs[d] = mf_cut_components_sharded_files(comms[d], fp.data(), (int)fp.size(), k, l, b1, b2, comp_file.c_str(), stat.c_str(), &ncs[d]);
        if (rcs[d] < 0) errs[d] = mf_last_error();
    };
    g_workers_active = true;
    vector<std::thread> th;
    for (size_t d = 1; d < W; d++) th.emplace_back([&, d]() { t_slot = (int)d; if (mf_ctx_bind_thread(e.ctxs[d]) < 0) { rcs[d] = MF_ERR; errs[d] = mf_last_error(); } work(d); mf_ctx_synchronize(e.ctxs[d]); });
    work(0);
    for (auto &t : th) t.join();
    g_workers_active = false;
    for (mf_comm *c : comms) mf_comm_destroy(c);
    for (size_t d = 0; d < W; d++)
        if (rcs[d] < 0) {
            if (rcs[d] == MF_ERR_TOGETHER) continue;
            die("%s", errs[d].c_str());                                          // (a file that cannot be read, ...: the reference's message)
        }
    for (size_t d = 0; d < W; d++) if (rcs[d] == MF_ERR_TOGETHER) { logmsg("WARN", "%s -- cutting the components on one device", errs[d].c_str()); return false; }
    *nc = ncs[0];
    return true;
}
static string run_component_cutter(Env &e, const Args &a, const vector<string> &files, int k, int l, int b1, int b2, const string &wd, const string &comp_file) {
    if (files.empty()) die("Mandatory option --sequences is not set");
    if (wide_k(k)) {
        // the wide cutter is replicated: whatever --devices names, this step runs on entry 0 (the per-library steps spread as ever)
        parse_devices(e, a);
        if (e.devs.size() > 1) logmsg("DEBUG", "Cutting components on one device context (the cutter for k > 31 is not sharded)");
        mf_ctx *ctx = ctx_of(e, a);
        auto fp = cptrs(files);
        logmsg("DEBUG", "Loading sequences from files...");
        mf_wtable *wt = nullptr;
        check(mf_count_reads_wide(ctx, fp.data(), (int)fp.size(), k, l, &wt));
        uint64_t size = 0; check(mf_wtable_stats(wt, &size, nullptr, nullptr));
        if (size == 0) die("No sequences were found in input files! The following steps will be useless");
        logmsg("INFO", "Searching for components...");
        mkdirs(wd); mkparent(comp_file);
        mf_wcomps *wc = nullptr;
        check(mf_cut_components_wide_device(ctx, wt, b1, b2, &wc));
        check(mf_wcomps_write(wc, comp_file.c_str(), (wd + "/components-stat-" + std::to_string(b1) + "-" + std::to_string(b2) + ".txt").c_str()));
        uint64_t nc = 0; check(mf_wcomps_stats(wc, &nc, nullptr));
        logmsg("INFO", "Total %s components were found", group_digits(nc).c_str());
        if (nc == 0) logmsg("WARN", "No components were extracted! Perhaps you should decrease --min-component-size value");
        logmsg("INFO", "Components saved to %s", comp_file.c_str());
        mf_wcomps_destroy(wc); mf_wtable_destroy(wt);
        return comp_file;
    }
    {
        mkdirs(wd);
        const string stat = wd + "/components-stat-" + std::to_string(b1) + "-" + std::to_string(b2) + ".txt";
        uint64_t nc = 0;
        logmsg("DEBUG", "Loading sequences from files...");
        if (run_component_cutter_sharded(e, a, files, k, l, b1, b2, comp_file, stat, &nc) && nc > 0) {
            // (no component at all: the run below repeats the step on one device and says what the reference says -- "No sequences were found" or
            // "No components were extracted" --, a case of toy inputs)
            logmsg("INFO", "Searching for components...");
            logmsg("INFO", "Total %s components were found", group_digits(nc).c_str());
            logmsg("INFO", "Components saved to %s", comp_file.c_str());
            return comp_file;
        }
    }
    mf_ctx *ctx = ctx_of(e, a);
    mf_table *t = nullptr;
    auto fp = cptrs(files);
    logmsg("DEBUG", "Loading sequences from files...");
    check(mf_count_reads(ctx, fp.data(), (int)fp.size(), k, l, &t));
    uint64_t size = 0; check(mf_table_stats(t, &size, nullptr));
    if (size == 0) die("No sequences were found in input files! The following steps will be useless");
    logmsg("INFO", "Searching for components...");
    mkdirs(wd);
    string stat = wd + "/components-stat-" + std::to_string(b1) + "-" + std::to_string(b2) + ".txt";
    uint64_t nc = 0;
    check(mf_cut_components(ctx, t, k, b1, b2, comp_file.c_str(), stat.c_str(), &nc));
    logmsg("INFO", "Total %s components were found", group_digits(nc).c_str());
    if (nc == 0) logmsg("WARN", "No components were extracted! Perhaps you should decrease --min-component-size value");
    logmsg("INFO", "Components saved to %s", comp_file.c_str());
    mf_table_destroy(t);
    return comp_file;
}
// features-calculator (src/tools/FeaturesCalculatorMain.java:77-167): reads files and k-mers files, with or without --selected
// (--wide-kmers and k > 31: the same three inputs on a wide components.bin and wide .kmers.bin files, mf_wfeatures.hip; matrix-builder keeps its
// refusal of --selected and --use-reads-for-calculating-features above k = 31 and never comes here with them)
static vector<string> run_features(Env &e, const Args &a, const string &comp_file, const vector<string> &reads, const vector<string> &kmers,
                                   int k, int thr, const string &wd, bool single_tool = false) {
    if (comp_file.empty()) die("Mandatory option --components-file is not set");
    if (kmers.empty() && reads.empty()) die("No input files: pass reads (-i) or k-mers files (-ka)");
    const bool wide = wide_k(k);
    if (!wide && single_tool) check_k(k);                                    // (the builder has checked its k)
    if (wide && (!reads.empty() || !a.list("selected").empty())) {
        if (!mf_features_reads_wide_selected) die("features-calculator: this build of the library has no mf_features_reads_wide_selected");
        if (!mf_features_wide_selected) die("features-calculator: this build of the library has no mf_features_wide_selected");
    }
    parse_devices(e, a);
    string out_dir = wd + "/vectors";
    mkdirs(out_dir);
    // --selected (FeaturesCalculatorMain.java:55-57, 113-116): selected = IOUtils.loadKmers(selectedKmers, 0, ...), one table per device context
    const vector<string> sel_files = a.list("selected");
    vector<mf_table *> sel(e.devs.size(), nullptr);
    auto selected = [&]() -> mf_table * {
        if (sel_files.empty()) return nullptr;
        mf_table *&t = sel[(size_t)t_slot];
        if (!t) { auto fp = cptrs(sel_files); check(mf_table_load_kmers(ctx_of(e, a), fp.data(), (int)fp.size(), 0, k, &t)); }
        return t;
    };
    vector<mf_wtable *> wsel(e.devs.size(), nullptr);                         // (the same for wide files)
    auto wselected = [&]() -> mf_wtable * {
        if (sel_files.empty()) return nullptr;
        mf_wtable *&t = wsel[(size_t)t_slot];
        if (!t) { auto fp = cptrs(sel_files); check(mf_wtable_load_kmers(ctx_of(e, a), fp.data(), (int)fp.size(), 0, k, &t)); }
        return t;
    };
    // reads files first, one vector per FILE, then k-mers files (FeaturesCalculatorMain.java:117-162)
    vector<string> vecs(reads.size() + kmers.size());
    for_each_library(e, a, vecs.size(), [&](size_t i) {
        mf_ctx *ctx = ctx_of(e, a);
        if (i < reads.size()) {
            const string &rf = reads[i];
            string base = library_name(rf);
            string vec = out_dir + "/" + base + ".vec", br = out_dir + "/" + base + ".breadth";
            const char *fs[1] = {rf.c_str()};
            if (wide) check(mf_features_reads_wide_selected(ctx, comp_file.c_str(), fs, 1, k, thr, wselected(), vec.c_str(), br.c_str()));
            else check(mf_features_reads_selected(ctx, comp_file.c_str(), fs, 1, k, thr, selected(), vec.c_str(), br.c_str()));
            logmsg("INFO", "Features for file %s printed to %s", basename_of(rf).c_str(), vec.c_str());
            vecs[i] = vec;
        } else {
            const string &kf = kmers[i - reads.size()];
            string base = remove_ext(basename_of(kf), {".kmers.bin"});
            string vec = out_dir + "/" + base + ".vec", br = out_dir + "/" + base + ".breadth";
            if (wide && sel_files.empty()) check(mf_features_wide(ctx, comp_file.c_str(), kf.c_str(), k, thr, vec.c_str(), br.c_str()));
            else if (wide) check(mf_features_wide_selected(ctx, comp_file.c_str(), kf.c_str(), k, thr, wselected(), vec.c_str(), br.c_str()));
            else check(mf_features_selected(ctx, comp_file.c_str(), kf.c_str(), k, thr, selected(), vec.c_str(), br.c_str()));
            logmsg("INFO", "Features for file %s printed to %s", basename_of(kf).c_str(), vec.c_str());
            vecs[i] = vec;
        }
    });
    for (mf_table *t : sel) if (t) mf_table_destroy(t);
    for (mf_wtable *t : wsel) if (t) mf_wtable_destroy(t);
    return vecs;
}
// Double.toString (what Java's "%s" prints for a double): shortest digits that round-trip, decimal notation in [1e-3, 1e7)
static string java_double(double d) {
    if (std::isnan(d)) return "NaN";
    if (std::isinf(d)) return d > 0 ? "Infinity" : "-Infinity";
    if (d == 0) return std::signbit(d) ? "-0.0" : "0.0";
    char buf[64];
    for (int prec = 1; prec <= 17; prec++) { snprintf(buf, sizeof buf, "%.*e", prec - 1, d); if (strtod(buf, nullptr) == d) break; }
    string s(buf);
    bool neg = s[0] == '-';
    if (neg) s = s.substr(1);
    size_t epos = s.find('e');
    int ex = atoi(s.c_str() + epos + 1);
    string digits;
    for (char ch : s.substr(0, epos)) if (ch != '.') digits.push_back(ch);
    string out;
    double ad = std::fabs(d);
    if (ad >= 1e-3 && ad < 1e7) {
        if (ex >= 0) {
            string ip = digits.substr(0, std::min<size_t>(digits.size(), (size_t)ex + 1));
            while ((int)ip.size() < ex + 1) ip.push_back('0');
            out = ip + "." + (digits.size() > (size_t)ex + 1 ? digits.substr(ex + 1) : string("0"));
        } else out = "0." + string((size_t)(-ex - 1), '0') + digits;
    } else out = digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : string("0")) + "E" + std::to_string(ex);
    return neg ? "-" + out : out;
}
// one matrix cell in a Java format string (PrintWriter.printf(format, double), DistanceMatrixCalculatorMain.java:112-116):
// "%s" -> Double.toString, "%[flags][width][.prec]{f,e,g}" -> printf; anything else is refused
static string format_cell(const string &fmt, double v) {
    if (fmt == "%s") return java_double(v);
    size_t i = 0;
    bool ok = fmt.size() >= 2 && fmt[0] == '%';
    for (i = 1; ok && i + 1 < fmt.size(); i++) if (!strchr("0123456789.+- ", fmt[i])) ok = false;
    if (!ok || !strchr("feg", fmt[fmt.size() - 1])) die("Unsupported --output-format '%s' (use %%s or %%[.N]f / e / g)", fmt.c_str());
    char buf[128]; snprintf(buf, sizeof buf, fmt.c_str(), v);
    return buf;
}
// DistanceMatrixCalculatorMain.printMatrix (:91-123): perm == nullptr prints the original order
static void print_matrix(const vector<double> &m, int n, const string &path, const vector<string> *names, const int *perm, const string &fmt) {
    mkparent(path);
    FILE *out = fopen(path.c_str(), "w");
    if (!out) die("Failed to print matrix to %s", path.c_str());
    if (names) { fprintf(out, "#"); for (int i = 0; i < n; i++) fprintf(out, "\t%s", (*names)[perm ? perm[i] : i].c_str()); fprintf(out, "\n"); }
    for (int i = 0; i < n; i++) {
        if (names) fprintf(out, "%s\t", (*names)[perm ? perm[i] : i].c_str());
        for (int j = 0; j < n; j++) {
            if (j) fprintf(out, "\t");
            fprintf(out, "%s", format_cell(fmt, perm ? m[(size_t)perm[i] * n + perm[j]] : m[(size_t)i * n + j]).c_str());
        }
        fprintf(out, "\n");
    }
    fclose(out);
}
// heatmap-maker, the numeric half (src/tools/HeatMapMakerMain.java:93-145): average-linkage clustering of the samples
// (FullHeatMap.clusterObjects :221-296: O(n^3), the FIRST closest pair in row-major order is merged, the merged node stays
// at the smaller index with the old node on the left) and the matrix renumbered in the dendrogram's leaf order
// (renumber :327-337).  The image itself is not rendered.
struct HNode { int no = -1, left = -1, right = -1; };
static void hm_group(const vector<HNode> &t, int node, vector<int> &out) {
    if (node < 0) return;
    if (t[node].no >= 0) { out.push_back(t[node].no); return; }
    hm_group(t, t[node].left, out); hm_group(t, t[node].right, out);
}
static vector<int> heatmap_order(const vector<double> &m, int n) {
    vector<HNode> t(n);
    vector<int> nodes(n);
    for (int i = 0; i < n; i++) { t[i].no = i; nodes[i] = i; }
    vector<double> dist((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) dist[(size_t)i * n + j] = m[(size_t)i * n + j] / 1 / 1;
    auto between = [&](const vector<int> &g1, const vector<int> &g2) {
        if (g1.empty() || g2.empty()) return -1.0;
        double sum = 0;
        for (int a : g1) for (int b : g2) sum += m[(size_t)a * n + b];
        return sum / (double)g1.size() / (double)g2.size();
    };
    int count = n, root = n > 0 ? 0 : -1;
    while (count > 1) {
        double best = 1.7976931348623157e308; int bi = -1, bj = -1;
        for (int i = 0; i < n; i++) for (int j = i + 1; j < n; j++)
            if (nodes[i] >= 0 && nodes[j] >= 0 && dist[(size_t)i * n + j] < best) { best = dist[(size_t)i * n + j]; bi = i; bj = j; }
        if (bi < 0 || best < 0) die("Internal error. Wrong minDist index.");
        HNode r; r.left = nodes[bi]; r.right = nodes[bj];
        t.push_back(r); root = (int)t.size() - 1;
        nodes[bi] = root; nodes[bj] = -1;
        vector<int> g1; hm_group(t, root, g1);
        for (int i = 0; i < n; i++) {
            dist[(size_t)i * n + bj] = dist[(size_t)bj * n + i] = -1;
            if (i != bi) { vector<int> g2; hm_group(t, nodes[i], g2); dist[(size_t)i * n + bi] = dist[(size_t)bi * n + i] = between(g1, g2); }
        }
        count--;
    }
    vector<int> perm;
    hm_group(t, root, perm);
    return perm;
}
static string run_heatmap_maker(Env &e, const string &matrix_path, const string &new_matrix_tpl, bool without_renumbering, const string &fmt) {
    FILE *fp = fopen(matrix_path.c_str(), "r");
    if (!fp) die("Can't read matrix file %s", matrix_path.c_str());
    vector<vector<string>> rows; char *line = nullptr; size_t cap = 0;
    while (getline(&line, &cap, fp) > 0) {
        vector<string> cells; string cur;
        for (char *q = line; *q && *q != '\n' && *q != '\r'; q++) { if (*q == '\t') { if (!cur.empty()) cells.push_back(cur); cur.clear(); } else cur.push_back(*q); }
        if (!cur.empty()) cells.push_back(cur);
        rows.push_back(cells);
    }
    free(line); fclose(fp);
    if (rows.empty()) die("No data to read in matrix file %s", matrix_path.c_str());
    const size_t fn = rows[0].size();
    if (fn > rows.size()) die("Can't parse matrix, columns' number > rows' number");
    for (size_t i = 0; i < fn; i++) if (rows[i].size() != fn) die("Can't parse matrix, columns' number is different for different rows");
    for (size_t i = fn; i < rows.size(); i++)                                                                                // HeatMapMakerMain.java:204-209 (white space is no token)
        for (auto &cell : rows[i]) if (cell.find_first_not_of(" \t\f") != string::npos) die("Can't parse matrix, too much rows");
    // (an empty first line: the reference indexes dataArray[0][0] of a 0 x 0 array there, :214 -- an exception, i.e. a failed run)
    if (fn == 0) die("Can't parse matrix, the first line of %s is empty", matrix_path.c_str());
    const bool with_names = rows[0][0] == "#";
    const int n = (int)fn - (with_names ? 1 : 0);
    vector<string> names;
    vector<double> m((size_t)n * n);
    for (int i = 0; i < n; i++) {
        if (with_names) names.push_back(rows[0][i + 1]);
        for (int j = 0; j < n; j++) {
            const string &cell = rows[i + (with_names ? 1 : 0)][j + (with_names ? 1 : 0)];
            char *end; m[(size_t)i * n + j] = strtod(cell.c_str(), &end);
            if (*end) die("Can't parse matrix, '%s' is not a number", cell.c_str());
        }
    }
    if (without_renumbering) return matrix_path;
    vector<int> perm = heatmap_order(m, n);
    const string path = with_dt(new_matrix_tpl.empty() ? remove_ext(matrix_path, {".txt"}) + "_renumbered.txt" : new_matrix_tpl, e.start_ts);
    print_matrix(m, n, path, with_names ? &names : nullptr, perm.data(), fmt);
    logmsg("INFO", "Renumbered matrix saved to %s", path.c_str());
    return path;
}

// ---- view / bin2fasta: text dumps of the binary files (src/tools/ViewMain.java:64-131, src/tools/BinaryToFasta.java:74-170).
// Host-only.  The reference prints the k-mers of a .kmers.bin in its hash map's iteration order; here: file order.
static string kmer_string(uint64_t km, int k) {             // ShortKmer.toString (itmo!/dna/kmers/ShortKmer.java:153-160)
    string s((size_t)k, 'A');
    for (int i = 0; i < k; i++) s[(size_t)i] = "AGCT"[(km >> (2 * (k - 1 - i))) & 3u];
    return s;
}
static uint64_t be_read(const unsigned char *p, int n) { uint64_t v = 0; for (int i = 0; i < n; i++) v = (v << 8) | p[i]; return v; }
static vector<unsigned char> slurp(const string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die("Can't read file %s", path.c_str());
    vector<unsigned char> b; unsigned char buf[1 << 16]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}
struct HostComp { int64_t weight; vector<uint64_t> kmers; };
static vector<HostComp> read_components(const string &path) {       // ConnectedComponent.loadComponents :95-122
    vector<unsigned char> b = slurp(path);
    if (b.size() < 4) die("Can't load components from %s", path.c_str());
    size_t pos = 0; uint64_t n = be_read(&b[0], 4); pos = 4;
    // (every component has its 12-byte header at least: a count the file cannot hold is a wrong file, not 2^32 empty components to
    // allocate for -- found by the sanitizer build, tests/test_host_sanitized_cpu.py)
    if (4 + 12 * n > b.size()) die("Can't load components from %s", path.c_str());
    vector<HostComp> cs((size_t)n);
    for (auto &cp : cs) {
        if (pos + 12 > b.size()) die("Can't load components from %s", path.c_str());
        uint64_t sz = be_read(&b[pos], 4); cp.weight = (int64_t)be_read(&b[pos + 4], 8); pos += 12;
        if (pos + 8 * sz > b.size()) die("Can't load components from %s", path.c_str());
        cp.kmers.resize((size_t)sz);
        for (auto &km : cp.kmers) { km = be_read(&b[pos], 8); pos += 8; }
    }
    return cs;
}
// ... and of the wide files behind --wide-kmers: 18-byte records, two words per member.  A headerless file of the wrong width is
// the mistake a user makes here: a size that is no whole number of wide records, or member lists that run past the end, is an error
static string kmer_string(uint64_t hi, uint64_t lo, int k) {
    string s((size_t)k, 'A');
    for (int i = 0; i < k; i++) { const int sh = 2 * (k - 1 - i); s[(size_t)i] = "AGCT"[(sh >= 64 ? hi >> (sh - 64) : lo >> sh) & 3u]; }
    return s;
}
static vector<unsigned char> slurp_wide_kmers(const string &path, int k) {
    vector<unsigned char> b = slurp(path);
    if (b.size() % 18) die("Can't read wide k-mers file %s: size %zu is not a multiple of the 18-byte record (k = %d; is this a file of another k?)", path.c_str(), b.size(), k);
    return b;
}
struct WideComp { int64_t weight; vector<std::pair<uint64_t, uint64_t>> kmers; };
static vector<WideComp> read_components_wide(const string &path, int k) {
    vector<unsigned char> b = slurp(path);
    if (b.size() < 4) die("Can't load wide components from %s: %zu bytes is not a components file", path.c_str(), b.size());
    size_t pos = 4; const uint64_t n = be_read(&b[0], 4);
    if (4 + 12 * n > b.size()) die("Can't load wide components from %s: %llu components, more than the file holds (k = %d; is this a file of another k?)", path.c_str(), (unsigned long long)n, k);
    vector<WideComp> cs((size_t)n);
    for (size_t i = 0; i < cs.size(); i++) {
        if (pos + 12 > b.size()) die("Can't load wide components from %s: the file ends inside the header of component %zu (k = %d; is this a file of another k?)", path.c_str(), i + 1, k);
        const uint64_t sz = be_read(&b[pos], 4); cs[i].weight = (int64_t)be_read(&b[pos + 4], 8); pos += 12;
        if (16 * sz > b.size() - pos) die("Can't load wide components from %s: component %zu has size %llu, more than the file holds (k = %d; is this a file of another k?)", path.c_str(), i + 1, (unsigned long long)sz, k);
        cs[i].kmers.resize((size_t)sz);
        for (auto &km : cs[i].kmers) { km.first = be_read(&b[pos], 8); km.second = be_read(&b[pos + 8], 8); pos += 16; }
    }
    if (pos != b.size()) die("Can't load wide components from %s: %zu bytes after the last component (k = %d; is this a file of another k?)", path.c_str(), b.size() - pos, k);
    return cs;
}
static FILE *open_out(const string &path) { if (path.empty()) return stdout; FILE *f = fopen(path.c_str(), "w"); if (!f) die("Couldn't open output file"); return f; }
static void close_out(FILE *f) { if (f != stdout) fclose(f); else fflush(f); }
static void run_view(const Args &a, int k) {
    const string kf = a.get("kmers-file"), cf = a.get("components-file");
    if (kf.empty() && cf.empty()) { logmsg("WARN", "No input file is selected  --->  no data to display!"); return; }
    const bool wide = wide_host_k(k);
    if (wide) no_wide(a.flag("long"), "long");
    FILE *out = open_out(a.get("output-file"));
    if (wide && !kf.empty()) {
        vector<unsigned char> b = slurp_wide_kmers(kf, k);
        fprintf(out, "Kmer\tCount\n");
        for (size_t p = 0; p < b.size(); p += 18) fprintf(out, "%s\t%lld\n", kmer_string(be_read(&b[p], 8), be_read(&b[p + 8], 8), k).c_str(), (long long)(int16_t)be_read(&b[p + 16], 2));
    }
    if (wide && !cf.empty()) {
        vector<WideComp> cs = read_components_wide(cf, k);
        logmsg("INFO", "%zu components loaded from %s", cs.size(), cf.c_str());
        fprintf(out, "%zu components:\n", cs.size());
        for (size_t i = 0; i < cs.size(); i++) {
            fprintf(out, "Component %zu, size = %zu kmers, weight = %lld. Kmers:\n", i + 1, cs[i].kmers.size(), (long long)cs[i].weight);
            for (auto &km : cs[i].kmers) fprintf(out, "%s\n", kmer_string(km.first, km.second, k).c_str());
            fprintf(out, "\n");
        }
    }
    if (wide) { close_out(out); return; }
    if (!kf.empty()) {
        const int rec = a.flag("long") ? 16 : 10;          // IOUtils.loadLongKmers / loadKmers
        vector<unsigned char> b = slurp(kf);
        fprintf(out, "Kmer\tCount\n");
        for (size_t p = 0; p + rec <= b.size(); p += rec)
            fprintf(out, "%s\t%lld\n", kmer_string(be_read(&b[p], 8), k).c_str(), rec == 10 ? (long long)(int16_t)be_read(&b[p + 8], 2) : (long long)be_read(&b[p + 8], 8));
    }
    if (!cf.empty()) {
        vector<HostComp> cs = read_components(cf);
        logmsg("INFO", "%zu components loaded from %s", cs.size(), cf.c_str());
        fprintf(out, "%zu components:\n", cs.size());
        for (size_t i = 0; i < cs.size(); i++) {
            fprintf(out, "Component %zu, size = %zu kmers, weight = %lld. Kmers:\n", i + 1, cs[i].kmers.size(), (long long)cs[i].weight);
            for (uint64_t km : cs[i].kmers) fprintf(out, "%s\n", kmer_string(km, k).c_str());
            fprintf(out, "\n");
        }
    }
    close_out(out);
}
static void run_bin2fasta(const Args &a, int k) {
    const string kf = a.get("kmers-file"), cf = a.get("components-file"), prefix = a.get("output-file");
    if (kf.empty() && cf.empty()) { logmsg("WARN", "No input file is selected  --->  no data to display!"); return; }
    if (!prefix.empty()) mkparent(prefix);
    if (wide_host_k(k)) {
        if (!kf.empty()) {
            vector<unsigned char> b = slurp_wide_kmers(kf, k);
            FILE *out = open_out(prefix.empty() ? "" : prefix + ".fasta");
            for (size_t p = 0, i = 1; p < b.size(); p += 18, i++) fprintf(out, ">%zu\n%s\n", i, kmer_string(be_read(&b[p], 8), be_read(&b[p + 8], 8), k).c_str());
            close_out(out);
        }
        if (!cf.empty()) {
            vector<WideComp> cs = read_components_wide(cf, k);
            logmsg("INFO", "%zu components loaded from %s", cs.size(), cf.c_str());
            const bool split = a.flag("split");
            FILE *out = split ? nullptr : open_out(prefix.empty() ? "" : prefix + ".fasta");
            for (size_t i = 0; i < cs.size(); i++) {
                if (split) out = open_out(prefix.empty() ? "" : prefix + "_" + std::to_string(i + 1) + ".fasta");
                size_t j = 1;
                for (auto &km : cs[i].kmers) {
                    if (split) fprintf(out, ">%zu\n", j++); else fprintf(out, ">%zu_%zu\n", i + 1, j++);
                    fprintf(out, "%s\n", kmer_string(km.first, km.second, k).c_str());
                }
                if (split) close_out(out);
            }
            if (!split) close_out(out);
        }
        return;
    }
    if (!kf.empty()) {
        FILE *out = open_out(prefix.empty() ? "" : prefix + ".fasta");
        vector<unsigned char> b = slurp(kf);
        size_t i = 1;
        for (size_t p = 0; p + 10 <= b.size(); p += 10, i++) fprintf(out, ">%zu\n%s\n", i, kmer_string(be_read(&b[p], 8), k).c_str());
        close_out(out);
    }
    if (!cf.empty()) {
        vector<HostComp> cs = read_components(cf);
        logmsg("INFO", "%zu components loaded from %s", cs.size(), cf.c_str());
        if (a.flag("split")) {
            for (size_t i = 0; i < cs.size(); i++) {
                FILE *out = open_out(prefix.empty() ? "" : prefix + "_" + std::to_string(i + 1) + ".fasta");
                size_t j = 1;
                for (uint64_t km : cs[i].kmers) fprintf(out, ">%zu\n%s\n", j++, kmer_string(km, k).c_str());
                close_out(out);
            }
        } else {
            FILE *out = open_out(prefix.empty() ? "" : prefix + ".fasta");
            for (size_t i = 0; i < cs.size(); i++) { size_t j = 1; for (uint64_t km : cs[i].kmers) fprintf(out, ">%zu_%zu\n%s\n", i + 1, j++, kmer_string(km, k).c_str()); }
            close_out(out);
        }
    }
}

// dist-matrix-calculator (src/tools/DistanceMatrixCalculatorMain.java:51-123)
static string run_dist_matrix(Env &e, const vector<string> &features, const string &matrix_path_tpl, bool without_names, const string &fmt) {
    if (features.empty()) die("Mandatory option --features is not set");
    vector<vector<int64_t>> vs;
    for (auto &f : features) {
        FILE *fp = fopen(f.c_str(), "r");
        if (!fp) die("Failed to read features from %s", f.c_str());
        vector<int64_t> v; char line[256];
        while (fgets(line, sizeof line, fp)) { if (line[0] != '\n' && line[0] != 0) v.push_back((int64_t)strtod(line, nullptr)); }
        fclose(fp);
        vs.push_back(v);
    }
    size_t nc = vs[0].size();
    for (auto &v : vs) if (v.size() != nc) die("feature files have different numbers of components");
    vector<int64_t> flat; for (auto &v : vs) flat.insert(flat.end(), v.begin(), v.end());
    int ns = (int)vs.size();
    vector<double> m((size_t)ns * ns, 0.0);
    check(mf_bray_curtis(flat.data(), ns, (int)nc, m.data()));
    const string path = with_dt(matrix_path_tpl, e.start_ts);
    vector<string> names;
    for (auto &f : features) names.push_back(remove_ext(basename_of(f), {"vec"}));
    print_matrix(m, ns, path, without_names ? nullptr : &names, nullptr, fmt);
    logmsg("INFO", "Distance matrix printed to %s", path.c_str());
    return path;
}

// ------------------------------------------------------------------------------------------------ step bookkeeping
// Tool.runAsStep (itmo!/utils/tool/Tool.java:318-392) and its property files (:740-960): every tool run, top level or sub-step,
// owns a directory with in.properties (its input parameters, written before it runs), out.properties (its output
// parameters) and SUCCESS.  A finished step is re-used by --continue iff in.properties and SUCCESS exist and every stored
// input equals the current one.  PropertiesConfiguration.save with delimiter parsing disabled: "key = value", one line
// per value of a multi-valued key, null parameters left out, files as absolute paths (Tool.objectToString :950-966).
struct PV {
    string name; vector<string> vals; bool set = true;                       // set == false: null, not written
    PV(string n, vector<string> v) : name(std::move(n)), vals(std::move(v)) {}
    PV(string n, const string &v) : name(std::move(n)), vals{v} {}
    PV(string n, int v) : name(std::move(n)), vals{std::to_string(v)} {}
    static PV null(string n) { PV p(std::move(n), vector<string>()); p.set = false; return p; }
    static PV file(string n, const string &v) { return v.empty() ? null(std::move(n)) : PV(std::move(n), abspath(v)); }
    static PV files(string n, const vector<string> &v) { vector<string> o; for (auto &x : v) o.push_back(abspath(x)); return PV(std::move(n), o); }
    static PV flag(string n, bool v) { return PV(std::move(n), string(v ? "true" : "false")); }
};
typedef std::map<string, vector<string>> Props;
static void props_write(const string &path, const vector<PV> &ps) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("Can't dump configuration to %s", path.c_str());
    for (auto &p : ps) if (p.set) for (auto &v : p.vals) {
        string esc; for (char c : v) { if (c == '\\') esc += "\\\\"; else esc.push_back(c); }
        fprintf(f, "%s = %s\n", p.name.c_str(), esc.c_str());
    }
    fclose(f);
}
static bool props_read(const string &path, Props &out) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return false;
    char *line = nullptr; size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        string l(line); while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
        size_t i = 0; while (i < l.size() && isspace((unsigned char)l[i])) i++;
        if (i == l.size() || l[i] == '#' || l[i] == '!') continue;
        size_t ke = i; while (ke < l.size() && l[ke] != '=' && l[ke] != ':' && !isspace((unsigned char)l[ke])) ke++;
        string key = l.substr(i, ke - i);
        size_t v = ke; while (v < l.size() && isspace((unsigned char)l[v])) v++;
        if (v < l.size() && (l[v] == '=' || l[v] == ':')) { v++; while (v < l.size() && isspace((unsigned char)l[v])) v++; }
        string val; for (size_t j = v; j < l.size(); j++) { if (l[j] == '\\' && j + 1 < l.size()) j++; val.push_back(l[j]); }
        out[key].push_back(val);
    }
    free(line); fclose(f);
    return true;
}
static bool props_equal(const vector<PV> &cur, const Props &stored) {      // (null and an empty list both leave no line)
    for (auto &p : cur) {
        auto it = stored.find(p.name);
        const vector<string> none, &now = p.set ? p.vals : none, &then = it == stored.end() ? none : it->second;
        if (now != then) { logmsg("DEBUG", "Parameter %s changed from last run", p.name.c_str()); return false; }
    }
    return true;
}
static vector<string> props_list(const Props &p, const string &k) { auto it = p.find(k); return it == p.end() ? vector<string>() : it->second; }
// one sub-step of a composite tool (Tool.runAllSteps :485-529): `force` turns true once a step has run, so everything
// after it runs too.  run() does the work and returns the output parameters; load() takes them from out.properties.
template <class RUN, class LOAD>
static void run_as_step(const string &name, const string &dir, const vector<PV> &in, const string &start, bool &force, RUN run, LOAD load) {
    if (name == start) force = true;
    mkdirs(dir);
    const string inp = dir + "/in.properties", outp = dir + "/out.properties", succ = dir + "/SUCCESS";
    const bool f = force || !exists(inp);
    bool can = exists(inp) && exists(succ);
    if (!f && can) { Props stored; can = props_read(inp, stored) && props_equal(in, stored); }
    if (!f && can) {
        logmsg("INFO", "SUCCESS file found for tool %s - loading results...", name.c_str());
        Props out; props_read(outp, out);
        load(out);
        return;
    }
    logmsg("DEBUG", "Running tool %s", name.c_str());
    unlink(succ.c_str()); unlink(outp.c_str());
    props_write(inp, in);
    const vector<PV> out = run();
    props_write(outp, out);
    touch(succ);
    force = true;
}
// output_description.txt in the current directory and in the workDir (DistanceMatrixBuilderMain.java:81-83, 178-200;
// IOUtils.tryToAppendDescription src/io/IOUtils.java:217-231)
static vector<string> g_desc_files;
static void describe(const string &path, const char *msg) {
    for (auto &d : g_desc_files) { FILE *f = fopen(d.c_str(), "a"); if (!f) continue; fprintf(f, "\n%s\n   %s\n", path.c_str(), msg); fclose(f); }
}
// input parameters of a tool as in.properties lists them: the row's declaration, values = what the run will use (defaults filled in)
static string param_default(const Param &p, const string &wd) { string d = p.dflt ? p.dflt : ""; if (d.rfind("$WD", 0) == 0) d.replace(0, 3, wd); return d; }
static vector<PV> tool_inputs(const Tool &t, const Args &a, const string &wd, const string &ts) {
    vector<PV> v;
    for (auto &p : t.params) {
        if (!p.name) break;
        const string n = p.name, d = param_default(p, wd);
        switch (p.kind) {
            case VAL: v.push_back(a.has(n) || p.dflt ? PV(n, a.get(n, d)) : PV::null(n)); break;
            case FILE1: v.push_back(PV::file(n, a.get(n, d))); break;
            case DTFILE: v.push_back(PV::file(n, with_dt(a.get(n, d), ts))); break;
            case FILES: v.push_back(PV::files(n, a.list(n))); break;
            case LIST: v.push_back(PV(n, a.list(n))); break;
            case FLAG: v.push_back(PV::flag(n, a.flag(n))); break;
        }
    }
    return v;
}
// what a run function sees: the launch, and the tool's parameters -- given on the command line, else taken from last run's in.properties
// under --continue (main), else the default its row declares
struct Run {
    Env &e; const Args &a; const Tool &t; const string wd, start, finish; bool force; int k;
    string dflt(const char *n, const Tool *of = nullptr, const string *dir = nullptr) const { const Param *p = (of ? of : &t)->param(n); return p ? param_default(*p, dir ? *dir : wd) : string(); }
    string str(const char *n) const { return a.get(n, dflt(n)); }
    int num(const char *n) const { const string d = dflt(n); return a.geti(n, d.empty() ? -1 : atoi(d.c_str())); }      // (-1: not given and no default)
    double real(const char *n) const { return a.getd(n, atof(dflt(n).c_str())); }
    mf_ctx *ctx() { return ctx_of(e, a); }
    void entry(bool present, const char *fn) const { if (!present) die("%s: this build of the library has no %s", t.name, fn); }
};
// the default that another tool's row declares, in that tool's work directory `dir`: what a sub-step runs with
static string sub_default(const Run &r, const char *tool, const char *n, const string &dir) { return r.dflt(n, find_tool(tool), &dir); }
static string cutter_stat(const string &wd, int b1, int b2) { return wd + "/components-stat-" + std::to_string(b1) + "-" + std::to_string(b2) + ".txt"; }

// ------------------------------------------------------------------------------------------------ the tools' run functions
static vector<PV> tool_kmer_counter(Run &r) {
    return {PV::file("resulting-kmers-file", run_kmer_counter(r.e, r.a, r.a.list("reads"), r.k, r.num("maximal-bad-frequence"), r.str("output-dir"), r.str("stats-dir")))};
}
static vector<PV> tool_kmer_counter_many(Run &r) {
    if (!wide_k(r.k)) check_k(r.k);
    return {PV::files("resulting-kmers-files", run_kmer_counter_many(r.e, r.a, r.a.list("reads"), r.k, r.num("maximal-bad-frequence"), r.wd, r.str("output-dir"), r.str("stats-dir")))};
}
// seq-builder-many declares no default for -b (it may not be given next to -bp) and hands a null on: seq-builder's own default applies
static vector<PV> tool_seq_builder(Run &r) {
    const bool many = !strcmp(r.t.name, "seq-builder-many");
    if (many && r.a.has("maximal-bad-frequency") && r.a.has("bottom-cut-percent")) die("-b and -bp can not be set both");
    const int b = r.a.geti("maximal-bad-frequency", atoi(r.dflt("maximal-bad-frequency", find_tool("seq-builder")).c_str()));
    const int bp = r.num("bottom-cut-percent"), l = r.num("sequence-len");
    if (!many) return {PV::file("output-file", run_seq_builder(r.e, r.a, r.a.list("k-mers"), r.k, b, bp, l, r.wd, r.str("output-dir")))};
    return {PV::files("output-files", run_seq_builder_many(r.e, r.a, r.a.list("k-mers"), r.k, b, bp, l, r.wd, r.str("output-dir")))};
}
static vector<PV> tool_component_cutter(Run &r) {
    const int b1 = r.num("min-component-size"), b2 = r.num("max-component-size");
    const string cf = run_component_cutter(r.e, r.a, r.a.list("sequences"), r.k, r.num("min-seq-len"), b1, b2, r.wd, r.str("components-file"));
    return {PV::file("components-file", cf), PV::file("components-stat", cutter_stat(r.wd, b1, b2))};
}
static vector<PV> tool_features(Run &r) {
    return {PV::files("features-files", run_features(r.e, r.a, r.str("components-file"), r.a.list("reads"), r.a.list("kmers"), r.k, r.num("threshold"), r.wd, true)),
            PV::file("features-dir", r.wd + "/vectors")};
}
static vector<PV> tool_dist_matrix(Run &r) {
    run_dist_matrix(r.e, r.a.list("features"), r.str("matrix-file"), r.a.flag("without-names"), r.str("output-format"));
    return {};
}
static vector<PV> tool_posneg(Run &r) {
    // KmersCounterPositiveNegative.java:66-108: two kmer-counter-many steps with the work directories <workDir>/pos and /neg
    const int k = r.k;
    vector<string> pos = r.a.list("positiveReads"), neg = r.a.list("negativeReads");
    logmsg("INFO", "Found %zu samples in positive class and %zu samples in negative class to process", pos.size(), neg.size());
    if (pos.empty() || neg.empty()) die("No libraries to process!!! Can't continue the calculations.");
    if (!wide_k(k)) check_k(k);                                            // (--wide-kmers and k > 31: run_kmer_counter_many counts wide, the files are wide .kmers.bin)
    const int b = r.num("maximal-bad-frequency");
    vector<string> kp, kn;
    for (int side = 0; side < 2; side++) {                                 // (each step with the counter's own defaults in ITS work directory)
        const string d = r.wd + (side ? "/neg" : "/pos"), od = sub_default(r, "kmer-counter-many", "output-dir", d), sd = sub_default(r, "kmer-counter-many", "stats-dir", d);
        const vector<string> &files = side ? neg : pos;
        vector<string> &res = side ? kn : kp;
        run_as_step("kmer-counter-many", d, {PV("k", k), PV::files("reads", files), PV("maximal-bad-frequence", b), PV::file("output-dir", od), PV::file("stats-dir", sd)},
                    r.start, r.force,
                    [&]() { res = run_kmer_counter_many(r.e, r.a, files, k, b, d, od, sd); return vector<PV>{PV::files("resulting-kmers-files", res)}; },
                    [&](const Props &o) { res = props_list(o, "resulting-kmers-files"); });
    }
    return {PV::files("resulting-pos-kmers-files", kp), PV::files("resulting-neg-kmers-files", kn)};
}
static vector<PV> tool_kmers_filter(Run &r) {
    // KmersFilter.java:80-121: every input k-mers file is written again with the records whose k-mer is frequent enough
    // in the filter files (IOUtils.filterAndPrintKmers, src/io/IOUtils.java:101-123)
    // (--wide-kmers and k > 31: the same on wide .kmers.bin files, mf_wtable_write_kmers_filtered)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    if (wide) r.entry(mf_wtable_write_kmers_filtered && mf_wtable_load_kmers && mf_wtable_stats && mf_wtable_destroy, "mf_wtable_write_kmers_filtered");
    const int b = r.num("maximal-bad-frequence"), mt = r.num("max-thresh");
    const string out_dir = r.str("output-dir");
    mkdirs(out_dir);
    mf_ctx *ctx = r.ctx();
    const vector<string> ff = r.a.list("filter-kmers");
    auto fp = cptrs(ff);
    mf_table *filter = nullptr;
    mf_wtable *wfilter = nullptr;
    check(wide ? mf_wtable_load_kmers(ctx, fp.data(), (int)fp.size(), b, k, &wfilter) : mf_table_load_kmers(ctx, fp.data(), (int)fp.size(), b, k, &filter));
    vector<string> written;
    for (auto &f : r.a.list("k-mers")) {
        mf_table *t = nullptr;
        mf_wtable *wt = nullptr;
        const char *one[1] = {f.c_str()};
        check(wide ? mf_wtable_load_kmers(ctx, one, 1, b, k, &wt) : mf_table_load_kmers(ctx, one, 1, b, k, &t));
        string name = basename_of(f);
        for (size_t q; (q = name.find(".kmers.bin")) != string::npos;) name.erase(q, 10);        // replaceAll(".kmers.bin", "")
        const string out = out_dir + "/" + name + ".kmers.bin";
        uint64_t c = 0, size = 0;
        if (wide) {
            check(mf_wtable_write_kmers_filtered(wt, b, wfilter, mt * (int)ff.size(), out.c_str(), &c));
            check(mf_wtable_stats(wt, &size, nullptr, nullptr));
        } else {
            check(mf_table_write_kmers_filtered(t, b, filter, mt * (int)ff.size(), out.c_str(), &c));
            check(mf_table_stats(t, &size, nullptr));
        }
        logmsg("INFO", "%s k-mers found, %s (%.1f%%) of them survived after filtering", group_digits(size).c_str(), group_digits(c).c_str(),
               size ? c * 100.0 / size : 0.0);
        logmsg("INFO", "Filtered k-mers printed to %s", out.c_str());
        if (wide) mf_wtable_destroy(wt); else mf_table_destroy(t);
        written.push_back(out);
    }
    if (wide) mf_wtable_destroy(wfilter); else mf_table_destroy(filter);
    return {written.empty() ? PV::null("resulting-kmers-file") : PV::file("resulting-kmers-file", written.back())};
}
static vector<PV> tool_kmers_samples_counter(Run &r) {
    // KmersSamplesCounter.java:69-140: the number of input files that hold each k-mer with a count > b
    const int k = r.k;
    check_k(k);
    const int b = r.num("maximal-bad-frequence");
    const string out_dir = r.str("output-dir"), st_dir = r.str("stats-dir");
    const vector<string> files = r.a.list("k-mers");
    mkdirs(out_dir); mkdirs(st_dir);
    r.entry(mf_kmers_samples_count != nullptr, "mf_kmers_samples_count");
    mf_ctx *ctx = r.ctx();
    auto fp = cptrs(files);
    const string out = out_dir + "/n_samples.kmers.bin", st = st_dir + "/n_samples.stat.txt";
    uint64_t c = 0;
    check(mf_kmers_samples_count(ctx, fp.data(), (int)fp.size(), b, k, out.c_str(), st.c_str(), &c));
    logmsg("INFO", "%s k-mers found, %s (100.0%%) of them is good (not erroneous)", group_digits(c).c_str(), group_digits(c).c_str());
    if (c == 0) logmsg("WARN", "No k-mers found in reads! Perhaps you reads file is empty or k-mer size is too big");
    logmsg("INFO", "Good k-mers printed to %s", out.c_str());
    return {PV::file("resulting-kmers-file", out)};
}
// the group comparisons (no -k: the joins work on the files' 64-bit keys).  What the library refuses is refused here first, in its words.
struct Groups { vector<string> files[3]; double pchi2, pmw; string out_dir; };
static Groups groups_of(Run &r, int n) {
    Groups g;
    for (int i = 0; i < n; i++) g.files[i] = r.a.list(i == 0 ? "a-kmers" : i == 1 ? "b-kmers" : "c-kmers");
    g.pchi2 = r.real("p-value-chi2"); g.pmw = r.real("p-value-mw");
    return g;
}
static void check_groups(const Run &r, const Groups &g, int n) {
    const vector<string> &af = g.files[0], &bf = g.files[1], &cf = g.files[2];
    if (n == 2 && (af.empty() || bf.empty())) die("%s: both groups need at least one sample (|A| = %zu, |B| = %zu)", r.t.name, af.size(), bf.size());
    if (n == 3 && (af.empty() || bf.empty() || cf.empty()))
        die("%s: every group needs at least one sample (|A| = %zu, |B| = %zu, |C| = %zu)", r.t.name, af.size(), bf.size(), cf.size());
    if (!(g.pchi2 >= 0.0 && g.pchi2 <= 1.0)) die("Error calculating chi-squared value! (p-value-chi2 = %g is not in [0, 1])", g.pchi2);
}
static void log_group_files(const string &out_dir, int n) {
    for (int i = 0; i < n; i++) logmsg("INFO", "Group %c k-mers printed to %s", 'A' + i, (out_dir + "/filtered_group" + char('A' + i) + ".kmers.bin").c_str());
}
// the counters of stats-kmers (n = 2) and stats-kmers-3 (n = 3): c[6 .. 6 + n) the groups, c[6 + n] the unique k-mers left
static void log_stats_counters(const uint64_t *c, int n) {
    uint64_t left = 0; for (int i = 0; i < n; i++) left += c[6 + i];
    logmsg("DEBUG", "Total k-mers count = %llu", (unsigned long long)c[0]);
    logmsg("DEBUG", "Total unique k-mers = %llu", (unsigned long long)c[3]);
    logmsg("DEBUG", "Total k-mers present in all files = %llu", (unsigned long long)c[2]);
    logmsg("DEBUG", "Total k-mers left = %llu", (unsigned long long)left);
    logmsg("DEBUG", "Total unique left = %llu", (unsigned long long)c[6 + n]);
    for (int i = 0; i < n; i++) logmsg("INFO", "Total group %c k-mers = %llu", 'A' + i, (unsigned long long)c[6 + i]);
    logmsg("DEBUG", "Total scarce k-mers = %llu", (unsigned long long)c[1]);
    logmsg("DEBUG", "Total skipped by Chi-squared test = %llu", (unsigned long long)c[4]);
    logmsg("DEBUG", "Total skipped by Mann-Whitney test = %llu", (unsigned long long)c[5]);
}
static vector<PV> tool_stats_kmers(Run &r) {
    // StatsKmersFinder.java:89-297, StatsKmers3GroupsFinder.java:92-343
    // (--wide-kmers and -k in 32 ... 63, two groups only: the same on wide .kmers.bin files, mf_stats_kmers_wide.  The tool declares no -k: the
    // option is accepted like any other it does not declare, and without the flag, without -k or with k <= 31 nothing changes)
    const int n = !strcmp(r.t.name, "stats-kmers-3") ? 3 : 2;
    const bool wide = n == 2 && wide_host_k(r.k);
    const Groups g = groups_of(r, n);
    const int b = r.num("maximal-bad-frequence");
    const string out_dir = r.str("output-dir");
    if (n == 3) check_groups(r, g, n);
    mkdirs(out_dir);
    if (n == 3) r.entry(mf_stats_kmers3 != nullptr, "mf_stats_kmers3");
    else if (wide) r.entry(mf_stats_kmers_wide != nullptr, "mf_stats_kmers_wide");
    else r.entry(mf_stats_kmers != nullptr, "mf_stats_kmers");
    mf_ctx *ctx = r.ctx();
    logmsg("INFO", "Loading k-mers occurrences...");
    auto pa = cptrs(g.files[0]), pb = cptrs(g.files[1]), pc = cptrs(g.files[2]);
    uint64_t c[MF_STATS3_COUNTERS] = {0};
    static_assert(MF_STATS_COUNTERS <= MF_STATS3_COUNTERS, "one array for both");
    if (n == 3) check(mf_stats_kmers3(ctx, pa.data(), (int)pa.size(), pb.data(), (int)pb.size(), pc.data(), (int)pc.size(), b, g.pchi2, g.pmw, out_dir.c_str(), c));
    else if (wide) check(mf_stats_kmers_wide(ctx, pa.data(), (int)pa.size(), pb.data(), (int)pb.size(), b, r.k, g.pchi2, g.pmw, out_dir.c_str(), c));
    else check(mf_stats_kmers(ctx, pa.data(), (int)pa.size(), pb.data(), (int)pb.size(), b, g.pchi2, g.pmw, out_dir.c_str(), c));
    logmsg("INFO", "Survived after chi-squared test k-mers printed to: %s", (out_dir + "/filtered_chisquared.kmers.bin").c_str());
    log_group_files(out_dir, n);
    log_stats_counters(c, n);
    if (n == 3) return {PV::file("filtered-kmers-file", out_dir + "/filtered_chisquared.kmers.bin")};
    return {PV::files("resulting-kmers-file", {out_dir + "/filtered_groupA.kmers.bin"})};
}
static vector<PV> tool_specific_kmers(Run &r) {
    // SpecificKmersFinder.java:65-216 (no -b either: every file is read at threshold 0)
    const Groups g = groups_of(r, 2);
    const string out_dir = r.str("output-dir");
    check_groups(r, g, 2);
    mkdirs(out_dir);
    r.entry(mf_specific_kmers != nullptr, "mf_specific_kmers");
    mf_ctx *ctx = r.ctx();
    logmsg("INFO", "Splitting k-mers...");
    auto pa = cptrs(g.files[0]), pb = cptrs(g.files[1]);
    uint64_t c[MF_SPECIFIC_COUNTERS] = {0};
    check(mf_specific_kmers(ctx, pa.data(), (int)pa.size(), pb.data(), (int)pb.size(), g.pchi2, g.pmw, out_dir.c_str(), c));
    log_group_files(out_dir, 2);
    logmsg("INFO", "Total specific k-mers in Group A = %llu", (unsigned long long)c[MF_SPECIFIC_GROUP_A]);
    logmsg("INFO", "Total specific k-mers in Group B = %llu", (unsigned long long)c[MF_SPECIFIC_GROUP_B]);
    logmsg("DEBUG", "Total unique k-mers = %llu", (unsigned long long)c[MF_SPECIFIC_UNIQUE]);
    logmsg("DEBUG", "Total scarce k-mers = = %llu", (unsigned long long)c[MF_SPECIFIC_SCARCE]);
    logmsg("DEBUG", "Total skipped by chi-squared test = %llu", (unsigned long long)c[MF_SPECIFIC_SKIP_CHI2]);
    logmsg("DEBUG", "Total skipped by Mann-Whitney test = %llu", (unsigned long long)c[MF_SPECIFIC_SKIP_MW]);
    logmsg("DEBUG", "Total unique left = %llu", (unsigned long long)c[MF_SPECIFIC_UNIQUE_LEFT]);
    logmsg("DEBUG", "Total kmers left = %llu", (unsigned long long)(c[MF_SPECIFIC_GROUP_A] + c[MF_SPECIFIC_GROUP_B]));
    logmsg("DEBUG", "Processed %llu k-mers", (unsigned long long)c[MF_SPECIFIC_TOTAL]);
    return {};
}
static vector<PV> tool_specific_kmers3(Run &r) {
    // SpecificKmers3GroupsFinder.java:70-280.  The counters are those of stats-kmers-3, logged at other levels: the groups at DEBUG, "scarce" at INFO
    const Groups g = groups_of(r, 3);
    const string out_dir = r.str("output-dir");
    check_groups(r, g, 3);
    mkdirs(out_dir);
    r.entry(mf_specific_kmers3 != nullptr, "mf_specific_kmers3");
    mf_ctx *ctx = r.ctx();
    logmsg("INFO", "Splitting k-mers...");
    auto pa = cptrs(g.files[0]), pb = cptrs(g.files[1]), pc = cptrs(g.files[2]);
    uint64_t c[MF_SPECIFIC3_COUNTERS] = {0};
    check(mf_specific_kmers3(ctx, pa.data(), (int)pa.size(), pb.data(), (int)pb.size(), pc.data(), (int)pc.size(), g.pchi2, g.pmw, out_dir.c_str(), c));
    log_group_files(out_dir, 3);
    logmsg("DEBUG", "Total k-mers count = %llu", (unsigned long long)c[0]);
    logmsg("DEBUG", "Total unique k-mers = %llu", (unsigned long long)c[3]);
    logmsg("DEBUG", "Total k-mers present in all files = %llu", (unsigned long long)c[2]);
    logmsg("DEBUG", "Total k-mers left = %llu", (unsigned long long)(c[6] + c[7] + c[8]));
    logmsg("DEBUG", "Total unique left = %llu", (unsigned long long)c[9]);
    logmsg("DEBUG", "Total group A k-mers = %llu", (unsigned long long)c[6]);
    logmsg("DEBUG", "Total group B k-mers = %llu", (unsigned long long)c[7]);
    logmsg("DEBUG", "Total group C k-mers = %llu", (unsigned long long)c[8]);
    logmsg("INFO", "Total scarce k-mers = %llu", (unsigned long long)c[1]);
    logmsg("DEBUG", "Total skipped by Chi-squared test = %llu", (unsigned long long)c[4]);
    logmsg("DEBUG", "Total skipped by Mann-Whitney test = %llu", (unsigned long long)c[5]);
    return {};
}
static vector<PV> tool_unique_kmers(Run &r) {
    // UniqueKmersFinder.java:73-144: the pooled k-mers of the input files that no filter file holds
    const int k = r.k;
    check_k(k);
    const int b = r.num("maximal-bad-frequence");
    const string out_dir = r.str("output-dir"), st_dir = r.str("stats-dir");
    const vector<string> files = r.a.list("k-mers"), filt = r.a.list("filter-kmers");
    r.entry(mf_unique_kmers != nullptr, "mf_unique_kmers");
    mf_ctx *ctx = r.ctx();
    mkdirs(out_dir); mkdirs(st_dir);
    auto fp = cptrs(files), ff = cptrs(filt);
    const string out = out_dir + "/filtered.kmers.bin", st = st_dir + "/filtered.stat.txt";
    uint64_t n = 0, c = 0;
    logmsg("DEBUG", "Starting to print k-mers to %s", out.c_str());
    check(mf_unique_kmers(ctx, fp.data(), (int)fp.size(), ff.data(), (int)ff.size(), b, k, out.c_str(), st.c_str(), &n, &c));
    logmsg("INFO", "%s k-mers found, %s (%s%%) of them is good (present in one dataset and missing in other)", group_digits(n).c_str(),
           group_digits(c).c_str(), percent_or_nan(c, n).c_str());
    if (n == 0) logmsg("WARN", "No k-mers found in reads! Perhaps you reads file is empty or k-mer size is too big");
    else if (c == 0 || c < (uint64_t)(int64_t)(n * 0.03))
        logmsg("WARN", "Too few good k-mers were found! Perhaps you should decrease k-mer size or --maximal-bad-frequency value");
    const uint64_t all_kmers = (1ull << (2 * k)) / 2;                   // (4^k)/2
    if (n == all_kmers) logmsg("WARN", "All possible k-mers were found in reads! Perhaps you should increase k-mer size");
    else if (n >= (uint64_t)(int64_t)(all_kmers * 0.99)) logmsg("WARN", "Almost all possible k-mers were found in reads! Perhaps you should increase k-mer size");
    logmsg("INFO", "Good k-mers printed to %s", out.c_str());
    return {PV::file("resulting-kmers-file", out)};
}
static vector<PV> tool_kmers_grouped_counter(Run &r) {
    // KmersGroupedSamplesCounter.java:82-190: per k-mer of -kf the CD, UC and nonIBD files that hold it with a count > b
    // (--wide-kmers and k > 31: the same on wide .kmers.bin files, mf_kmers_grouped_count_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const int b = r.num("maximal-bad-frequence");
    const string out_dir = r.str("output-dir"), st_dir = r.str("stats-dir");
    const vector<string> kf = r.a.list("kmers-file"), cd = r.a.list("cd-kmers"), uc = r.a.list("uc-kmers"), ni = r.a.list("nonibd-kmers");
    mkdirs(out_dir); mkdirs(st_dir);
    if (wide) r.entry(mf_kmers_grouped_count_wide != nullptr, "mf_kmers_grouped_count_wide"); else r.entry(mf_kmers_grouped_count != nullptr, "mf_kmers_grouped_count");
    mf_ctx *ctx = r.ctx();
    auto pkf = cptrs(kf), pcd = cptrs(cd), puc = cptrs(uc), pni = cptrs(ni);
    const string out = out_dir + "/kmers.groups.txt";
    uint64_t c = 0;
    logmsg("DEBUG", "Starting to print k-mers to %s", out.c_str());
    check((wide ? mf_kmers_grouped_count_wide : mf_kmers_grouped_count)(ctx, pkf.data(), (int)pkf.size(), pcd.data(), (int)pcd.size(), puc.data(), (int)puc.size(),
                                                                        pni.data(), (int)pni.size(), b, k, out.c_str(), &c));
    logmsg("INFO", "K-mers printed to %s", out.c_str());
    return {};
}
static vector<PV> tool_kmers_per_sample(Run &r) {
    // KmersPerSampleCounter.java:56-157: the abundance in every file of the k-mers that enough files hold (no -b: every load is at 0).
    // The first file is not counted, as in the reference (:82-96): count_first = 0.
    // (--wide-kmers and k > 31: the same on wide .kmers.bin files, mf_kmers_per_sample_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const int perc = r.num("percent-present");
    const string out_dir = r.str("output-dir");
    const vector<string> files = r.a.list("k-mers");
    mkdirs(out_dir);
    if (wide) r.entry(mf_kmers_per_sample_wide != nullptr, "mf_kmers_per_sample_wide"); else r.entry(mf_kmers_per_sample != nullptr, "mf_kmers_per_sample");
    mf_ctx *ctx = r.ctx();
    auto fp = cptrs(files);
    const string out = out_dir + "/selected_kmers_" + std::to_string(perc) + ".txt";
    uint64_t c = 0;
    logmsg("INFO", "Loading all k-mers...");
    logmsg("DEBUG", "Starting to print k-mers to %s", out.c_str());
    check((wide ? mf_kmers_per_sample_wide : mf_kmers_per_sample)(ctx, fp.data(), (int)fp.size(), k, perc, 0, out.c_str(), &c));
    logmsg("DEBUG", "Selected k-mers = %s", group_digits(c).c_str());
    logmsg("INFO", "K-mers printed to %s", out.c_str());
    return {};
}
static vector<PV> tool_unique_kmers_multi(Run &r) {
    // UniqueKmersMultipleSamplesFinder.java:84-185: the k-mers that enough input files hold and no filter file does
    // (--wide-kmers and k > 31: the same on wide .kmers.bin files, mf_unique_kmers_multi_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const int mn = r.num("min-samples"), mx = r.num("max-samples"), b = r.num("maximal-bad-frequence");
    if (mn > mx) die("--min-samples parameter cannot be greater than --max-samples parameter.");
    const string out_dir = r.str("output-dir"), st_dir = r.str("stats-dir");
    const vector<string> files = r.a.list("k-mers"), filt = r.a.list("filter-kmers");
    if (wide) r.entry(mf_unique_kmers_multi_wide != nullptr, "mf_unique_kmers_multi_wide"); else r.entry(mf_unique_kmers_multi != nullptr, "mf_unique_kmers_multi");
    mf_ctx *ctx = r.ctx();
    mkdirs(out_dir); mkdirs(st_dir);
    auto fp = cptrs(files), ff = cptrs(filt);
    const int64_t top = std::min<int64_t>(mx, std::max<int64_t>(mn, (int64_t)files.size() + 1));
    vector<uint64_t> c((size_t)std::max<int64_t>(1, top - mn + 1), 0);
    int n_out = 0; uint64_t n_union = 0;
    check((wide ? mf_unique_kmers_multi_wide : mf_unique_kmers_multi)(ctx, fp.data(), (int)fp.size(), ff.data(), (int)ff.size(), b, k, mn, mx, out_dir.c_str(), &n_out, &n_union, c.data()));
    for (int q = 0; q < n_out; q++) {
        const string out = out_dir + "/filtered_" + std::to_string(mn + q) + ".kmers.bin";
        logmsg("INFO", "%s k-mers found, %s (%s%%) of them is good (present in one dataset and missing in other)", group_digits(n_union).c_str(),
               group_digits(c[(size_t)q]).c_str(), percent_or_nan(c[(size_t)q], n_union).c_str());
        if (c[(size_t)q] == 0) { logmsg("INFO", "No good k-mers found. Stop at maxSamples=%d", mn + q); break; }
        logmsg("INFO", "Good k-mers printed to %s", out.c_str());
    }
    return {PV::files("resulting-kmers-file", {out_dir + "/filtered_" + std::to_string(mn) + ".kmers.bin"})};
}
static vector<PV> tool_kmers_multiple_filters(Run &r) {
    // KmersMultipleFilters.java:77-133: every input file against the CD, UC and nonIBD sets of n_samples files
    const int k = r.k;
    check_k(k);
    const int b = r.num("maximal-bad-frequence");
    const string out_dir = r.str("output-dir"), st_dir = r.str("stats-dir");
    const vector<string> files = r.a.list("k-mers"), cd = r.a.list("cd-filter-kmers"), uc = r.a.list("uc-filter-kmers"), ni = r.a.list("nonibd-filter-kmers");
    r.entry(mf_kmers_multiple_filters != nullptr, "mf_kmers_multiple_filters");
    mf_ctx *ctx = r.ctx();
    mkdirs(out_dir); mkdirs(st_dir);
    vector<string> ok, os;
    for (auto &f : files) {
        // file.getName().replaceAll(".kmers.bin", ""): a regular expression, every '.' matches any character but a line end
        const string base = basename_of(f), pat = ".kmers.bin";
        string name;
        for (size_t q = 0; q < base.size();) {
            bool m = q + pat.size() <= base.size();
            for (size_t r = 0; m && r < pat.size(); r++) m = pat[r] == '.' ? (base[q + r] != '\n' && base[q + r] != '\r') : base[q + r] == pat[r];
            if (m) q += pat.size(); else name.push_back(base[q++]);
        }
        ok.push_back(out_dir + "/" + name + ".kmers.bin"); os.push_back(st_dir + "/" + name + ".stat.txt");
    }
    auto fp = cptrs(files), pcd = cptrs(cd), puc = cptrs(uc), pni = cptrs(ni), pok = cptrs(ok), pos = cptrs(os);
    vector<uint64_t> fk(2 * files.size() + 2, 0);
    check(mf_kmers_multiple_filters(ctx, fp.data(), (int)fp.size(), pcd.data(), (int)pcd.size(), puc.data(), (int)puc.size(), pni.data(), (int)pni.size(),
                                    b, k, pok.data(), pos.data(), fk.data()));
    for (size_t j = 0; j < files.size(); j++) {
        logmsg("INFO", "%s k-mers found, %s (%s%%) of them survived after filtering", group_digits(fk[2 * j]).c_str(), group_digits(fk[2 * j + 1]).c_str(),
               percent_or_nan(fk[2 * j + 1], fk[2 * j]).c_str());
        logmsg("INFO", "Filtered k-mers printed to %s", ok[j].c_str());
    }
    return {};
}
static vector<PV> tool_kmers_color(Run &r) {
    // ColorKmersMain.java:89-136: per k-mer and class 0 / 1 / 2 the number of samples that hold it (-val: their summed coverage)
    // (--wide-kmers and k > 31: the same on wide .kmers.bin files into 24-byte records, mf_kmers_color_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const int b = r.num("maximal-bad-frequency");
    const bool val = r.a.flag("val");
    const string out_dir = r.str("output-dir"), cls = r.str("class");
    const vector<string> files = r.a.list("k-mers");
    logmsg("INFO", "Loading class file...");
    // readFileToColor :70-82: tab-separated lines, name (the file name without .kmers.bin) and class
    std::map<string, int> color;
    {
        FILE *f = fopen(cls.c_str(), "r");
        if (!f) die("Cannot read file: %s", cls.c_str());
        char line[8192]; int ln = 0;
        while (fgets(line, sizeof line, f)) {
            ln++;
            string l(line);
            while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
            const size_t t1 = l.find('\t');
            if (t1 == string::npos) { fclose(f); die("class file %s, line %d: no tab-separated class after '%s'", cls.c_str(), ln, l.c_str()); }
            const size_t t2 = l.find('\t', t1 + 1);
            const string name = l.substr(0, t1), cv = l.substr(t1 + 1, t2 == string::npos ? string::npos : t2 - t1 - 1);
            char *end; const long c = strtol(cv.c_str(), &end, 10);
            if (cv.empty() || *end) { fclose(f); die("class file %s, line %d: can't parse class '%s' of sample '%s'", cls.c_str(), ln, cv.c_str(), name.c_str()); }
            if (c < 0 || c > 2) { fclose(f); die("class file %s, line %d: sample '%s' has class %ld (the classes are 0, 1 and 2)", cls.c_str(), ln, name.c_str(), c); }
            color[name] = (int)c;
        }
        fclose(f);
    }
    vector<int> classes;
    for (auto &fn : files) {
        const string name = remove_ext(basename_of(fn), {".kmers.bin"});
        auto it = color.find(name);
        if (it == color.end()) die("class file %s has no line for sample '%s' (%s)", cls.c_str(), name.c_str(), fn.c_str());
        classes.push_back(it->second);
    }
    if (files.size() > 1024) die("kmers-color: %zu k-mers files, at most 1024 (a field of the packed value holds 20 bits)", files.size());
    mkdirs(out_dir);
    if (wide) r.entry(mf_kmers_color_wide != nullptr, "mf_kmers_color_wide"); else r.entry(mf_kmers_color != nullptr, "mf_kmers_color");
    mf_ctx *ctx = r.ctx();
    logmsg("INFO", "Loading kmers files...");
    auto fp = cptrs(files);
    const string out = out_dir + "/colored_kmers.kmers.bin", st = out_dir + "/colored_kmers.stat.txt";
    uint64_t c = 0;
    check((wide ? mf_kmers_color_wide : mf_kmers_color)(ctx, fp.data(), classes.data(), (int)fp.size(), b, val ? 1 : 0, k, out.c_str(), st.c_str(), &c));
    logmsg("INFO", "%s colored k-mers printed to %s", group_digits(c).c_str(), out.c_str());
    return {PV::file("resulting-kmers-file", out)};
}
static vector<PV> tool_component_colored(Run &r) {
    // ColoredComponentMain.java:83-119, default and --separate modes of ColoredComponentsBuilder
    // (--wide-kmers and k > 31: the same on a wide colored_kmers.kmers.bin into wide components_color_<c>.bin, mf_colored_components_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const int groups = r.num("n_groups"), ncomps = r.num("n_comps");
    const bool separate = r.a.flag("separate");
    const double perc = r.real("perc");
    if (r.a.flag("linear"))
        die("component-colored: --linear is not supported: its result depends on the iteration order of the reference's hash map");
    if (ncomps != -1)
        die("component-colored: --n_comps %d is not supported (only -1, all components): which components are selected depends on the iteration order of the reference's hash map", ncomps);
    if (groups < 1) die("component-colored: --n_groups %d: at least 1", groups);
    const string out_dir = r.str("output-dir"), stat = r.wd + "/components-stat.txt";
    const vector<string> files = r.a.list("k-mers");
    mkdirs(out_dir);
    if (wide) r.entry(mf_colored_components_wide != nullptr, "mf_colored_components_wide"); else r.entry(mf_colored_components != nullptr, "mf_colored_components");
    mf_ctx *ctx = r.ctx();
    logmsg("DEBUG", "Loading colored k-mers...");
    logmsg("INFO", "Searching for colored components...");
    auto fp = cptrs(files);
    vector<uint64_t> cnt((size_t)groups, 0);
    // (IOUtils.loadLongKmers(files, k, ...): the reference passes k where the loader takes its value threshold)
    check((wide ? mf_colored_components_wide : mf_colored_components)(ctx, fp.data(), (int)fp.size(), k, (int64_t)k, groups, separate ? 1 : 0, perc, out_dir.c_str(), stat.c_str(), cnt.data()));
    uint64_t total = 0;
    vector<string> written;
    for (int c = 0; c < groups; c++) {
        total += cnt[(size_t)c];
        logmsg("INFO", "%s components were found for class %d", group_digits(cnt[(size_t)c]).c_str(), c);
        written.push_back(out_dir + "/components_color_" + std::to_string(c) + ".bin");
    }
    logmsg("INFO", "Total %s components were found", group_digits(total).c_str());
    return {PV::files("components-files", written)};
}
static vector<PV> tool_comp2seq(Run &r) {
    // ComponentsToSequences.java:41-76: bin2fasta, kmer-counter-many -b 0, seq-builder-many -b 0 -l k as sub-steps with the work
    // directories kmers_fasta, kmer-counter-many and seq-builder-many -- here one segmented build of all components (mf_comp2seq)
    // (--wide-kmers and k > 31: the same on a wide components.bin, mf_comp2seq_wide)
    const int k = r.k; const string &wd = r.wd;
    const bool wide = wide_k(k);
    if (!wide) check_k(k);
    const bool split = r.a.flag("split");
    const string cf = r.str("components-file");
    if (wide) r.entry(mf_comp2seq_wide != nullptr, "mf_comp2seq_wide"); else r.entry(mf_comp2seq != nullptr, "mf_comp2seq");
    mf_ctx *ctx = r.ctx();
    uint64_t nf = 0, ns = 0;
    check(wide ? mf_comp2seq_wide(ctx, cf.c_str(), k, split ? 1 : 0, wd.c_str(), &nf, &ns) : mf_comp2seq(ctx, cf.c_str(), k, split ? 1 : 0, wd.c_str(), &nf, &ns));
    if (split) logmsg("INFO", "%s components loaded from %s", group_digits(nf).c_str(), cf.c_str());
    logmsg("INFO", "%s sequences found", group_digits(ns).c_str());
    if (ns == 0) logmsg("WARN", "No sequences were found! Perhaps you should decrease --min-seq-len or --maximal-bad-frequency values");
    logmsg("INFO", "Sequences printed to %s", (wd + "/seq-builder-many/sequences").c_str());
    vector<string> written;
    for (uint64_t i = 0; i < nf; i++) written.push_back(wd + "/seq-builder-many/sequences/component" + (split ? "_" + std::to_string(i + 1) : string()) + ".seq.fasta");
    return {PV::files("output-files", written)};
}
static vector<PV> tool_comp2graph(Run &r) {
    // ComponentsToGraph.java:70-130: one Comp2Graph per component on a thread pool, a HashMap of strings and a quadratic merge loop
    // each -- here the graphs of all components in one pass, the text formatted on the device (mf_comp2graph)
    // (--wide-kmers and k > 31: the same on a wide components.bin and wide .kmers.bin files, mf_comp2graph_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const string cf = r.str("components-file"), gf = r.str("graph-file");
    const vector<string> files = r.a.list("k-mers");
    const bool cov = r.a.flag("coverage");                                // (without -i: accepted and ignored, as in the reference)
    if (wide) r.entry(mf_comp2graph_wide != nullptr, "mf_comp2graph_wide"); else r.entry(mf_comp2graph != nullptr, "mf_comp2graph");
    mf_ctx *ctx = r.ctx();
    auto fp = cptrs(files);
    uint64_t nc = 0, ns = 0, nl = 0;
    check((wide ? mf_comp2graph_wide : mf_comp2graph)(ctx, cf.c_str(), k, files.empty() ? nullptr : fp.data(), (int)files.size(), cov ? 1 : 0, gf.c_str(), &nc, &ns, &nl));
    logmsg("INFO", "%s components loaded from %s", group_digits(nc).c_str(), cf.c_str());
    logmsg("INFO", "Graph components saved to GFA format!");
    return {PV::file("graph-file", gf)};
}
static vector<PV> tool_seq2comp(Run &r) {
    // SequencesToComponents.java:61-103: a component per sequence that survives the readers, its members the distinct canonical k-mers
    // (a LongArraySet with a linear scan per add there: quadratic in the sequence's length) -- here a segmented set-build on the
    // device (mf_seq2comp).  Components in file order, then record order (the reference: as its thread pool finishes); a sequence
    // shorter than k keeps its place as an empty component
    // (--wide-kmers and k > 31: the same on 2k-bit k-mers into a wide components.bin, mf_seq2comp_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const vector<string> files = r.a.list("sequences");
    const string cf = r.str("components-file"), sf = r.wd + "/components-stat.txt";
    for (auto &f : files) if (!exists(f)) die("Can't load sequences: file not found (%s)", f.c_str());
    if (wide) r.entry(mf_seq2comp_wide != nullptr, "mf_seq2comp_wide"); else r.entry(mf_seq2comp != nullptr, "mf_seq2comp");
    mf_ctx *ctx = r.ctx();
    logmsg("DEBUG", "Loading sequences from files...");
    auto fp = cptrs(files);
    vector<uint64_t> per(files.size() + 1, 0);
    uint64_t nc = 0;
    mkparent(cf);
    check((wide ? mf_seq2comp_wide : mf_seq2comp)(ctx, files.empty() ? nullptr : fp.data(), (int)files.size(), k, cf.c_str(), sf.c_str(), &nc, per.data()));
    for (size_t i = 0; i < files.size(); i++) {          // (the reference logs each pair as it goes; the numbers are the same)
        logmsg("INFO", "Loading file %s...", basename_of(files[i]).c_str());
        logmsg("INFO", "%llu components added", (unsigned long long)per[i]);
    }
    logmsg("INFO", "Total %s components were found", group_digits(nc).c_str());
    logmsg("INFO", "Components saved to %s", cf.c_str());
    describe(sf, "File with components' statistics (in text format)");
    describe(cf, "File with components made from the input sequences, one per sequence (in binary format)");
    return {PV::file("components-file", cf), PV::file("components-stat", sf)};
}
static vector<PV> tool_component_paths(Run &r) {
    // ComponentPathsMain.java:82-190: for every sequence one hash set per selected component is probed, O(components x bases) -- here
    // one lookup per k-mer position in an index over the members of all selected components, the runs found, paired, capped, sorted
    // and printed on the device (mf_comppaths.hip).  Without a selection the reference logs its message and ends cleanly; here the
    // run fails with it.  A number out of range is an exception there and an error here.
    // (--wide-kmers and k > 31: a wide components.bin through mf_wcomps_load, the same handle from mf_paths_create_wide)
    const int k = r.k;
    const bool wide = wide_host_k(k);
    if (!wide) check_k(k);
    const string cf = r.str("components-file"), od = r.str("output-dir");
    const vector<string> files = r.a.list("seq");
    const bool all = r.a.flag("all-components");
    const int min_len = r.num("min-length");
    vector<uint32_t> sel;
    for (auto &v : r.a.list("components")) {
        char *end = nullptr; const long long no = strtoll(v.c_str(), &end, 10);
        if (v.empty() || *end) die("Can't parse integer value '%s' of option --components", v.c_str());
        if (no < 1 || no > 0xFFFFFFFFll) die("There is no component %s (components are numbered from 1)", v.c_str());
        sel.push_back((uint32_t)no);
    }
    if (!all && sel.empty()) die("No components to process!!! Do you forget to set --all-components or --components n1,n2,...?");
    if (!exists(cf)) die("Can't load components: file not found (%s)", cf.c_str());
    for (auto &f : files) if (!exists(f)) die("Can't load sequences: file not found (%s)", f.c_str());
    if (wide) r.entry(mf_paths_create_wide && mf_wcomps_load && mf_wcomps_stats && mf_wcomps_destroy, "mf_paths_create_wide");
    r.entry(mf_paths_create && mf_paths_add && mf_paths_finish && mf_paths_destroy && mf_paths_slots && mf_paths_write && mf_paths_stats && mf_comps_load &&
            mf_comps_set_k && mf_comps_stats && mf_comps_destroy && mf_reads_load && mf_reads_stats && mf_reads_device_view && mf_reads_destroy, "mf_paths_create");
    mf_ctx *ctx = r.ctx();
    logmsg("DEBUG", "Loading components...");
    mf_comps *c = nullptr;
    mf_wcomps *wc = nullptr;
    uint64_t nc = 0;
    if (wide) {
        check(mf_wcomps_load(ctx, cf.c_str(), k, &wc));
        check(mf_wcomps_stats(wc, &nc, nullptr));
    } else {
        check(mf_comps_load(ctx, cf.c_str(), &c));
        check(mf_comps_set_k(c, k));
        check(mf_comps_stats(c, &nc, nullptr));
    }
    logmsg("INFO", "%s components loaded from %s", group_digits(nc).c_str(), cf.c_str());
    if (all && nc == 0) die("No components to process!!!");
    logmsg("DEBUG", "Preparing...");
    mf_paths *paths = nullptr;
    const uint64_t max_paths = 1000000;                                   // MAX_PATHS_COUNT (:30)
    if (wide) check(mf_paths_create_wide(ctx, wc, all ? nullptr : sel.data(), all ? 0 : sel.size(), min_len, max_paths, &paths));
    else check(mf_paths_create(ctx, c, all ? nullptr : sel.data(), all ? 0 : sel.size(), min_len, max_paths, &paths));
    logmsg("DEBUG", "Loading sequences and extracting paths...");
    for (auto &f : files) {                                               // one file resident at a time
        logmsg("INFO", "Loading file %s...", basename_of(f).c_str());
        const char *fp = f.c_str();
        mf_reads *r = nullptr;
        check(mf_reads_load(ctx, &fp, 1, &r));
        const void *db = nullptr, *doff = nullptr; uint64_t nr = 0, nb = 0;
        check(mf_reads_stats(r, &nr, &nb));
        check(mf_reads_device_view(r, &db, &doff));
        check(mf_paths_add(paths, db, doff, nr, nb));
        mf_reads_destroy(r);
    }
    check(mf_paths_finish(paths));
    uint64_t nslots = 0;
    check(mf_paths_stats(paths, &nslots, nullptr, nullptr, nullptr));
    vector<uint32_t> no(nslots + 1, 0); vector<uint8_t> reached(nslots + 1, 0);
    check(mf_paths_slots(paths, no.data(), nullptr, nullptr, reached.data()));
    for (uint64_t i = 0; i < nslots; i++)
        if (reached[i]) logmsg("WARN", "Too many paths in component %u, keeping only first %llu of them!", no[i], (unsigned long long)max_paths);
    logmsg("INFO", "Sorting...");
    logmsg("INFO", "Saving to files...");
    mkparent(od);
    uint64_t np = 0;
    check(mf_paths_write(paths, od.c_str(), &np));
    mf_paths_destroy(paths);
    if (wide) mf_wcomps_destroy(wc); else mf_comps_destroy(c);
    logmsg("INFO", "Paths for %llu component(s) were saved in directory %s", (unsigned long long)nslots, od.c_str());
    return {};
}
static vector<PV> tool_view(Run &r) { run_view(r.a, r.k); return {}; }
static vector<PV> tool_bin2fasta(Run &r) { run_bin2fasta(r.a, r.k); return {}; }
static vector<PV> tool_heatmap_maker(Run &r) {
    const bool wr = r.a.flag("without-renumbering");
    const string nm = run_heatmap_maker(r.e, r.str("matrix-file"), r.str("newMatrix-file"), wr, r.str("output-format"));
    return {PV::null("heatmap-file"), wr ? PV::null("newMatrix-file-out") : PV::file("newMatrix-file-out", nm)};
}
static vector<PV> tool_matrix_builder(Run &r) {
    // DistanceMatrixBuilderMain.java:88-175: steps kmer-counter-many, seq-builder-many, component-cutter, features-calculator,
    // dist-matrix-calculator, heatmap-maker (its image is not rendered here).  What the builder does not fix is the step's own default.
    Env &e = r.e; const Args &a = r.a; const string &wd = r.wd, &start = r.start, &finish = r.finish; const int k = r.k; bool &force = r.force;
    vector<string> reads = a.list("reads");
    logmsg("INFO", "Found %zu libraries to process", reads.size());
    if (reads.empty()) die("No libraries to process!!! Can't continue the calculations.");
    const bool use_reads = a.flag("use-reads-for-calculating-features");                       // DistanceMatrixBuilderMain.java:162-165
    if (wide_k(k)) { no_wide(!a.list("selected").empty(), "selected"); no_wide(use_reads, "use-reads-for-calculating-features"); }
    else check_k(k);
    // (-b in either spelling: the counters' --maximal-bad-frequence is taken where --maximal-bad-frequency is not given)
    const int b = a.geti("maximal-bad-frequency", a.geti("maximal-bad-frequence", atoi(r.dflt("maximal-bad-frequency").c_str()))), l = r.num("min-seq-len");
    const int b1 = r.num("min-component-size"), b2 = r.num("max-component-size");
    static const char *STEPS[] = {"kmer-counter-many", "seq-builder-many", "component-cutter", "features-calculator", "dist-matrix-calculator", "heatmap-maker"};
    for (const string *bound : {&start, &finish})                           // Tool.checkBoundExistence :726-741
        if (!bound->empty() && std::find_if(std::begin(STEPS), std::end(STEPS), [&](const char *n) { return *bound == n; }) == std::end(STEPS))
            die("There is no substep with name '%s' in step matrix-builder!", bound->c_str());
    {   // createOutputDescFiles :178-200
        g_desc_files = {"output_description.txt", wd + "/output_description.txt"};
        time_t t = time(nullptr); struct tm tmv; localtime_r(&t, &tmv);
        char hdr[128]; strftime(hdr, sizeof hdr, "%d-%b-%Y (%a) %H:%M:%S", &tmv);
        for (auto &d : g_desc_files) {
            FILE *f = fopen(d.c_str(), "w");
            if (!f) { logmsg("WARN", "Can't create file %s, skipping", d.c_str()); continue; }
            fprintf(f, "# Output files' description for run started at %s\n\n%s\n%s\n   Identical files with run log\n\n%s\n%s\n   Identical files with output files' description\n",
                    hdr, (wd + "/log").c_str(), (wd + "/logs/log_" + e.start_ts).c_str(), g_desc_files[0].c_str(), g_desc_files[1].c_str());
            fclose(f);
        }
    }
    const string d1 = wd + "/kmer-counter-many", d2 = wd + "/seq-builder-many", d3 = wd + "/component-cutter", d4 = wd + "/features-calculator",
                 d5 = wd + "/dist-matrix-calculator", d6 = wd + "/heatmap-maker";
    const string dirs[] = {d1, d2, d3, d4, d5, d6};
    // --finish <step>: stop after it; the next step's results are outdated then (:512-527)
    auto finished = [&](int i) {
        if (finish.empty() || finish != STEPS[i]) return false;
        if (i + 1 < 6) { unlink((dirs[i + 1] + "/SUCCESS").c_str()); unlink((dirs[i + 1] + "/in.properties").c_str()); }
        return true;
    };
    auto done = [&]() -> vector<PV> { for (mf_ctx *c : e.ctxs) if (c) mf_ctx_destroy(c); exit(0); };      // (a run cut short by --finish ends here: no out.properties, no SUCCESS)
    vector<string> kmers, seqs, vecs;
    // 1 kmer-counter-many
    const string stats_dir = r.str("stats-dir"), kmers_dir = sub_default(r, STEPS[0], "output-dir", d1);
    run_as_step(STEPS[0], d1, {PV("k", k), PV::files("reads", reads), PV("maximal-bad-frequence", b), PV::file("output-dir", kmers_dir), PV::file("stats-dir", stats_dir)},
                start, force,
                [&]() { kmers = run_kmer_counter_many(e, a, reads, k, b, d1, kmers_dir, stats_dir); return vector<PV>{PV::files("resulting-kmers-files", kmers)}; },
                [&](const Props &o) { kmers = props_list(o, "resulting-kmers-files"); });
    describe(stats_dir, "Directory with kmer frequency statistics (statistics files is in text format for every input reads file)");
    if (finished(0)) return done();
    // 2 seq-builder-many
    const int bp = r.num("bottom-cut-percent");
    const string seq_dir = sub_default(r, STEPS[1], "output-dir", d2);
    run_as_step(STEPS[1], d2, {PV("k", k), PV::files("k-mers", kmers), PV("maximal-bad-frequency", b), bp >= 0 ? PV("bottom-cut-percent", bp) : PV::null("bottom-cut-percent"),
                               PV("sequence-len", l), PV::file("output-dir", seq_dir)},
                start, force,
                [&]() { seqs = run_seq_builder_many(e, a, kmers, k, b, bp, l, d2, seq_dir);
                        return vector<PV>{PV::files("output-files", seqs)}; },
                [&](const Props &o) { seqs = props_list(o, "output-files"); });
    describe(seq_dir, "Directory with FASTA files - paths from reads for every library");
    if (finished(1)) return done();
    // 3 component-cutter
    const string comp = sub_default(r, STEPS[2], "components-file", d3), cstat = cutter_stat(d3, b1, b2);
    run_as_step(STEPS[2], d3, {PV("k", k), PV("min-seq-len", l), PV("min-component-size", b1), PV("max-component-size", b2), PV::files("sequences", seqs), PV::file("components-file", comp)},
                start, force,
                [&]() { run_component_cutter(e, a, seqs, k, l, b1, b2, d3, comp); return vector<PV>{PV::file("components-file", comp), PV::file("components-stat", cstat)}; },
                [&](const Props &) {});
    describe(cstat, "File with components' statistics (in text format)");
    describe(comp, "File with extracted components (in binary format)");
    if (finished(2)) return done();
    // 4 features-calculator
    const vector<string> none;
    const int thr = atoi(sub_default(r, STEPS[3], "threshold", d4).c_str());
    run_as_step(STEPS[3], d4, {PV("k", k), PV::file("components-file", comp), PV::files("reads", use_reads ? reads : none), PV::files("kmers", use_reads ? none : kmers),
                               PV::files("selected", a.list("selected")), PV("threshold", thr)},
                start, force,
                [&]() { vecs = use_reads ? run_features(e, a, comp, reads, {}, k, thr, d4) : run_features(e, a, comp, {}, kmers, k, thr, d4);
                        return vector<PV>{PV::files("features-files", vecs), PV::file("features-dir", d4 + "/vectors")}; },
                [&](const Props &o) { vecs = props_list(o, "features-files"); });
    describe(d4 + "/vectors", "Directory with features values files for every library (in text format)");
    if (finished(3)) return done();
    // 5 dist-matrix-calculator: the matrix in the original order goes to <workDir>/matrices (:132-134)
    string mpath = wd + "/matrices/dist_matrix_" + e.start_ts + "_original_order.txt";
    const bool wn = a.flag("without-names");
    const string fmt = r.str("output-format");
    run_as_step(STEPS[4], d5, {PV::files("features", vecs), PV::flag("without-names", wn), PV::file("matrix-file", mpath), PV("output-format", fmt)},
                start, force,
                [&]() { mkdirs(wd + "/matrices"); mpath = run_dist_matrix(e, vecs, mpath, wn, fmt); return vector<PV>(); },
                [&](const Props &) {});
    describe(mpath, "File with resulted distance matrix between samples keeping original order");
    if (finished(4)) return done();
    // 6 heatmap-maker, numeric half: dendrogram order + renumbered matrix (:137-145)
    const string npath = with_dt(r.str("matrix-file"), e.start_ts);
    const bool wr = a.flag("without-renumbering");
    run_as_step(STEPS[5], d6, {PV::file("matrix-file", mpath), PV::file("colors-file", r.str("colors-file")), PV::flag("without-renumbering", wr), PV::file("newMatrix-file", npath),
                               PV::file("heatmap-file", with_dt(r.str("heatmap-file"), e.start_ts)), PV::flag("invert-colors", a.flag("invert-colors")), PV("output-format", fmt)},
                start, force,
                [&]() { run_heatmap_maker(e, mpath, npath, wr, fmt); return vector<PV>{PV::null("heatmap-file"), wr ? PV::null("newMatrix-file-out") : PV::file("newMatrix-file-out", npath)}; },
                [&](const Props &) {});
    if (!wr) describe(npath, "File with resulted distance matrix between samples with new order based on adjacency of the samples");
    logmsg("INFO", "heatmap image (dist_matrix_<date>_heatmap.png) is not rendered by the HIP path");
    if (finished(5)) return done();
    return {};
}

// ------------------------------------------------------------------------------------------------ the table: one row per tool, in the order of -ts
// name, description, run function; {short option, what it means here}; {mandatory argument, its short name in the message} in checking
// order; {parameter, kind, default} in the reference's declaration order.  A new tool is one row here and one run function above.
#define K_ {"k", VAL}
#define B_(spelling, dflt) {"maximal-bad-" spelling, VAL, dflt}
#define OUT_(dir) {"output-dir", FILE1, "$WD/" dir}
#define STATS_ {"stats-dir", FILE1, "$WD/stats"}
#define PVALUES_ {"p-value-chi2", VAL, "0.05"}, {"p-value-mw", VAL, "0.05"}
static const Tool TOOLS[] = {
    {"kmer-counter", "Count k-mers in given reads", tool_kmer_counter, {{"b", "maximal-bad-frequence"}}, {{"k", "k"}, {"reads", "i"}},
     {K_, {"reads", FILES}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    {"kmer-counter-many", "Count k-mers in many files (one library = one output)", tool_kmer_counter_many, {{"b", "maximal-bad-frequence"}}, {{"k", "k"}, {"reads", "i"}},
     {K_, {"reads", FILES}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    {"seq-builder", "Metagenome De Bruijn graph analysis and sequences building", tool_seq_builder, {{"i", "k-mers"}, {"l", "sequence-len"}},
     {{"k", "k"}, {"k-mers", "i"}, {"sequence-len", "l"}}, {K_, {"k-mers", FILES}, B_("frequency", "1"), {"bottom-cut-percent", VAL}, {"sequence-len", VAL}, OUT_("sequences")}},
    {"seq-builder-many", "seq-builder for many k-mers files", tool_seq_builder, {{"i", "k-mers"}, {"l", "sequence-len"}},
     {{"k", "k"}, {"k-mers", "i"}, {"sequence-len", "l"}}, {K_, {"k-mers", FILES}, B_("frequency", nullptr), {"bottom-cut-percent", VAL}, {"sequence-len", VAL}, OUT_("sequences")}},
    {"component-cutter", "Build graph components from sequences", tool_component_cutter, {{"i", "sequences"}}, {{"k", "k"}, {"sequences", "i"}},
     {K_, {"min-seq-len", VAL, "100"}, {"min-component-size", VAL, "1000"}, {"max-component-size", VAL, "10000"}, {"sequences", FILES}, {"components-file", FILE1, "$WD/components.bin"}}},
    {"features-calculator", "Calculate features values for input reads/k-mers files", tool_features, {}, {{"k", "k"}, {"components-file", "cm"}},
     {K_, {"components-file", FILE1}, {"reads", FILES}, {"kmers", FILES}, {"selected", FILES}, {"threshold", VAL, "0"}}},
    {"dist-matrix-calculator", "Calculate the distance matrix using features values", tool_dist_matrix, {}, {{"features"}},
     {{"features", FILES}, {"without-names", FLAG}, {"matrix-file", DTFILE, "$WD/dist_matrix_$DT_original_order.txt"}, {"output-format", VAL, "%.4f"}}},
    {"heatmap-maker", "Cluster the samples of a distance matrix and renumber it (no image)", tool_heatmap_maker, {{"i", "matrix-file"}}, {{"matrix-file", "i"}},   // HeatMapMakerMain.java:34-36
     {{"matrix-file", FILE1}, {"colors-file", FILE1}, {"without-renumbering", FLAG}, {"newMatrix-file", FILE1}, {"heatmap-file", FILE1}, {"invert-colors", FLAG},
      {"output-format", VAL, "%.4f"}}},
    {"kmer-counter-posneg", "Count k-mers for files from two groups independently", tool_posneg, {}, {{"k", "k"}, {"positiveReads", "pos"}, {"negativeReads", "neg"}},
     {K_, {"positiveReads", FILES}, {"negativeReads", FILES}, B_("frequency", "1"), OUT_("kmers_posneg")}},
    {"kmers-filter", "Filter k-mers from test set according to known samples", tool_kmers_filter, {{"i", "k-mers"}, {"b", "maximal-bad-frequence"}},
     {{"k", "k"}, {"k-mers", "i"}, {"filter-kmers"}}, {K_, {"k-mers", FILES}, {"filter-kmers", FILES}, B_("frequence", "1"), {"max-thresh", VAL, "0"}, OUT_("kmers"), STATS_}},
    {"kmers-samples-counter", "Count number of samples containing k-mers from multiple samples", tool_kmers_samples_counter, {{"i", "k-mers"}, {"b", "maximal-bad-frequence"}},
     {{"k", "k"}, {"k-mers", "i"}}, {K_, {"k-mers", FILES}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    // (stats-kmers: -i means --k-mers, which the tool does not declare: accepted and ignored)
    {"stats-kmers", "Find k-mers that differ significantly between two groups of samples (chi-squared + Mann-Whitney)", tool_stats_kmers,
     {{"i", "k-mers"}, {"b", "maximal-bad-frequence"}}, {{"a-kmers", "A"}, {"b-kmers", "B"}}, {{"a-kmers", FILES}, {"b-kmers", FILES}, PVALUES_, B_("frequence", "0"), OUT_("kmers")}},
    {"stats-kmers-3", "Find k-mers that differ significantly between three groups of samples (chi-squared + Mann-Whitney)", tool_stats_kmers,
     {{"b", "maximal-bad-frequence"}}, {{"a-kmers", "A"}, {"b-kmers", "B"}, {"c-kmers", "C"}},
     {{"a-kmers", FILES}, {"b-kmers", FILES}, {"c-kmers", FILES}, PVALUES_, B_("frequence", "0"), OUT_("kmers")}},
    {"specific-kmers", "Output k-mers specific to groups of samples based on chi-squared & Mann-Whitney tests", tool_specific_kmers, {}, {{"a-kmers", "A"}, {"b-kmers", "B"}},
     {{"a-kmers", FILES}, {"b-kmers", FILES}, PVALUES_, OUT_("kmers")}},                                         // (SpecificKmersFinder.java:30-57: no maximal-bad-frequence)
    {"specific-kmers-3", "Output k-mers specific to each of three groups of samples based on chi-squared & Mann-Whitney tests", tool_specific_kmers3, {},
     {{"a-kmers", "A"}, {"b-kmers", "B"}, {"c-kmers", "C"}}, {{"a-kmers", FILES}, {"b-kmers", FILES}, {"c-kmers", FILES}, PVALUES_, OUT_("kmers")}},
    {"kmers-grouped-counter", "Count number of samples from 3 groups containing specified k-mers", tool_kmers_grouped_counter,              // KmersGroupedSamplesCounter.java:38-60
     {{"b", "maximal-bad-frequence"}, {"cd", "cd-kmers"}, {"uc", "uc-kmers"}, {"nonibd", "nonibd-kmers"}}, {{"k", "k"}, {"cd-kmers", "cd"}, {"uc-kmers", "uc"}, {"nonibd-kmers", "nonibd"}},
     {K_, {"kmers-file", FILES}, {"cd-kmers", FILES}, {"uc-kmers", FILES}, {"nonibd-kmers", FILES}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    {"kmers-per-sample", "Counts the abundance of frequent k-mers from dataset in each sample", tool_kmers_per_sample, {{"i", "k-mers"}, {"perc", "percent-present"}},   // KmersPerSampleCounter.java:43-48
     {{"k", "k"}, {"k-mers", "i"}}, {K_, {"k-mers", FILES}, {"percent-present", VAL, "20"}, OUT_("kmers_per_samples")}},
    {"unique-kmers", "Output k-mers present in one dataset and missing in other", tool_unique_kmers, {{"i", "k-mers"}, {"b", "maximal-bad-frequence"}},
     {{"k", "k"}, {"k-mers", "i"}, {"filter-kmers"}}, {K_, {"k-mers", FILES}, {"filter-kmers", FILES}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    {"unique-kmers-multi", "Output k-mers present in one dataset in fixed number of samples and missing in other", tool_unique_kmers_multi,
     {{"i", "k-mers"}, {"b", "maximal-bad-frequence"}}, {{"k", "k"}, {"k-mers", "i"}, {"filter-kmers"}},
     {K_, {"k-mers", FILES}, {"filter-kmers", FILES}, {"min-samples", VAL, "1"}, {"max-samples", VAL, "1"}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    {"kmers-multiple-filters", "Filter k-mers from test set according to three specified sets", tool_kmers_multiple_filters, {{"i", "k-mers"}, {"b", "maximal-bad-frequence"}},
     {{"k", "k"}, {"k-mers", "i"}, {"cd-filter-kmers", "cd"}, {"uc-filter-kmers", "uc"}, {"nonibd-filter-kmers", "nonibd"}},
     {K_, {"k-mers", FILES}, {"cd-filter-kmers", FILES}, {"uc-filter-kmers", FILES}, {"nonibd-filter-kmers", FILES}, B_("frequence", "1"), OUT_("kmers"), STATS_}},
    {"kmers-color", "Color k-mers based on their occurrences in three groups of samples", tool_kmers_color, {{"kf", "k-mers"}},                     // ColorKmersMain.java:39-43
     {{"k", "k"}, {"k-mers", "kf"}, {"class"}}, {K_, {"k-mers", FILES}, {"class", FILE1}, B_("frequency", "1"), {"val", FLAG}, OUT_("colored-kmers")}},
    {"component-colored", "Extract graph components from tangled graph based on k-mers coloring", tool_component_colored, {{"i", "k-mers"}}, {{"k", "k"}, {"k-mers", "i"}},
     {K_, {"k-mers", FILES}, {"n_groups", VAL, "3"}, {"separate", FLAG}, {"linear", FLAG}, {"n_comps", VAL, "-1"}, {"perc", VAL, "0.9"}, OUT_("colored-components")}},
    {"comp2seq", "Transforms components in binary format to FASTA sequences (contigs)", tool_comp2seq, {}, {{"components-file", "cf"}},
     {{"k", VAL, "31"}, {"components-file", FILE1}, {"split", FLAG}}},                                           // (ComponentsToSequences.java:21-26: k has a default)
    {"comp2graph", "Transforms components in binary format to de Bruijn graph in GFA format", tool_comp2graph, {{"i", "k-mers"}}, {{"k", "k"}, {"components-file", "cf"}},
     {K_, {"components-file", FILE1}, {"k-mers", FILES}, {"coverage", FLAG}, {"graph-file", FILE1, "$WD/components-graph.gfa"}}},
    {"seq2comp", "Transforms sequences to components", tool_seq2comp, {{"i", "sequences"}}, {{"k", "k"}, {"sequences", "i"}},
     {K_, {"sequences", FILES}, {"components-file", FILE1, "$WD/components.bin"}}},
    {"component-paths", "Extracts paths in the components", tool_component_paths, {{"cm", "components"}, {"l", "min-length"}},                          // ComponentPathsMain.java:52-71
     {{"k", "k"}, {"components-file", "cf"}, {"seq"}},
     {K_, {"components-file", FILE1}, {"seq", FILES}, {"components", LIST}, {"all-components", FLAG}, {"min-length", VAL, "50"}, OUT_("paths")}},
    {"view", "View different binary objects (k-mers files, components)", tool_view, {{"o", "output-file"}}, {},
     {K_, {"kmers-file", FILE1}, {"components-file", FILE1}, {"output-file", FILE1}}},
    {"bin2fasta", "Converts different binary objects to FASTA format", tool_bin2fasta, {{"o", "output-file"}}, {},
     {K_, {"kmers-file", FILE1}, {"components-file", FILE1}, {"output-file", FILE1}}},
    // matrix-builder: its own parameters, then the sub-tools' parameters it does not fix (Tool.addSubTool :168-207)
    {"matrix-builder", "Build the distance matrix for input sequences (default tool)", tool_matrix_builder, {}, {{"reads", "i"}},
     {{"k", VAL, "31"}, {"reads", FILES}, B_("frequency", "1"), {"min-seq-len", VAL, "100"}, {"use-reads-for-calculating-features", FLAG},
      {"matrix-file", DTFILE, "$WD/matrices/dist_matrix_$DT.txt"}, {"heatmap-file", DTFILE, "$WD/matrices/dist_matrix_$DT_heatmap.png"},
      {"stats-dir", FILE1, "$WD/kmer-counter-many/stats"}, {"bottom-cut-percent", VAL}, {"min-component-size", VAL, "1000"}, {"max-component-size", VAL, "10000"},
      {"selected", FILES}, {"without-names", FLAG}, {"output-format", VAL, "%.4f"}, {"colors-file", FILE1}, {"without-renumbering", FLAG}, {"invert-colors", FLAG}}},
};
static const Tool *find_tool(const string &name) { for (auto &t : TOOLS) if (name == t.name) return &t; return nullptr; }
static string tools_text() {                                // the -ts listing: the descriptions start in the fourth tab column
    string s;
    for (auto &t : TOOLS) s += string(t.name) + string(3 - strlen(t.name) / 8, '\t') + t.desc + "\n";
    return s;
}

static double since_start() {
    static struct timespec t0 = [] { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t; }();
    struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
    return (t.tv_sec - t0.tv_sec) + (t.tv_nsec - t0.tv_nsec) * 1e-9;
}
int main(int argc, char **argv) {
    since_start();
    string tool;
    Args a = parse_args(argc, argv, &tool);
    if (a.has("version")) { printf("MetaFast (MI355X HIP hot path) %s\n", mf_version()); return 0; }
    if (a.has("tools")) { printf("Available tools:\n%s", tools_text().c_str()); return 0; }
    if (a.has("help") || a.has("help-all")) {
        printf("Usage: metafast.sh [-t <tool>] [options]\n\nTools:\n%s\nLaunch options: -w/--work-dir <dir>  -p/--available-processors <n>  -c/--continue  --force  "
               "-s/--start <step>  -f/--finish <step>  -v/--verbose  --devices <a,b,...> (default: every visible device, twice where two libraries fit side by side; the per-library steps run one library per entry)  --device <n>\nTool options follow the reference (see SURVEY.md 8(b1)).\n", tools_text().c_str());
        return 0;
    }
    const Tool *t = find_tool(tool);
    if (!t) {
        fprintf(stderr, "ERROR: Tool '%s' not found !\n", tool.c_str());          // itmo!/Runner.java:136-139
        return 1;
    }
    g_verbose = a.flag("verbose");
    Env e;
    e.work_dir = a.get("work-dir", "workDir");
    e.start_ts = timestamp();
    const string wd = e.work_dir;
    mkdirs(wd); mkdirs(wd + "/logs");
    {   // Tool.updateFileLoggers :666-690: <workDir>/log (this run only) and <workDir>/logs/log_<ts>, same content
        time_t t = time(nullptr); struct tm tmv; localtime_r(&t, &tmv);
        char hdr[128]; strftime(hdr, sizeof hdr, "Log created at %d-%b-%Y (%a) %H:%M:%S", &tmv);
        g_logfile = fopen((wd + "/log").c_str(), "w");
        g_logfile2 = fopen((wd + "/logs/log_" + e.start_ts).c_str(), "w");
        for (FILE *f : {g_logfile, g_logfile2}) if (f) { fprintf(f, "%s\n", hdr); fflush(f); }
    }
    // ---- --continue / --force (Tool.run :400-462).  matrix-builder forces by default, unless -c or -s is given
    // (DistanceMatrixBuilderMain.java:23-26, 211-216).
    const bool builder = t->run == tool_matrix_builder;
    bool cont = a.flag("continue"), force = a.flag("force");
    if (builder) {
        if (a.has("force")) die("Cannot parse command line: Unrecognized option: --force");       // (removed from its launch options, :25)
        force = !(a.has("continue") || a.has("start"));
    }
    const string inprop = wd + "/in.properties";
    if (cont && force) die("Continue and force options can't be set simultaneously");
    if (exists(inprop)) {
        if (cont) {}
        else if (force) { if (!builder) logmsg("WARN", "Force run, all data in working directory will be rewritten!"); }
        else {
            fprintf(stderr, "Working directory (%s/) contains files from previous run, rewrite them? [Yes(y)/No(n), default:No] ", wd.c_str());
            char ans[64] = ""; if (!fgets(ans, sizeof ans, stdin)) ans[0] = 0;
            string s(ans); while (!s.empty() && isspace((unsigned char)s.back())) s.pop_back();
            for (auto &c : s) c = (char)tolower((unsigned char)c);
            if (s == "y" || s == "yes") force = true; else return 1;
        }
    } else force = true;
    e.cont = cont;
    // ---- runAsStep for the tool itself (:318-392)
    bool can = exists(inprop) && exists(wd + "/SUCCESS");
    if (!force) {
        Props stored;
        if (props_read(inprop, stored)) {
            // parameters not given on the command line take last run's values (loadUnsetParametersFromProperties :757-793)
            for (auto &kv : stored) if (!a.has(kv.first)) a.opt[kv.first] = kv.second;
            can = can && props_equal(tool_inputs(*t, a, wd, e.start_ts), stored);
        } else can = false;
    }
    // --wide-kmers goes to in.properties like a parameter where it is in effect (k > 31), so that -c and -s continue a wide workDir
    g_wide = a.flag("wide-kmers");
    // (stats-kmers declares no k and takes one with the flag: its wide run records k as well)
    const bool takes_k = !strcmp(t->name, "stats-kmers");
    const bool wide_run = g_wide && (t->param("k") || takes_k) && a.geti("k", 0) > 31;
    auto inputs = [&]() {
        vector<PV> v = tool_inputs(*t, a, wd, e.start_ts);
        if (wide_run && takes_k) v.push_back(PV("k", a.get("k")));
        if (wide_run) v.push_back(PV::flag("wide-kmers", true));
        return v;
    };
    Run r{e, a, *t, wd, a.get("start"), a.get("finish"), force, 0};
    if (!force && r.start.empty() && can) {
        logmsg("INFO", "SUCCESS file found for tool %s - loading results...", tool.c_str());
        return 0;
    }
    unlink((wd + "/SUCCESS").c_str()); unlink((wd + "/out.properties").c_str());
    r.k = r.num("k");
    // mandatory parameters are checked before anything is written (Tool.checkArguments :712-724)
    for (auto &n : t->needs) {
        if (!n.name) break;
        if (!a.has(n.name)) { if (n.sht) die("Mandatory argument --%s (-%s) not set", n.name, n.sht); else die("Mandatory argument --%s not set", n.name); }
    }
    props_write(inprop, inputs());
    const vector<PV> outs = t->run(r);
    const double t_work = since_start();
    for (mf_ctx *c : e.ctxs) if (c) mf_ctx_synchronize(c);
    if (r.finish.empty()) {                             // (a run cut short by --finish leaves no SUCCESS, :377-379)
        props_write(wd + "/out.properties", outs);
        touch(wd + "/SUCCESS");
    }
    if (g_logfile) fclose(g_logfile);
    if (g_logfile2) fclose(g_logfile2);
    if (getenv("MF_IO_TIMING")) fprintf(stderr, "[mf] driver: %.3f s until the last step was done\n", t_work);
    // every output is written and closed.  Handing hundreds of megabytes of pinned memory and the arena's regions back one by one, and
    // the HIP runtime's own shutdown after that, cost 0.2 s; the process ends here and the driver reclaims them with it
    // (MF_CLEAN_EXIT=1: the long way, for leak checkers)
    fflush(nullptr);
    if (getenv("MF_CLEAN_EXIT")) { for (mf_ctx *c : e.ctxs) if (c) mf_ctx_destroy(c); return 0; }
    _exit(0);
}
