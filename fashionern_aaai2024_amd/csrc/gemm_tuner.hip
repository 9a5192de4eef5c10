// The process-wide state of the GEMM tuners (gemm_tuner.h) and its text form: forced configurations, the choice store, the lines of
// fern_tuner_export / fern_tuner_import / FERN_GEMM_TILES.  Host code only: nothing here touches a device.
#include "gemm_tuner.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace fern {

// ---- forced configurations, switches ----------------------------------------------------------------------------------------------
static std::atomic<int> g_force[kNumFamilies] = {{-2}, {-2}, {-2}, {-2}, {-2}};      // -2 = the environment's value, not read yet
int forced_cfg(int family) {
    int v = g_force[family].load(std::memory_order_relaxed);
    if (v == -2) {
        const char* e = getenv(kFamilies[family].env);
        v = e ? atoi(e) : -1;
        g_force[family].store(v, std::memory_order_relaxed);
    }
    return v;
}
bool gemm_force_cfg(const char* family, int cfg) {      // cfg < 0: back to the environment's value
    for (int f = 0; family && f < kNumFamilies; ++f)
        if (!strcmp(family, kFamilies[f].name)) {
            g_force[f].store(cfg < 0 ? -2 : cfg, std::memory_order_relaxed);
            return true;
        }
    return false;
}
static bool env_switch_on(const char* var) {
    const char* e = getenv(var);
    return !(e && e[0] == '0');
}
bool tuning_enabled() {
    static const bool on = env_switch_on("FERN_GEMM_TUNE");
    return on;
}
bool pair_enabled() {
    static const bool on = env_switch_on("FERN_GEMM_PAIR");
    return on;
}

thread_local int g_last_dispatches = 1;
int gemm_last_dispatches() { return g_last_dispatches; }

ChoiceStore& choice_store() {
    static ChoiceStore st;
    return st;
}
void gemm_tuner_set_concurrency(int n) {
    ChoiceStore& st = choice_store();
    std::lock_guard<std::mutex> lock(st.mu);
    st.concurrency = n < 1 ? 1 : n;
}
int tuner_concurrency() {
    ChoiceStore& st = choice_store();
    std::lock_guard<std::mutex> lock(st.mu);
    return st.concurrency;
}

// ---- text form ------------------------------------------------------------------------------------------------------------------
// One line per choice, a kind and up to 11 integers:
//   f32   M N K epi aload cfg [rows_a cfg_b]           aload: the loader + 1000 x ksplit
//   f32x3 M N K epi cfg [rows_a cfg_b]                 (no loader field: the family has the plain loader only)
//   pair  M1 N1 K1 epi1 a1 M2 N2 K2 epi2 a2 one        a = aload, 3000 for the f32x3 family
//   bf16 | fp8 | mx8  M N K epi ob cfg                 ob: the key's tag bits (ShapeKey)
//   pairb M1 N1 K1 epi1 ob1 M2 N2 K2 epi2 ob2 choice   a (block-scaled, bf16) pair of shapes
// A line that names no kind, has too few numbers or fails its kind's check is skipped; numbers past a kind's last field are ignored.
static ShapeKey key_at(const int* v) { return ShapeKey{v[0], v[1], v[2], v[3], v[4]}; }

static void accept_f32(ChoiceStore& st, const int* v, int n) {
    const int M = v[0], K = v[2], cfg = v[5];
    Plan pl{cfg, 0, cfg};
    if (n == 8 && cfg >= kCfgMixed) {      // a mixed plan
        pl = Plan{cfg, v[6], v[7]};
        if (!mixed_plan_ok(pl, M) || K % 16 != 0) return;
    } else {
        if (!cfg_fits(FAM_F32, cfg, K)) return;
        // bulk + remainder; a remainder that cannot run degrades the line to the single configuration
        if (n == 8 && v[6] > 0 && v[6] < M && cfg_fits(FAM_F32, v[7], K)) pl = Plan{cfg, v[6], v[7]};
    }
    st.f32[key_at(v)] = pl;
}
static void accept_f32x3(ChoiceStore& st, const int* v, int n) {
    const int cfg = v[4];
    Plan pl{cfg, 0, cfg};
    if (cfg_k_tile(FAM_F32X3, cfg) == 0) {      // not a single configuration: a mixed plan, which wants all three numbers
        pl = Plan{cfg, v[5], v[6]};
        if (n != 7 || !mixed_plan_ok(pl, v[0])) return;
    }
    st.f32x3[ShapeKey{v[0], v[1], v[2], v[3], 0}] = pl;
}
static void accept_pair(ChoiceStore& st, const int* v, int) { st.pair[{key_at(v), key_at(v + 5)}] = v[10] != 0; }
static void accept_pairb(ChoiceStore& st, const int* v, int) {
    if (v[10] >= 0 && v[10] <= 2) st.pairb[{key_at(v), key_at(v + 5)}] = v[10];
}
// The LAUNCH family of a reduced-precision shape is selected by the tag bits of its key (bit 1: per-row fp8, bit 2: block-scaled fp8), so
// the family the configuration index is checked against comes from the tag, and a line whose kind disagrees with it is dropped (an mx8
// configuration pinned under a bf16 key would fail every launch of that shape).
static int rp_family(int tag) { return (tag & 4) ? FAM_MX8 : (tag & 2) ? FAM_FP8 : FAM_BF16; }
template <int FAMILY>
static void accept_rp(ChoiceStore& st, const int* v, int) {
    if (rp_family(v[4]) != FAMILY || v[0] <= 0 || v[1] <= 0 || v[2] <= 0 || !cfg_fits(FAMILY, v[5], v[2])) return;
    st.rp[key_at(v)] = v[5];
}

struct LineKind {
    const char* name;
    int min_fields, max_fields;      // integers after the kind: fewer refuse the line, more are ignored
    void (*accept)(ChoiceStore& st, const int* v, int n);      // checks the n fields read and stores the choice; the caller holds st.mu
};
static const LineKind kLineKinds[] = {{"f32", 6, 8, accept_f32},
                                      {"f32x3", 5, 7, accept_f32x3},
                                      {"pair", 11, 11, accept_pair},
                                      {"bf16", 6, 6, accept_rp<FAM_BF16>},
                                      {"fp8", 6, 6, accept_rp<FAM_FP8>},
                                      {"mx8", 6, 6, accept_rp<FAM_MX8>},
                                      {"pairb", 11, 11, accept_pairb}};

static void read_line(ChoiceStore& st, const char* line) {      // caller holds st.mu
    char kind[16];
    int used = 0;
    if (sscanf(line, "%15s%n", kind, &used) != 1) return;
    for (const LineKind& k : kLineKinds) {
        if (strcmp(kind, k.name)) continue;
        int v[11] = {}, n = 0;
        const char* at = line + used;
        for (int adv = 0; n < k.max_fields && sscanf(at, "%d%n", &v[n], &adv) == 1; at += adv) ++n;
        // the optional fields of a plan come as a pair: with one of them missing the line is its short form
        if (n > k.min_fields && n < k.max_fields) n = k.min_fields;
        if (n >= k.min_fields) k.accept(st, v, n);
        return;
    }
}
static void write_line(std::string& out, const char* kind, std::initializer_list<int> fields) {
    out += kind;
    for (int f : fields) out += ' ' + std::to_string(f);
    out += '\n';
}

void load_pinned_tiles() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char* path = getenv("FERN_GEMM_TILES");
        FILE* f = path ? fopen(path, "r") : nullptr;
        if (!f) return;
        char line[256];
        ChoiceStore& st = choice_store();
        std::lock_guard<std::mutex> lock(st.mu);
        while (fgets(line, sizeof line, f)) read_line(st, line);
        fclose(f);
    });
}
// fern_tuner_import: the lines of another process's fern_tuner_export replace this process's choices for the listed shapes
// (rank 0 tunes, every rank runs rank 0's kernels: no rank-to-rank tile skew in a max-over-ranks step time)
void gemm_tuner_import(const std::string& text) {
    load_pinned_tiles();
    ChoiceStore& st = choice_store();
    std::lock_guard<std::mutex> lock(st.mu);
    for (size_t at = 0; at < text.size();) {
        size_t nl = text.find('\n', at);
        if (nl == std::string::npos) nl = text.size();
        read_line(st, text.substr(at, nl - at).c_str());
        at = nl + 1;
    }
}
void gemm_tuner_export(std::string& out) {
    ChoiceStore& st = choice_store();
    std::lock_guard<std::mutex> lock(st.mu);
    for (const auto& [k, pl] : st.f32x3) write_line(out, "f32x3", {k.M, k.N, k.K, k.epi, pl.cfg, pl.rows_a, pl.cfg_b});
    for (const auto& [k, pl] : st.f32) write_line(out, "f32", {k.M, k.N, k.K, k.epi, k.tag, pl.cfg, pl.rows_a, pl.cfg_b});
    for (const auto& [k, one] : st.pair)
        write_line(out, "pair", {k.first.M, k.first.N, k.first.K, k.first.epi, k.first.tag, k.second.M, k.second.N, k.second.K, k.second.epi, k.second.tag, one});
    for (const auto& [k, cfg] : st.rp) write_line(out, kFamilies[rp_family(k.tag)].name, {k.M, k.N, k.K, k.epi, k.tag, cfg});
    for (const auto& [k, choice] : st.pairb)
        write_line(out, "pairb", {k.first.M, k.first.N, k.first.K, k.first.epi, k.first.tag, k.second.M, k.second.N, k.second.K, k.second.epi, k.second.tag, choice});
}

}  // namespace fern
