// Host side shared by the GEMM families (gemm.hip: fp32 and f32x3; gemm_bf16.hip: bf16, per-row fp8, block-scaled fp8): the tile tables,
// the forced configuration of a family, the per-shape choices of the tuners and their text form, and the timer of the trial launches.
// Host code only; the process-wide state and the text codec are in gemm_tuner.hip.
#pragma once
#include "kernels.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace fern {

// ---- tile tables ------------------------------------------------------------------------------------------------------------------
struct TileCfg { int bm, bn, bk; float eff; };
// fp32 family.  order matters only for ties; eff = relative main-loop efficiency used by the shape heuristic
inline constexpr TileCfg kCfgs[] = {
    {128, 128, 32, 1.00f},   // 0: register-staged, 4 waves of 64x64
    {64, 128, 32, 0.93f},    // 1
    {128, 64, 32, 0.93f},    // 2
    {64, 64, 32, 0.86f},     // 3
    {0, 0, 0, 0.f}, {0, 0, 0, 0.f},   // 4-5: unused (retired A/B variants of the register-staged kernel)
    {64, 32, 64, 0.5f},      // 6: small-M kernel on the 16x16x4 MFMA (M <= 128, plain loader, no SR / patch epilogue)
    {0, 0, 0, 0.f},          // 7: unused
    {128, 128, 16, 1.00f},   // 8: LDS-DMA staging, 16-wide k tiles, double buffered
    {64, 128, 16, 0.93f},    // 9
    {128, 64, 16, 0.93f},    // 10
    {64, 64, 16, 0.86f},     // 11
    {256, 128, 16, 1.00f},   // 12: 8 waves, 256x128 macro-tile (0.75x the L2->LDS bytes per flop of 128x128), 2 workgroups per CU
    {128, 256, 16, 1.00f},   // 13
    // column counts that are not multiples of 64 (the ModifiedResNet's 80 / 160 / 320-channel layers: a 64- or 128-wide tile spends
    // 37.5 % / 17 % of its MFMAs on padding columns): four waves stacked over the rows, each 32 rows x the whole tile width
    {128, 96, 16, 1.00f},    // 14: wave tile 32x96
    {128, 160, 16, 1.00f},   // 15: wave tile 32x160
};
constexpr int kNumAuto = 4;      // configs the heuristic may pick
constexpr int kNumCfgs = 16;

// f32x3 family (GemmParams.split == 3).  The planes of a wave tile are 12 VGPRs per 32-row fragment, so the configurations trade
// occupancy for room: the 128x128 tile at <= 170 VGPRs (three workgroups per CU), the macro-tiles on four fat waves (wave tile 128x64 /
// 64x128, two workgroups per CU), and the small tiles at the usual 128.  All bit-identical to each other; tuned per shape like the fp32
// family.
// 6 (round 4): 256x256 on EIGHT fat waves (wave tile 128x64, one workgroup per CU).  The bf16 MFMAs of this family retire an fp32 k pair
// in 6 x 32 cycles instead of 2 x 64, so the tile's L2 -> LDS bytes are due 2.67x sooner than in the fp32 kernel: the 256x128 tile on
// four fat waves needs 32 B/clk per workgroup (two per CU: 64) of a path that delivers ~33 B/clk per CU -- copy-bound at about half the
// MFMA rate, which is the 1.5x the family measured.  256x256 stages 32 KiB per 3 072 MFMA cycles per SIMD: 10.7 B/clk.
constexpr int kNumCfgsS = 8;
inline constexpr TileCfg kCfgsS[kNumCfgsS] = {{128, 128, 16, 1.f}, {256, 128, 16, 1.f}, {128, 256, 16, 1.f}, {64, 128, 16, 1.f}, {128, 64, 16, 1.f}, {64, 64, 16, 1.f},
                                              {256, 256, 16, 1.f},
                                              // 7: operands split once per workgroup (gemm_f32x3_shared_kernel), 8 fat waves
                                              {256, 256, 16, 1.f}};

struct TileCfgB { int bm, bn, bk, per_cu; };     // per_cu: workgroups of the configuration one CU holds (LDS / registers / waves)
// bf16 family: the tuner's candidates.  Retired after A/B runs on MI355X: 3- and 4-stage rings of the 128x128 tile and
// 128x64 / 128x128 per-wave tiles -- fewer resident workgroups cost more than the deeper prefetch or the saved LDS reads gain.
inline constexpr TileCfgB kCfgsB[] = {
    {128, 128, 32, 4},   // 0: 4 waves of 64x64, 64-byte rows, 2 stages, 4 workgroups per CU
    {256, 128, 32, 2},   // 1: 8 waves of 64x64, 3 stages
    {256, 256, 32, 1},   // 2: 16 waves of 64x64, 3 stages
    {64, 128, 32, 4},    // 3: 4 waves of 32x64, 2 stages
    {128, 64, 32, 4},    // 4: 4 waves of 64x32, 2 stages
    {64, 64, 32, 8},     // 5: 4 waves of 32x32, 2 stages
    {128, 128, 64, 2},   // 6: as 0 with 128-byte rows (64-element k tiles): whole 128-byte lines per request, half the barriers, 2 per CU
    {256, 256, 32, 1},   // 7: round 6, gemm_pp.h: 8 waves of 128x64 in two groups half a phase apart, 4-slot ring of 64-byte-row k tiles (128 KiB)
    // round 6, the short-K shapes of the text tower / fusion BERT (M = 4928 / 5824, K = 512): with 32-element k tiles and ONE tile in
    // flight a 16-tile k loop is 16 L2 round trips -- every such GEMM took ~20 us whatever its size (129 TFLOP/s at N = 512).  128-byte
    // rows halve the round trips, the third stage keeps two tiles in flight
    {64, 64, 64, 3},     // 8: 4 waves of 32x32, 128-byte rows, 3 stages (48 KiB)
    {64, 128, 64, 2},    // 9: 4 waves of 32x64, 128-byte rows, 3 stages (72 KiB)
};
constexpr int kNumCfgsB = 10;
// fp8 tile family (k tile = 64 elements = 64-byte rows, 2 stages): same block shapes as the bf16 candidates
inline constexpr TileCfgB kCfgsF8[] = {{128, 128, 64, 4}, {256, 128, 64, 2}, {256, 256, 64, 1}, {64, 128, 64, 4}, {128, 64, 64, 4}, {64, 64, 64, 8}};
constexpr int kNumCfgsF8 = 6;
// MX tile family (k tile = 128 bytes).  LDS per stage = (bm + bn) * 132 bytes.
inline constexpr TileCfgB kCfgsMx[] = {
    {128, 128, 128, 2},   // 0: 4 waves of 64x64, 2 stages (66 KiB: 2 workgroups per CU)
    {256, 128, 128, 1},   // 1: 8 waves of 64x64, 2 stages (99 KiB)
    {256, 128, 128, 1},   // 2: 4 waves of 128x64, 2 stages: 12 LDS reads per 8 MFMAs instead of 8 per 4
    {128, 128, 128, 1},   // 3: as 0 with a 3-stage ring (99 KiB)
    {64, 128, 128, 3},    // 4: 4 waves of 32x64
    {128, 64, 128, 3},    // 5: 4 waves of 64x32
    {64, 64, 128, 4},     // 6: 4 waves of 32x32
    {256, 256, 128, 1},   // 7: 16 waves of 64x64, 2 stages (132 KiB)
    {128, 128, 64, 3},    // 8: as 0 with 64-byte rows (one MFMA step per barrier), 3 stages: 50 KiB, 3 workgroups per CU
    {256, 128, 64, 2},    // 9: as 1 with 64-byte rows, 3 stages: 75 KiB, 2 workgroups per CU (needs <= 128 VGPRs)
    {256, 256, 64, 1},    // 10: 8 waves of 128x64, 64-byte rows, 4 stages (136 KiB): fewest staged bytes per FLOP, deep prefetch instead of occupancy
    {256, 256, 64, 1},    // 11: round 6, gemm_pp.h: the ping-pong form of 10 (two wave groups half a phase apart, one 16 KiB unit staged per phase)
};
constexpr int kNumCfgsMx = 12;

// ---- the five families and their forced configuration ---------------------------------------------------------------------------------
// A forced tile configuration per family: the environment's value (read on first use) unless gemm_force_cfg has set one at run time
// (fern_tuner_force_config: the test suite walks every variant inside one process).
enum GemmFamily { FAM_F32, FAM_F32X3, FAM_BF16, FAM_FP8, FAM_MX8, kNumFamilies };
struct FamilyInfo {
    const char* name;      // fern_tuner_force_config's name of the family, and the kind of its lines in the text form
    const char* env;       // the variable that holds the forced configuration at start-up
    int ncfg;
    int kq;                // K must be a multiple of this whatever the configuration; 0: of the configuration's own k tile
};
inline constexpr FamilyInfo kFamilies[kNumFamilies] = {{"f32", "FERN_GEMM_CFG", kNumCfgs, 0},
                                                       {"f32x3", "FERN_GEMM_SPLIT_CFG", kNumCfgsS, 0},
                                                       {"bf16", "FERN_GEMM_BF16_CFG", kNumCfgsB, 0},
                                                       {"fp8", "FERN_GEMM_FP8_CFG", kNumCfgsF8, 64},
                                                       {"mx8", "FERN_GEMM_MX8_CFG", kNumCfgsMx, 128}};
int forced_cfg(int family);      // < 0: nothing forced
// the multiple of K that configuration `c` of a family needs; 0: `c` is no configuration of the family (out of range, retired slot)
inline int cfg_k_tile(int family, int c) {
    if (c < 0 || c >= kFamilies[family].ncfg) return 0;
    return family == FAM_F32 ? kCfgs[c].bk : family == FAM_F32X3 ? kCfgsS[c].bk : family == FAM_BF16 ? kCfgsB[c].bk : kFamilies[family].kq;
}
inline bool cfg_fits(int family, int c, int K) {
    const int kt = cfg_k_tile(family, c);
    return kt > 0 && K % kt == 0;
}
bool tuning_enabled();      // FERN_GEMM_TUNE != 0, read once per process
bool pair_enabled();        // FERN_GEMM_PAIR != 0, read once per process: the one-launch forms of both pair launchers

// ---- per-shape choices ----------------------------------------------------------------------------------------------------------
// Every configuration of a family accumulates each output element over k in the same order, so all of them produce bit-identical
// results: the choice is purely a speed choice.  Large problems are tuned once per shape by timing the candidates on scratch outputs.
struct ShapeKey {
    // tag: fp32 plans: loader + 1000 x ksplit; f32x3 plans: 0; fp32 / f32x3 pairs: loader / 3000; reduced precision: bit 0 = bf16 output,
    // bit 1 = fp8 operands, bit 2 = MX fp8 operands, bit 3 = MX fp8 output
    int M, N, K, epi, tag;
    bool operator<(const ShapeKey& o) const {
        if (M != o.M) return M < o.M;
        if (N != o.N) return N < o.N;
        if (K != o.K) return K < o.K;
        if (epi != o.epi) return epi < o.epi;
        return tag < o.tag;
    }
};
using PairKey = std::pair<ShapeKey, ShapeKey>;
// What the fp32 / f32x3 tuners pick for a shape: one tile configuration for the whole matrix, or -- plain row-independent epilogues only -- a
// BULK + REMAINDER pair: rows [0, rows_a) in configuration cfg, the rest in cfg_b.  rows_a is the largest row count whose tiles
// fill whole rounds of the 256 CUs; the ragged last round (e.g. 72 of 2 376 tiles at 12608 x 3072: every CU waits for the
// 72 that got a tenth tile) is recut into small tiles that spread over all CUs.  Every configuration produces bit-identical
// results, so the split changes nothing but the time.
// cfg 20 / 21: a MIXED plan (gemm_f32_mixed_kernel, macro-tile 256x128 / 128x256): rows [0, rows_a) in macro-tiles, [rows_a, cfg_b) in
// 128x128 tiles, [cfg_b, M) in 64x128 tiles, one launch -- cfg_b then holds a ROW, not a configuration.
struct Plan { int cfg, rows_a, cfg_b; };
constexpr int kCfgMixed = 20;
inline bool mixed_plan_ok(const Plan& pl, int M) {
    const int bma = pl.cfg == kCfgMixed + 1 ? 128 : 256;
    return (pl.cfg == kCfgMixed || pl.cfg == kCfgMixed + 1) && pl.rows_a > 0 && pl.rows_a <= M && pl.rows_a % bma == 0 && pl.cfg_b >= pl.rows_a &&
           pl.cfg_b <= M && (pl.cfg_b == M || (pl.cfg_b - pl.rows_a) % 128 == 0);
}

// The choices of this process, all under one mutex.  FERN_GEMM_TILES=<file of export lines> pins choices: listed shapes are never timed,
// so a run's kernels -- and its HBM / L2 traffic -- are reproducible from box to box; the file is read once, before the first look-up.
struct ChoiceStore {
    std::mutex mu;
    std::map<ShapeKey, Plan> f32, f32x3;      // f32x3: Plan{cfg, 0, cfg} or a mixed plan {20|21, ra, rb}
    std::map<PairKey, int> pair;              // launch_gemm_pair: 1 = the one-launch form beats two launches
    std::map<ShapeKey, int> rp;               // bf16 / fp8 / block-scaled fp8 configurations
    std::map<PairKey, int> pairb;             // launch_gemm_mxbf_pair: 0 = two launches, 1 / 2 = the pair kernel V = 0 / 1
    // Launches of other streams expected to run beside a reduced-precision GEMM (fern_tuner_set_concurrency; the query pipeline sets its
    // lane count).  1: a trial's score is its duration.  > 1: duration x (share of the chip's workgroup slots the launch fills)^0.75 --
    // a launch that leaves CUs to its neighbours is worth more to the pipeline than its own latency says.  Measured on the c5 pipeline
    // (3 lanes, tools/c5_tiles_ab.sh): 256x256 tiles for the N = 768 block GEMMs (150 workgroups on 150 CUs) instead of the 1 200
    // small workgroups the latency score picks: 17.7 -> 18.9 k queries/s, although each of those launches takes longer.
    int concurrency = 1;
};
ChoiceStore& choice_store();
void load_pinned_tiles();
int tuner_concurrency();

// The stored choice of `key`, or -- first sight of the shape -- what tune(tuned) times, all under the store's lock: tune() launches
// kernels of its own family only.  tuned == false: nothing was timed (the stream is being captured, no scratch memory, tuning off) and
// tune() returned its fallback, which is NOT stored: the shape would stay on the untuned choice (and be exported as a tuned one) for good.
template <class V, class Fn>
V lookup_or_tune(std::map<ShapeKey, V>& map, const ShapeKey& key, Fn&& tune) {
    load_pinned_tiles();
    ChoiceStore& st = choice_store();
    std::lock_guard<std::mutex> lock(st.mu);
    const auto it = map.find(key);
    if (it != map.end()) return it->second;
    bool tuned = false;
    const V v = tune(tuned);
    if (tuned) map.emplace(key, v);
    return v;
}
// The pair launchers' form of it: their trials call back into launch_gemm / launch_gemm_bf16, which take the lock themselves (and tune
// the single shapes on first sight), so no lock is held while tune() runs.
template <class Fn>
int lookup_or_tune_pair(std::map<PairKey, int>& map, const PairKey& key, Fn&& tune) {
    load_pinned_tiles();
    ChoiceStore& st = choice_store();
    {
        std::lock_guard<std::mutex> lock(st.mu);
        const auto it = map.find(key);
        if (it != map.end()) return it->second;
    }
    bool timed = false;
    const int v = tune(timed);
    if (timed) {
        std::lock_guard<std::mutex> lock(st.mu);
        map[key] = v;
    }
    return v;
}

extern thread_local int g_last_dispatches;      // kernel dispatches of the calling thread's last launch_gemm* (gemm_last_dispatches)

// ---- trial launches ---------------------------------------------------------------------------------------------------------------
// One tuner run: the launch timer of an instrumented pass is paused (trial launches are not part of the launch being timed), the
// stream must not be capturing (trials cannot be timed inside a capture), scratch outputs and an event pair live as long as the run.
// A timer that is not ok() times nothing: its tuner returns the fallback, uncached.
class TrialTimer {
public:
    explicit TrialTimer(hipStream_t s) : s_(s) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        ok_ = hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
        if (ok_) ok_ = hipEventCreate(&e0_) == hipSuccess && hipEventCreate(&e1_) == hipSuccess;
    }
    TrialTimer(const TrialTimer&) = delete;
    TrialTimer& operator=(const TrialTimer&) = delete;
    ~TrialTimer() {
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
        for (void* p : scratch_) (void)hipFree(p);
    }
    bool ok() const { return ok_; }
    // a scratch buffer the trials may write to, freed with the timer; nullptr (and the timer unusable) when there is no memory for it
    void* scratch(size_t bytes) {
        void* p = nullptr;
        if (!ok_) return nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            ok_ = false;
            return nullptr;
        }
        scratch_.push_back(p);
        return p;
    }
    // The fastest of `rounds` windows of `reps` launches, each window after one warm launch; 1e30f when a launch or the synchronise fails.
    // More than one window because the first launches after an idle spell run while the clocks are still ramping.
    template <class Fn>
    float best_ms(Fn&& fn, int rounds, int reps) {
        float best = 1e30f;
        for (int round = 0; ok_ && round < rounds; ++round) {
            if (fn() != hipSuccess) return 1e30f;      // warm
            (void)hipEventRecord(e0_, s_);
            for (int i = 0; i < reps; ++i) (void)fn();
            (void)hipEventRecord(e1_, s_);
            if (hipEventSynchronize(e1_) != hipSuccess) return 1e30f;
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0_, e1_);
            best = std::min(best, ms);
        }
        return best;
    }

private:
    LaunchTimerPause pause_;
    hipStream_t s_;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
    bool ok_ = false;
    std::vector<void*> scratch_;
};

}  // namespace fern
