// Exact target ranks (include/fern.h: fern_rank_keys / fern_rank_count): everything but the fp32 counting sweep itself, which is the
// EPI_RANK_COUNT epilogue of the LDS-DMA GEMM (gemm_epilogue.h: rank_count_epilogue).
//   rank_keys_kernel            the ranking key of named gallery rows, fp32 form: the sweep's fma chain on gathered rows
//   rank_gather_bf16_kernel /   bf16 form: the targets' rows become a small gallery that the bf16 sweep itself scores (same MFMA
//   rank_keys_scores_kernel     sequence, same k order, so the same bits), the keys are then read off its score rows
//   rank_count_rows_kernel      bf16 form: counting over the score rows the bf16 sweep stored
//   rank_finalize_kernel        sum of the partial counter sets, -1 for a target without a key
#include "kernels.h"
#include "rescore.h"

#include <algorithm>

namespace fern {

constexpr int RK_T = CHAIN_T;            // targets per wave
constexpr int RK_CH = 256;               // k per step: one 16-byte load per lane and row

__device__ __forceinline__ long rank_local_row(int target, long idx_offset, long N) {      // -1: not a row of this gallery
    const long r = (long)target - idx_offset;
    return (target >= 0 && r >= 0 && r < N) ? r : -1;
}

// One wave per (query, 16 targets): the per-lane chain stager (rescore.h: chain_rows_lane) at 256 k per step -- one load per lane and
// row, all 17 in flight behind one wait; lane t < 16 ends up with target t's chain in the sweep's order.
__global__ __launch_bounds__(64) void rank_keys_kernel(const float* q, const float* gallery, const int* targets, int B, long N, int D, int m,
                                                       long idx_offset, u64* keys) {
    __shared__ __attribute__((aligned(16))) float tile[chain_tile_floats<RK_CH>()];
    const int b = blockIdx.x, t0 = blockIdx.y * RK_T, lane = threadIdx.x;
    const int nt = min(RK_T, m - t0);
    const int* tg = targets + (long)b * m + t0;
    const float acc = chain_rows_lane<RK_CH>(
        [&](int t) {
            const long r = t < nt ? rank_local_row(tg[t], idx_offset, N) : -1;
            return gallery + (r < 0 ? 0 : r) * D;            // (a target without a row reads row 0; its key is 0 below)
        },
        q + (long)b * D, D, tile);
    if (lane < nt) {
        const int t = tg[lane];
        keys[(long)b * m + t0 + lane] = rank_local_row(t, idx_offset, N) >= 0 ? make_key(acc, (unsigned)t) : 0ull;
    }
}

// rows[i] = bf16 gallery row of target i (row 0 for a target without a row): one wave per row, 16 bytes per lane and step
__global__ __launch_bounds__(256) void rank_gather_bf16_kernel(const unsigned short* gallery, const int* targets, long count, long N, int D,
                                                               long idx_offset, unsigned short* rows) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= count) return;
    const long r = rank_local_row(targets[i], idx_offset, N);
    const uint4* src = reinterpret_cast<const uint4*>(gallery + (r < 0 ? 0 : r) * D);
    uint4* dst = reinterpret_cast<uint4*>(rows + i * D);
    for (int c = lane; c < D / 8; c += 64) dst[c] = src[c];
}

__global__ __launch_bounds__(256) void rank_keys_scores_kernel(const float* S, long ld, const int* targets, int B, long N, int m, long idx_offset,
                                                               u64* keys) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * m) return;
    const long b = i / m, j = i % m;
    const int t = targets[i];
    keys[i] = rank_local_row(t, idx_offset, N) >= 0 ? make_key(S[b * ld + (b & 63) * m + j], (unsigned)t) : 0ull;
}

// Stored score rows S [B, ld]: blockIdx.y = query, the workgroups of a query stride over its row.  Per-lane counts, one wave sum per
// target at the end, one add per wave and target into the partial set of the wave.
__global__ __launch_bounds__(256) void rank_count_rows_kernel(const float* S, long ld, long N, RankCount rc, int B) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    u64 tk[RANKC_T];
#pragma unroll
    for (int t = 0; t < RANKC_T; ++t) tk[t] = t < rc.nt ? rc.keys[(long)b * rc.kstride + t] : ~0ull;
    const long ex = excluded_local_row(rc.exclude, b, rc.exclude_off, N);
    // a per-query row filter (kernels.h: RowTags): the sweep stored its ineligible rows as -inf; they carry key 0 here like the excluded row
    const bool tagged = rc.rt.tags != nullptr;
    const QueryTags qt = query_tags(rc.rt, b);
    int cnt[RANKC_T];
#pragma unroll
    for (int t = 0; t < RANKC_T; ++t) cnt[t] = 0;
    const float* row = S + (long)b * ld;
    for (long n = (long)blockIdx.x * 256 + tid; n < N; n += (long)gridDim.x * 256) {
        // (not stored_row_key: a row that scores -inf of its own counts here as it does in the fp32 form's epilogue, which sees no stored row)
        const bool ok = n != ex && (!tagged || row_eligible(rc.rt.tags[n], qt.mask, qt.value));
        const u64 key = ok ? make_key(row[n], (unsigned)(n + rc.idx_offset)) : 0ull;
#pragma unroll
        for (int t = 0; t < RANKC_T; ++t) cnt[t] += key > tk[t] ? 1 : 0;
    }
    int* part = rc.partial + (long)((blockIdx.x * 4 + (tid >> 6)) & (RANKC_P - 1)) * B * RANKC_T + (long)b * RANKC_T;
#pragma unroll
    for (int t = 0; t < RANKC_T; ++t) {
        const int v = wave_sum_i32(cnt[t]);
        if (lane == 0 && t < rc.nt && v != 0) atomicAdd(&part[t], v);
    }
}

__global__ __launch_bounds__(256) void rank_finalize_kernel(RankCount rc, int B, int* count, int cstride) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * rc.nt) return;
    const int b = i / rc.nt, t = i % rc.nt;
    int sum = 0;
    for (int p = 0; p < RANKC_P; ++p) sum += rc.partial[((long)p * B + b) * RANKC_T + t];
    count[(long)b * cstride + t] = rc.keys[(long)b * rc.kstride + t] ? sum : -1;
}

hipError_t launch_rank_keys(const float* q, const float* gallery, const int* targets, int B, long N, int D, int m, long idx_offset,
                            unsigned long long* keys, hipStream_t s) {
    if (B <= 0 || m <= 0) return hipSuccess;
    if (D <= 0 || D % 8) return hipErrorInvalidValue;
    if (N <= 0) return hipMemsetAsync(keys, 0, (size_t)B * m * sizeof(u64), s);
    FERN_LAUNCH(rank_keys_kernel, dim3((unsigned)B, (unsigned)((m + RK_T - 1) / RK_T)), dim3(64), 0, s, q, gallery, targets, B, N, D, m, idx_offset, keys);
    return hipGetLastError();
}

hipError_t launch_rank_gather_bf16(const unsigned short* gallery, const int* targets, long count, long N, int D, long idx_offset,
                                   unsigned short* rows, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (N <= 0 || D <= 0 || D % 8) return hipErrorInvalidValue;
    FERN_LAUNCH(rank_gather_bf16_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, gallery, targets, count, N, D, idx_offset, rows);
    return hipGetLastError();
}

hipError_t launch_rank_keys_from_scores(const float* S, long ld, const int* targets, int B, long N, int m, long idx_offset,
                                        unsigned long long* keys, hipStream_t s) {
    if (B <= 0 || m <= 0) return hipSuccess;
    FERN_LAUNCH(rank_keys_scores_kernel, dim3((unsigned)(((long)B * m + 255) / 256)), dim3(256), 0, s, S, ld, targets, B, N, m, idx_offset, keys);
    return hipGetLastError();
}

hipError_t launch_rank_count_rows(const float* S, long ld, int B, long N, const RankCount& rc, hipStream_t s) {
    if (B <= 0 || N <= 0) return hipSuccess;
    if (rc.nt < 1 || rc.nt > RANKC_T || !rc.partial) return hipErrorInvalidValue;
    // ~4096 rows per workgroup (16 per lane), at most 64 workgroups per query
    const unsigned gx = (unsigned)std::min<long>(64, std::max<long>(1, (N + 4095) / 4096));
    FERN_LAUNCH(rank_count_rows_kernel, dim3(gx, (unsigned)B), dim3(256), 0, s, S, ld, N, rc, B);
    return hipGetLastError();
}

hipError_t launch_rank_finalize(const RankCount& rc, int B, int* count, int cstride, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (rc.nt < 1 || rc.nt > RANKC_T || !rc.partial) return hipErrorInvalidValue;
    FERN_LAUNCH(rank_finalize_kernel, dim3((unsigned)((B * rc.nt + 255) / 256)), dim3(256), 0, s, rc, B, count, cstride);
    return hipGetLastError();
}

}  // namespace fern
