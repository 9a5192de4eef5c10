// Item-level ranking (include/fern.h: fern_sim_topk_items, fern_item_rank): galleries whose rows belong to items.
//
// The gallery carries one int32 item id per row, items[N]; G is the number of items.  The item-level ranking of a query is its exact row
// ranking (score descending, global row index ascending; exclude_idx and the row filter applied first) with every row that is not the
// FIRST row of its item removed: an item is represented by its best eligible row.  The stage works on the deep stage's stored score rows
// S [m, ld] (topk_deep.hip) and a table best [m, G] of 64-bit ranking keys (kernels.h: make_key on the GLOBAL row index), zero = no row:
//   item_best_kernel       best[b][items[n]] = max(best, key(S[b][n], n + idx_offset)) over the rows that can represent an item for
//                          query b (item_quad below).  Items are mostly runs of consecutive rows, so a wave reduces the runs inside its 256
//                          rows with a segmented max (in the lane's four rows, then a segmented scan over the 64 lanes) and issues one
//                          64-bit atomicMax per (wave, run), not one per row;
//   item_keep_best_kernel  S[b][n] = -inf unless key(S[b][n], n + idx_offset) == best[b][items[n]]: the key holds the row index, so exactly
//                          one row per non-empty item survives.  launch_deep_select / launch_deep_fallback then rank the rows unchanged
//                          (they give -inf rows no place and break ties by row index);
//   item_gather_kernel     out_item[b][k] = items[out_idx[b][k] - idx_offset], -1 for an unfilled place;
//   item_keys_kernel, item_count_kernel   a place is a count over the table: #{g : best[b][g] > best[b][t]}; no selection is needed.
// Rows whose id is outside [0, G) belong to no item: they carry key 0 everywhere and never index the table.
#include "kernels.h"
#include "wave.h"

#include <algorithm>
#include <cstdint>

namespace fern {

typedef int i32x4i __attribute__((ext_vector_type(4)));

constexpr int ITEM_NT = 256;                    // threads per workgroup: four waves, 256 rows per wave and step
constexpr int ITEM_T = 8;                       // targets per pass of the count kernel over a query's table

// Rows i .. i + 3 (i % 4 == 0, i < ld) of query b: v = the stored scores, g = the item id (-1: outside [0, G) or past the gallery), k = the
// ranking key, 0 unless the row can represent its item for this query: the row-key rule (kernels.h: stored_row_key -- inside the
// gallery, not the excluded row, a score above -inf) and, as conditions of this stage, an id inside [0, G) and a row that is eligible
// under the row filter (applied here again, not only through the -inf the score producers store).
__device__ __forceinline__ void item_quad(const ItemRows& r, const float* row, long i, long drop, QueryTags qt, f32x4& v, u64 (&k)[4], int (&g)[4]) {
    v = *reinterpret_cast<const f32x4*>(row + i);
    int id[4];
    if (r.aligned && i + 3 < r.N) {
        const i32x4i t = *reinterpret_cast<const i32x4i*>(r.items + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) id[e] = t[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) id[e] = i + e < r.N ? r.items[i + e] : -1;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long n = i + e;
        const bool in = n < r.N && (unsigned)id[e] < (unsigned)r.G;
        u64 key = in ? stored_row_key(v[e], n, r.N, drop, r.idx_offset) : 0ull;
        if (r.rt.tags && key != 0 && !row_eligible(r.rt.tags[n], qt.mask, qt.value)) key = 0ull;
        g[e] = in ? id[e] : -1;
        k[e] = key;
    }
}

// Workgroup (x, b): wave w takes the 256-row steps 4 x + w + j * 4 gridDim.x of query b's score row; lane l rows 4 l .. 4 l + 3 of a step.
__global__ __launch_bounds__(ITEM_NT) void item_best_kernel(const float* S, long ld, ItemRows r, u64* best) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* row = S + (long)b * ld;
    u64* bb = best + (long)b * r.G;
    const long drop = excluded_local_row(r.exclude, b, r.idx_offset, r.N);
    const QueryTags qt = query_tags(r.rt, b);
    const long nq = (r.N + 3) & ~3L;
    for (long base = ((long)blockIdx.x * 4 + wave) * 256; base < nq; base += (long)gridDim.x * 1024) {      // (wave-uniform)
        const long i = base + lane * 4;
        f32x4 v;
        u64 k[4] = {0ull, 0ull, 0ull, 0ull};
        int g[4] = {-1, -1, -1, -1};
        if (i < nq) item_quad(r, row, i, drop, qt, v, k, g);
        // runs inside the lane: the LAST row of a run ends up with the run's maximum
#pragma unroll
        for (int e = 1; e < 4; ++e)
            if (g[e] == g[e - 1]) k[e] = k[e] > k[e - 1] ? k[e] : k[e - 1];
        const bool uni = g[0] == g[1] && g[1] == g[2] && g[2] == g[3];
        const int gprev = __shfl_up(g[3], 1), gnext = __shfl_down(g[0], 1);
        const bool joins_prev = lane > 0 && g[0] >= 0 && g[0] == gprev;       // the lane's first run continues the previous lane's last run
        const bool joins_next = lane < 63 && g[3] >= 0 && g[3] == gnext;      // ... and its last run goes on in the next lane, which issues it
        // segmented inclusive max scan of the lanes' last-run maxima: a lane opens a segment unless it is ONE run that continues its neighbour's
        u64 sv = k[3];
        int sf = !(uni && joins_prev);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 pv = shfl_up64(sv, d);
            const int pf = __shfl_up(sf, d);
            if (lane >= d) {
                if (!sf && pv > sv) sv = pv;
                sf |= pf;
            }
        }
        const u64 cin = shfl_up64(sv, 1);      // what the run the lane continues has gathered so far
        bool first = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool tail = e == 3 || g[e] != g[e + (e < 3 ? 1 : 0)];
            if (!tail) continue;
            u64 key = k[e];
            if (e == 3 && uni) key = sv;
            else if (first && joins_prev && cin > key) key = cin;
            first = false;
            if (e == 3 && joins_next) continue;
            if (key != 0 && (unsigned)g[e] < (unsigned)r.G) atomicMax(&bb[g[e]], key);
        }
    }
}

__global__ __launch_bounds__(ITEM_NT) void item_keep_best_kernel(float* S, long ld, ItemRows r, const u64* best) {
    const int b = blockIdx.y;
    float* row = S + (long)b * ld;
    const u64* bb = best + (long)b * r.G;
    const long drop = excluded_local_row(r.exclude, b, r.idx_offset, r.N);
    const QueryTags qt = query_tags(r.rt, b);
    const long nq = (r.N + 3) & ~3L;
    for (long i = ((long)blockIdx.x * ITEM_NT + threadIdx.x) * 4; i < nq; i += (long)gridDim.x * ITEM_NT * 4) {
        f32x4 v;
        u64 k[4];
        int g[4];
        item_quad(r, row, i, drop, qt, v, k, g);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (k[e] != 0 && k[e] == bb[g[e] >= 0 ? g[e] : 0]) ? v[e] : -INFINITY;
        *reinterpret_cast<f32x4*>(row + i) = o;
    }
}

__global__ __launch_bounds__(ITEM_NT) void item_gather_kernel(const int* idx, long count, const int* items, long N, int G, long idx_offset, int* out_item) {
    const long t = (long)blockIdx.x * ITEM_NT + threadIdx.x;
    if (t >= count) return;
    const long n = (long)idx[t] - idx_offset;
    int id = -1;
    if (idx[t] >= 0 && n >= 0 && n < N) id = items[n];
    out_item[t] = (unsigned)id < (unsigned)G ? id : -1;
}

// keys[b][j] = best[b][targets[b][j]], 0 for an id outside [0, G)
__global__ __launch_bounds__(ITEM_NT) void item_keys_kernel(const u64* best, int G, const int* targets, long count, int m, u64* keys) {
    const long t = (long)blockIdx.x * ITEM_NT + threadIdx.x;
    if (t >= count) return;
    const int id = targets[t];
    keys[t] = (unsigned)id < (unsigned)G ? best[(t / m) * G + id] : 0ull;
}

// Workgroup (b, y): targets 8 y .. 8 y + 7 of query b; out[b][j] = #{g : best[b][g] > keys[b][j]}, -1 for a key of 0
__global__ __launch_bounds__(ITEM_NT) void item_count_kernel(const u64* best, int G, const u64* keys, int m, int* out) {
    __shared__ int part[ITEM_NT / 64][ITEM_T];
    const int b = blockIdx.x, t0 = blockIdx.y * ITEM_T, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64* bb = best + (long)b * G;
    u64 key[ITEM_T];
    int cnt[ITEM_T];
#pragma unroll
    for (int t = 0; t < ITEM_T; ++t) {
        key[t] = t0 + t < m ? keys[(long)b * m + t0 + t] : ~0ull;
        cnt[t] = 0;
    }
    for (int g = tid; g < G; g += ITEM_NT) {
        const u64 v = bb[g];
#pragma unroll
        for (int t = 0; t < ITEM_T; ++t) cnt[t] += v > key[t] ? 1 : 0;
    }
#pragma unroll
    for (int t = 0; t < ITEM_T; ++t) {
        const int c = wave_sum_i32(cnt[t]);
        if (lane == 0) part[wave][t] = c;
    }
    __syncthreads();
    if (tid < ITEM_T && t0 + tid < m) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < ITEM_NT / 64; ++w) sum += part[w][tid];
        out[(long)b * m + t0 + tid] = keys[(long)b * m + t0 + tid] != 0 ? sum : -1;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
static bool item_rows_ok(const ItemRows& r, long ld) {
    if (r.N < 0 || r.G < 1 || (ld & 3) || ld < ((r.N + 3) & ~3L) || (r.N > 0 && !r.items)) return false;
    RowTags rt;
    return row_tags_arg(&r.rt, rt);
}
static ItemRows item_rows_aligned(ItemRows r) {
    r.aligned = (reinterpret_cast<uintptr_t>(r.items) & 15) == 0;
    return r;
}
static dim3 item_grid(long N, int B) {
    const long steps = (N + 1023) / 1024;
    return dim3((unsigned)std::max<long>(1, std::min<long>(steps, std::max(1, 4096 / B))), (unsigned)B);
}

hipError_t launch_item_best(const float* S, long ld, int B, const ItemRows& r, unsigned long long* best, hipStream_t s) {
    if (B <= 0 || r.N == 0) return hipSuccess;
    if (!S || !best || !item_rows_ok(r, ld)) return hipErrorInvalidValue;
    FERN_LAUNCH(item_best_kernel, item_grid(r.N, B), dim3(ITEM_NT), 0, s, S, ld, item_rows_aligned(r), best);
    return hipGetLastError();
}

hipError_t launch_item_keep_best(float* S, long ld, int B, const ItemRows& r, const unsigned long long* best, hipStream_t s) {
    if (B <= 0 || r.N == 0) return hipSuccess;
    if (!S || !best || !item_rows_ok(r, ld)) return hipErrorInvalidValue;
    FERN_LAUNCH(item_keep_best_kernel, item_grid(r.N, B), dim3(ITEM_NT), 0, s, S, ld, item_rows_aligned(r), best);
    return hipGetLastError();
}

hipError_t launch_item_gather(const int* idx, int B, int K, const int* items, long N, int G, long idx_offset, int* out_item, hipStream_t s) {
    const long count = (long)B * K;
    if (count <= 0) return hipSuccess;
    if (!idx || !out_item || (N > 0 && !items) || G < 1) return hipErrorInvalidValue;
    FERN_LAUNCH(item_gather_kernel, dim3((unsigned)((count + ITEM_NT - 1) / ITEM_NT)), dim3(ITEM_NT), 0, s, idx, count, items, N, G, idx_offset, out_item);
    return hipGetLastError();
}

hipError_t launch_item_keys(const unsigned long long* best, int G, const int* targets, int B, int m, unsigned long long* keys, hipStream_t s) {
    const long count = (long)B * m;
    if (count <= 0) return hipSuccess;
    if (!best || !targets || !keys || G < 1) return hipErrorInvalidValue;
    FERN_LAUNCH(item_keys_kernel, dim3((unsigned)((count + ITEM_NT - 1) / ITEM_NT)), dim3(ITEM_NT), 0, s, best, G, targets, count, m, keys);
    return hipGetLastError();
}

hipError_t launch_item_count(const unsigned long long* best, int G, const unsigned long long* keys, int B, int m, int* out, hipStream_t s) {
    if (B <= 0 || m <= 0) return hipSuccess;
    if (!best || !keys || !out || G < 1) return hipErrorInvalidValue;
    FERN_LAUNCH(item_count_kernel, dim3(B, (m + ITEM_T - 1) / ITEM_T), dim3(ITEM_NT), 0, s, best, G, keys, m, out);
    return hipGetLastError();
}

}  // namespace fern
