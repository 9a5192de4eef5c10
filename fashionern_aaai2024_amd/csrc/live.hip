// Live gallery: rows of a prepared store change in place (include/fern.h: fern_gallery_upsert, fern_gallery_move, fern_scatter_u32).
//
// A serving process keeps one [capacity, D] store for its lifetime -- fp32 rows, their bf16 pre-filter copy, the three norms that
// certify the copy (fern_gallery_prepare), one tag and one item id per row -- and a catalogue changes a few hundred of a million rows
// at a time.  The kernels here write the chosen slots of ALL forms in one launch, so the forms of a row never disagree once the launch
// has finished, and they fold the new rows' norms into `meta` by maximum: a bound that is only ever raised stays a bound, so the
// certificate of the pre-filter keeps holding without a pass over the rows that did not change.
//
// Nothing here is restated arithmetic: a row's bf16 bits and its norms come from row_ops.h's gallery_chunk / gallery_norms_fold --
// the functions gallery_prepare_kernel is made of -- and the optional normalisation is l2norm_kernel's row_l2_normalize, which is why
// upserting every row of a gallery into a zeroed store reproduces fern_gallery_prepare byte for byte.
// One wave per row, four rows per 256-thread block, 16-byte accesses; HBM-bound (m * D * 10 bytes per upsert).
//
// A slot outside [0, capacity) cannot raise from inside a kernel: the wave writes nothing and records 1 + its position in a host-mapped
// flag (the text embedding kernel's scheme for token ids); api.hip turns it into FERN_ERR_ARG without a synchronisation on the launch path.
#include "live.h"
#include "row_ops.h"

namespace fern {

typedef unsigned short u16;

__device__ __forceinline__ void flag_bad_slot(int* bad, long pos) {
    __hip_atomic_store(bad, (int)(pos < 0x7FFFFFFEL ? pos + 1 : 0x7FFFFFFF), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// rows [m, ld] -> slot slots[p] of g [cap, d] (fp32, may be null), gb [cap, d] (bf16, may be null); meta (may be null) is raised, never
// reset.  NORM: the row is F.normalize'd first (held in registers: d <= 256 * MAXV).
template <bool NORM>
__global__ __launch_bounds__(256) void gallery_upsert_kernel(const float* rows, long ld, const int* slots, int m, float* g, u16* gb, float* meta,
                                                             long cap, int d, int* bad) {
    const long pos = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pos >= m) return;
    const long slot = slots[pos];
    if (slot < 0 || slot >= cap) {
        if (lane == 0) flag_bad_slot(bad, pos);
        return;
    }
    const float* x = rows + pos * ld;
    float* gr = g ? g + slot * d : nullptr;
    u16* br = gb ? gb + slot * d : nullptr;
    GalleryNorms s;
    auto put = [&](const f32x4 v, int c) {
        if (gr) *reinterpret_cast<f32x4*>(gr + c) = v;
        const ushort4 o = gallery_chunk(v, s);
        if (br) *reinterpret_cast<ushort4*>(br + c) = o;
    };
    if (NORM) {
        RowRegs r;
        row_load(r, x, d, lane);
        row_l2_normalize(r, 1e-12f, 0);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {      // the chunks in gallery_prepare_kernel's order: c = lane * 4, + 256, ...
            const int c = (i * 64 + lane) * 4;
            if (c < d) put(r.v[i], c);
        }
    } else {
        for (int c = lane * 4; c < d; c += 256) put(*reinterpret_cast<const f32x4*>(x + c), c);
    }
    if (meta) gallery_norms_fold(s, lane, meta);
}

// row src[p] -> row dst[p] of every array given; the two index sets are disjoint (the caller's contract), so no wave reads what another writes
__global__ __launch_bounds__(256) void gallery_move_kernel(const int* src, const int* dst, int m, float* g, u16* gb, unsigned* tags, int* items,
                                                           long cap, int d, int* bad) {
    const long pos = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pos >= m) return;
    const long from = src[pos], to = dst[pos];
    if (from < 0 || from >= cap || to < 0 || to >= cap) {
        if (lane == 0) flag_bad_slot(bad, pos);
        return;
    }
    if (g)
        for (int c = lane * 4; c < d; c += 256) *reinterpret_cast<f32x4*>(g + to * d + c) = *reinterpret_cast<const f32x4*>(g + from * d + c);
    if (gb)
        for (int c = lane * 4; c < d; c += 256) *reinterpret_cast<ushort4*>(gb + to * d + c) = *reinterpret_cast<const ushort4*>(gb + from * d + c);
    if (lane == 0) {
        if (tags) tags[to] = tags[from];
        if (items) items[to] = items[from];
    }
}

__global__ __launch_bounds__(256) void scatter_u32_kernel(const unsigned* src, const int* slots, int m, unsigned* dst, long cap, int* bad) {
    const long pos = (long)blockIdx.x * 256 + threadIdx.x;
    if (pos >= m) return;
    const long slot = slots[pos];
    if (slot < 0 || slot >= cap) {
        flag_bad_slot(bad, pos);
        return;
    }
    dst[slot] = src[pos];
}

static inline dim3 wave_rows_grid(long rows) { return dim3((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)); }

hipError_t launch_gallery_upsert(const float* rows, long ld, const int* slots, int m, float* g, unsigned short* gb, float* meta, long cap, int d,
                                 bool normalize, int* bad, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (d <= 0 || (d & 3) || ld < d || (ld & 3) || cap < 0 || !bad || (normalize && d > 256 * MAXV)) return hipErrorInvalidValue;
    if (normalize) hipLaunchKernelGGL(gallery_upsert_kernel<true>, wave_rows_grid(m), dim3(256), 0, s, rows, ld, slots, m, g, gb, meta, cap, d, bad);
    else hipLaunchKernelGGL(gallery_upsert_kernel<false>, wave_rows_grid(m), dim3(256), 0, s, rows, ld, slots, m, g, gb, meta, cap, d, bad);
    return hipGetLastError();
}

hipError_t launch_gallery_move(const int* src, const int* dst, int m, float* g, unsigned short* gb, unsigned* tags, int* items, long cap, int d,
                               int* bad, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (d <= 0 || (d & 3) || cap < 0 || !bad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gallery_move_kernel, wave_rows_grid(m), dim3(256), 0, s, src, dst, m, g, gb, tags, items, cap, d, bad);
    return hipGetLastError();
}

hipError_t launch_scatter_u32(const unsigned* src, const int* slots, int m, unsigned* dst, long cap, int* bad, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (cap < 0 || !bad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_u32_kernel, dim3((unsigned)(((long)m + 255) / 256)), dim3(256), 0, s, src, slots, m, dst, cap, bad);
    return hipGetLastError();
}

}  // namespace fern
