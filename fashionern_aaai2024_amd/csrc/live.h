// Launchers of live.hip: in-place updates of a gallery store (include/fern.h: fern_gallery_upsert / fern_gallery_move / fern_scatter_u32).
// `bad` is a host-mapped int: a wave that meets a slot outside [0, cap) writes nothing and stores 1 + its position there.
#pragma once
#include <hip/hip_runtime.h>

namespace fern {

// rows [m, ld] (ld >= d, ld % 4 == 0) -> g[slots[p]] (fp32, may be null) and gb[slots[p]] = bf16(row) (may be null); meta (may be null)
// is raised to the new rows' three norms, never reset.  normalize: F.normalize first (d <= 1280).  d % 4 == 0.
hipError_t launch_gallery_upsert(const float* rows, long ld, const int* slots, int m, float* g, unsigned short* gb, float* meta, long cap, int d,
                                 bool normalize, int* bad, hipStream_t s);
// row src[p] -> row dst[p] of g, gb, tags, items (each may be null); src and dst are disjoint index sets
hipError_t launch_gallery_move(const int* src, const int* dst, int m, float* g, unsigned short* gb, unsigned* tags, int* items, long cap, int d,
                               int* bad, hipStream_t s);
// dst[slots[p]] = src[p]
hipError_t launch_scatter_u32(const unsigned* src, const int* slots, int m, unsigned* dst, long cap, int* bad, hipStream_t s);

}  // namespace fern
