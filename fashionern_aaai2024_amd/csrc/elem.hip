// Row-wise kernels of the encode -> fuse -> rank path (HBM-bound; one wave64 per row, 16-byte accesses).
//
// LayerNorm (CLIP eps 1e-5, BERT eps 1e-12 with fused residual), F.normalize / VisualSR.l2norm,
// patch means, embedding gathers, and the scalar-gate / attention-pooling tails of
// CombinerSimple (fusion_model.py:92-94) and VisualSR (fusion_model.py:149-154).
#include "kernels.h"
#include "row_ops.h"      // RowRegs, load4, row_load / row_store / row_sumsq, wave_sum, row_l2_normalize: shared with live.hip
#include <type_traits>

namespace fern {

__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_move<0xB1>(v));
    v = fmaxf(v, dpp_move<0x4E>(v));
    v = fmaxf(v, dpp_move<0x141>(v));
    v = fmaxf(v, dpp_move<0x140>(v));
    return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}
// maximum over the aligned group of 4 / 8 consecutive lanes (the lanes that share a 32-element MX block)
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, dpp_move<0xB1>(v));
    return fmaxf(v, dpp_move<0x4E>(v));
}
__device__ __forceinline__ float oct_max(float v) { v = quad_max(v); return fmaxf(v, dpp_move<0x141>(v)); }

// ==== Row producers: the kernels that turn the residual stream, an activation or an image into the operand form of the next GEMM ====
// A lane holds its part of a row as CHUNKS of W consecutive elements, x[i][e] = element e of chunk i: f32x4 chunks (W = 4: RowRegs and
// the several-rows kernel, 64 lanes per row) or float[8] chunks (W = 8: the plain quantisers over 64 lanes, the half-wave LayerNorm over
// 32).  Every load, the LayerNorm statement and every output form below is stated once over such chunks: in "LN -> fp8 equals
// quantize_rows_fp8(layernorm(x)) byte for byte" (tests/test_gpu_quant_producers.py) both sides run the same text.  (Contraction is
// still left to the compiler, as it always was here: which products of the variance become fmas depends on the code around the
// call -- layernorm_rows_kernel below keeps its own copy for that reason.)
template <class V>
constexpr int chunk_width = sizeof(V) / sizeof(float);

// ---- input forms (four elements: load4, row_ops.h) -----------------------------------------------------------------------------
// Eight consecutive elements of a lane as fp32: two 16-byte loads of fp32, or one of bf16 (widened exactly).
__device__ __forceinline__ void load8(float (&v)[8], const float* p) {
    const f32x4 a = load4(p), b = load4(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
__device__ __forceinline__ void load8(float (&v)[8], const unsigned short* p) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(w[e] << 16); v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
}

// ---- LayerNorm: y = (x - mean) / sqrt(var + eps) * gamma + beta with the two-pass variance torch uses -----------------------------
// Over this lane's chunks of this row.  `sum` adds a value over the lanes that share the row (wave_sum, or the half-wave's sum);
// live(i): chunk i lies inside the row (a chunk outside holds zeros: nothing for the sum, but (0 - mean)^2 for the variance).
// A 4-element chunk enters the sum as one partial sum, the 8 elements of a half-wave chunk one by one: the orders these layouts have
// always had, and the reason the half-wave kernel's values may differ from the one-row kernel's in the last bits.
template <int CH, class V, class Sum>
__device__ __forceinline__ float ln_mean(const V (&x)[CH], Sum sum, float d) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if constexpr (chunk_width<V> == 4) s += x[i][0] + x[i][1] + x[i][2] + x[i][3];
        else
#pragma unroll
            for (int e = 0; e < chunk_width<V>; ++e) s += x[i][e];
    }
    return sum(s) / d;
}
template <int CH, class V, class Live, class Sum>
__device__ __forceinline__ float ln_rstd(const V (&x)[CH], float mean, Live live, Sum sum, float d, float eps) {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i)
        if (live(i)) {
#pragma unroll
            for (int e = 0; e < chunk_width<V>; ++e) { const float t = x[i][e] - mean; q += t * t; }
        }
    return rsqrtf(sum(q) / d + eps);
}
__device__ __forceinline__ float ln_affine(float x, float mean, float rstd, float g, float b) { return (x - mean) * rstd * g + b; }

// the RowRegs instance (one wave per row of any width d % 4 == 0): the one-row kernels below and bert_embed_kernel
__device__ __forceinline__ void row_layernorm(RowRegs& r, const float* gamma, const float* beta, int d, int lane, float eps) {
    const auto live = [&](int i) { return (i * 64 + lane) * 4 < d; };
    const float mean = ln_mean(r.v, wave_sum, (float)d);
    const float rstd = ln_rstd(r.v, mean, live, wave_sum, (float)d, eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < d) {
            const f32x4 g = load4(gamma + c), bb = load4(beta + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) r.v[i][e] = ln_affine(r.v[i][e], mean, rstd, g[e], bb[e]);
        }
    }
}

// ---- output forms (the fp32 store of a row: row_store, row_ops.h) -----------------------------------------------------------------
// four fp32 -> four bf16 (round to nearest even), one 8-byte store
__device__ __forceinline__ void store4_bf16(unsigned short* p, const f32x4 v) {
    ushort4 o;
    o.x = f32_to_bf16_bits(v[0]); o.y = f32_to_bf16_bits(v[1]); o.z = f32_to_bf16_bits(v[2]); o.w = f32_to_bf16_bits(v[3]);
    *reinterpret_cast<ushort4*>(p) = o;
}
// max(am, |v[e]|) over a chunk, and the same without a running maximum.  A maximum is exact, so the order cannot change a bit: a
// 4-element chunk is reduced by pairs and an 8-element one in turn because those are the instructions each layout has always had.
template <class V>
__device__ __forceinline__ float chunk_amax(float am, const V& v) {
    if constexpr (chunk_width<V> == 4) return fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
#pragma unroll
    for (int e = 0; e < chunk_width<V>; ++e) am = fmaxf(am, fabsf(v[e]));
    return am;
}
template <class V>
__device__ __forceinline__ float chunk_amax(const V& v) {
    if constexpr (chunk_width<V> == 4) return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
    return chunk_amax(0.f, v);
}
// a chunk times `inv` as e4m3fn bytes: one 4- or 8-byte store, or (NT) non-temporal dword stores
template <bool NT = false, class V>
__device__ __forceinline__ void store_fp8(unsigned char* p, const V& v, float inv) {
    constexpr int NW = chunk_width<V> / 4;
    unsigned w[NW];
#pragma unroll
    for (int h = 0; h < NW; ++h) w[h] = pack4_fp8(v[4 * h] * inv, v[4 * h + 1] * inv, v[4 * h + 2] * inv, v[4 * h + 3] * inv);
    if constexpr (NT) {
#pragma unroll
        for (int h = 0; h < NW; ++h) __builtin_nontemporal_store(w[h], reinterpret_cast<unsigned*>(p) + h);
    } else if constexpr (NW == 1) {
        *reinterpret_cast<unsigned*>(p) = w[0];
    } else {
        *reinterpret_cast<uint2*>(p) = uint2{w[0], w[1]};
    }
}
// Per-row fp8 (e4m3fn) of a row held by the 64 lanes of a wave, chunk i at column (i * 64 + lane) * W: scale = max|x| / 448 (1 for an
// all-zero row), bytes = fp8(x / scale).
// `am`: max|x| over this lane's chunks (chunk_amax over the chunks inside the row) -- an argument, because a kernel that takes the
// maximum where it loads a chunk has one guarded region per chunk, where a second loop is a second set of them: quantize_rows_fp8 at
// 12608 x 3072 took 21.1 us with the second loop against 19.4 us.
template <int CH, class V>
__device__ __forceinline__ void row_store_fp8(const V (&x)[CH], float am, unsigned char* yr, float* scale, int d, int lane) {
    constexpr int W = chunk_width<V>;
    am = wave_max(am);
    const float sc = am > 0.f ? am * (1.0f / 448.0f) : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) *scale = sc;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = (i * 64 + lane) * W;
        if (c < d) store_fp8(yr + c, x[i], inv);
    }
}
// MX (block-scaled) e4m3fn: one E8M0 byte per 32 consecutive k, the operand form of v_mfma_scale_f32_32x32x64_f8f6f4 (gemm_bf16.hip:
// gemm_mx8_kernel).  e = the smallest power of two that brings the block's maximum to <= 448, read off the maximum's exponent /
// mantissa bits (448 = 1.75 * 2^8); the scaling x * 2^(127-e) is exact.
// This lane's chunk at column c of `row` (bytes at yr + c); the 32 / W consecutive lanes that hold a 32-element block all call this
// (the group maximum is a DPP exchange), live or not -- a chunk outside the row holds zeros and stores nothing.
template <bool NT = false, class V>
__device__ __forceinline__ void store_mx8(const V& v, bool live, unsigned char* yr, int c, unsigned char* scales, long srows, long row, int lane) {
    constexpr int W = chunk_width<V>;
    static_assert(W == 4 || W == 8, "a 32-element block is 8 or 4 lanes");
    const float lm = chunk_amax(v);
    const float am = W == 4 ? oct_max(lm) : quad_max(lm);
    if (live) {
        const unsigned e = mx_scale_byte(am);
        const float inv = mx_inv_scale(e);
        store_fp8<NT>(yr + c, v, inv);
        if ((lane & (32 / W - 1)) == 0) scales[mx_scale_offset(row, c >> 5, srows)] = (unsigned char)e;
    }
}

// ---- one row per wave: LayerNorm of fp32 (or bf16) rows of any width, into any operand form ----------------------------------------
// Out: where the normalised row goes.
struct RowToF32 {
    float* y; long ldy;
    __device__ void operator()(const RowRegs& r, long row, int d, int lane) const { row_store(r, y + row * ldy, d, lane); }
};
struct RowToBf16 {
    unsigned short* y; long ldy;
    __device__ void operator()(const RowRegs& r, long row, int d, int lane) const {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < d) store4_bf16(y + row * ldy + c, r.v[i]);
        }
    }
};
struct RowToFp8 {
    unsigned char* y; long ldy; float* scale;
    __device__ void operator()(const RowRegs& r, long row, int d, int lane) const {
        float am = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i)
            if ((i * 64 + lane) * 4 < d) am = chunk_amax(am, r.v[i]);
        row_store_fp8(r.v, am, y + row * ldy, scale + row, d, lane);
    }
};
struct RowToMx8 {      // a lane holds 4 consecutive elements: a 32-block is 8 lanes
    unsigned char* y; long ldy; unsigned char* scales; long srows;
    __device__ void operator()(const RowRegs& r, long row, int d, int lane) const {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * 4;
            store_mx8(r.v[i], c < d, y + row * ldy, c, scales, srows, row, lane);
        }
    }
};
template <class T, class Out>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* x, const float* gamma, const float* beta, Out out, long rows, int d, long ldx,
                                                        float eps, const float* res) {
    // (res is the LAST argument: with it among the first, the quantising instances fetched gamma / beta / out from the argument
    // segment only where the affine map needs them -- a scalar-load wait in the middle of every wave, where the four kernels this body
    // replaces had all their arguments in the prologue; in a kernel trace LN -> fp8 at 16448 x 1024 took 17.7 us for 16.7, 17.3 for 17.4 now)
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    RowRegs r;
    row_load(r, x + row * ldx, d, lane);
    if constexpr (std::is_same_v<Out, RowToF32>) {      // the fused residual (BERT): fp32 -> fp32 only
        if (res) {
            RowRegs q;
            row_load(q, res + row * ldx, d, lane);
#pragma unroll
            for (int i = 0; i < MAXV; ++i) r.v[i] += q.v[i];
        }
    }
    row_layernorm(r, gamma, beta, d, lane, eps);
    out(r, row, d, lane);
}

// Per-row fp8 / MX quantisation of a bf16 or fp32 matrix: one wave per row, a lane holds 8 consecutive elements (a 32-block is 4
// lanes), rows up to 8 * 512 = 4096 wide, d % 8 == 0.  Used for the attention / GELU outputs (bf16) and the weight matrices (fp32).
__device__ __forceinline__ void row_load8(float (&v)[8], const unsigned short* xb, const float* xf, long at, bool live) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (live) {
        if (xb) load8(v, xb + at);
        else load8(v, xf + at);
    }
}
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const unsigned short* xb, const float* xf, long ldx, unsigned char* y, long ldy,
                                                                float* scale, long rows, int d) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float v[8][8];
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = (i * 64 + lane) * 8;
        row_load8(v[i], xb, xf, row * ldx + c, c < d);
        if (c < d) am = chunk_amax(am, v[i]);
    }
    row_store_fp8(v, am, y + row * ldy, scale + row, d, lane);
}
__global__ __launch_bounds__(256) void quantize_mx8_kernel(const unsigned short* xb, const float* xf, long ldx, unsigned char* y, long ldy,
                                                           unsigned char* scales, long srows, long rows, int d) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = (i * 64 + lane) * 8;
        float v[8];
        row_load8(v, xb, xf, row * ldx + c, c < d);
        store_mx8(v, c < d, y + row * ldy, c, scales, srows, row, lane);
    }
}

// d = 256 * NV, NV = 1 .. 4 (the widths the two fixed-width LayerNorm kernels below cover): f(NV as a compile-time constant)
template <class F>
static void with_nv(int d, F f) {
    switch (d / 256) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// ---- several rows per wave (round 4), fp32 -> fp32 --------------------------------------------------------------------------------
// One wave per row is one memory round trip, two dependent wave reductions and one store per row, back to back: at 12608 rows x
// 768 columns the LayerNorm launches ran at 2.8 TB/s (bf16 rows in, fp8 out) -- latency, not bytes.  Here a wave owns RPW consecutive
// rows: all their loads are issued before the first reduction (one round trip per RPW rows), the 2 x RPW reductions interleave, and
// gamma / beta are fetched once per wave.  The width is a template parameter (d = 256 NV: no per-chunk bounds tests).  The per-row
// arithmetic is the one-row kernel's statement for statement, and the kernel is used for EVERY row count of a width it covers,
// so a row's bits still do not depend on the batch it travels in.  The output may alias the input.
// (The bf16-input and MX-output forms this kernel once had lost to the half-wave kernel below in rounds 4 and 6 -- 15.1 and 14.0 us
// against 9.1 at 12608 x 768 -- and are gone: rows the half-wave kernel does not take go to the one-row kernel, with the same bytes.)
template <int NV, int RPW>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* x, const float* gamma, const float* beta, float* y, long rows, long ldx,
                                                             long ldy, float eps) {
    constexpr int D = 256 * NV;
    const int lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    f32x4 v[RPW][NV];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long row = row0 + r < rows ? row0 + r : rows - 1;      // a short last group re-reads the last row (not stored)
#pragma unroll
        for (int i = 0; i < NV; ++i) v[r][i] = load4(x + row * ldx + (i * 64 + lane) * 4);
    }
    f32x4 g[NV], bb[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g[i] = load4(gamma + (i * 64 + lane) * 4);
        bb[i] = load4(beta + (i * 64 + lane) * 4);
    }
    float mean[RPW], rstd[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) mean[r] = ln_mean(v[r], wave_sum, (float)D);
    // ln_rstd's statement, written out: called as a function (any of five ways of passing the rows tried) the compiler pairs the four
    // rows' products differently and contracts other terms of q into fmas than it does here (at 768 columns 42 instead of 16; at 512
    // and 1024, 12 and 46 instead of none), which moves the last bit of rstd.  These are the operations the kernel has always had.
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float t = v[r][i][e] - mean[r]; q += t * t; }
        rstd[r] = rsqrtf(wave_sum(q) / (float)D + eps);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long row = row0 + r;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ln_affine(v[r][i][e], mean[r], rstd[r], g[i][e], bb[i][e]);
            if (row < rows) *reinterpret_cast<f32x4*>(y + row * ldy + (i * 64 + lane) * 4) = o;
        }
    }
}
constexpr int LN_RPW = 4;
// widths the several-rows kernel covers (256, 512, 768, 1024): launch it and return true
static bool launch_ln_rows(const float* x, const float* gamma, const float* beta, float* y, long rows, int d, long ldx, long ldy, float eps,
                           hipStream_t s) {
    if (d % 256 || d > 1024) return false;
    // gamma / beta are read as f32x4: the public entry points accept any 4-byte-aligned view, so a pointer that is not 16-byte aligned
    // takes the one-row kernel instead
    if (((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return false;
    const dim3 grid((unsigned)((rows + ROWS_PER_BLOCK * LN_RPW - 1) / (ROWS_PER_BLOCK * LN_RPW)));
    with_nv(d, [&](auto nv) {
        hipLaunchKernelGGL((layernorm_rows_kernel<decltype(nv)::value, LN_RPW>), grid, dim3(256), 0, s, x, gamma, beta, y, rows, ldx, ldy, eps);
    });
    return true;
}

// ---- bf16 rows in, MX fp8 out: half a wave per row (round 4, tools/probe/ln_lab.hip) ---------------------------------------------
// The block-scaled mode's LayerNorm reads the bf16 residual stream the GEMM before it has just written (from other XCDs: nothing of
// it is in this CU's L2) and is a single round of waves: its time is the latency of that round, not its 29 MB.  Measured in the chain
// writer -> LayerNorm -> reader at 12608 x 768: four rows per wave (the several-rows kernel's layout) 15.1 us, one row per wave 10.7,
// this form 9.1 (a byte-for-byte copy of the same shape: 8.7).  A lane holds 8 consecutive elements of each 256-column chunk of ITS
// half-wave's row -- one 16-byte load and one 8-byte store per chunk, 512 contiguous bytes per half-wave -- and a 32-element MX block
// is 4 lanes.  The fp8 bytes leave with nt stores: the next kernel reads them from other XCDs anyway.  Statistics: the row's 32 lanes
// on the DPP network, the two 16-lane rows of the half added in a fixed order; used for EVERY row count of a width it covers
// (batch-invariant).
// T = float (round 6, FERN_PREC_MX8_MLP / _MX8_IMG: block-scaled operands over the FP32 residual stream): the same kernel on fp32 rows
// -- two 16-byte loads per chunk and lane -- instead of four rows per wave (14.0 us at 12608 x 768, 22 launches per step).
template <int NV, class T>
__global__ __launch_bounds__(256) void layernorm_half_kernel(const T* x, const float* gamma, const float* beta, unsigned char* y, unsigned char* scales,
                                                             long srows, long rows, long ldx, long ldy, float eps) {
    constexpr int D = 256 * NV;
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const long rowp = ((long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)) * 2;
    if (rowp >= rows) return;
    const long row = rowp + lh;
    const long rrow = row < rows ? row : rows - 1;             // an odd row count: the last wave's upper half re-reads the last row (not stored)
    float v[NV][8], g[NV][8], bb[NV][8];
#pragma unroll
    for (int i = 0; i < NV; ++i) load8(v[i], x + rrow * ldx + (i * 32 + l31) * 8);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        load8(g[i], gamma + (i * 32 + l31) * 8);
        load8(bb[i], beta + (i * 32 + l31) * 8);
    }
    const auto half_sum = [&](float t) {      // over the 32 lanes of this lane's half
        t += dpp_move<0xB1>(t);
        t += dpp_move<0x4E>(t);
        t += dpp_move<0x141>(t);
        t += dpp_move<0x140>(t);
        const float lo = lane_f(t, 0) + lane_f(t, 16), hi = lane_f(t, 32) + lane_f(t, 48);
        return lh ? hi : lo;
    };
    const float mean = ln_mean(v, half_sum, (float)D);
    const float rstd = ln_rstd(v, mean, [](int) { return true; }, half_sum, (float)D, eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ln_affine(v[i][e], mean, rstd, g[i][e], bb[i][e]);
        store_mx8<true>(o, row < rows, y + row * ldy, (i * 32 + l31) * 8, scales, srows, row, lane);
    }
}
template <class T>
static bool launch_ln_half(const T* x, const float* gamma, const float* beta, unsigned char* y, unsigned char* scales, long srows, long rows, int d,
                           long ldx, long ldy, float eps, hipStream_t s) {
    if (d % 256 || d > 1024 || (ldx & 7) || (ldy & 7) || ((uintptr_t)x & 15) || ((uintptr_t)y & 7) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return false;
    const dim3 grid((unsigned)((rows + ROWS_PER_BLOCK * 2 - 1) / (ROWS_PER_BLOCK * 2)));
    with_nv(d, [&](auto nv) {
        hipLaunchKernelGGL((layernorm_half_kernel<decltype(nv)::value, T>), grid, dim3(256), 0, s, x, gamma, beta, y, scales, srows, rows, ldx, ldy, eps);
    });
    return true;
}

// ---- patch rows of a [b, 3, img, img] image batch ------------------------------------------------------------------------------
// Row (image, gy, gx) = the 3 x patch x patch pixels of one patch in (channel, y, x) order -- the k order of conv1's
// [width, 3 * patch * patch] weight -- so that the patch embedding is a plain GEMM.  One wave per patch.
struct PatchRow {
    const float* src;      // the patch's top left pixel in channel 0
    int img, patch, pp;
    __device__ const float* at(int k) const {      // element k of the row
        const int ch = k / pp, rem = k % pp;
        return src + ((long)ch * img + rem / patch) * img + rem % patch;
    }
};
__device__ __forceinline__ PatchRow patch_row(const float* images, long row, int img, int patch, int grid) {
    const int g2 = grid * grid;
    const long b = row / g2;
    const int gy = (int)(row % g2) / grid, gx = (int)(row % g2) % grid;
    return PatchRow{images + b * 3L * img * img + (long)(gy * patch) * img + gx * patch, img, patch, patch * patch};
}

// Block-scale quantised (the patch embedding of the block-scaled mode is a plain MX GEMM); a lane holds 4 consecutive x of one
// (channel, y) per step.
__global__ __launch_bounds__(256) void im2col_mx8_kernel(const float* images, unsigned char* y, unsigned char* scales, long srows, long rows,
                                                         int img, int patch, int grid) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const PatchRow p = patch_row(images, row, img, patch, grid);
    const int d = 3 * p.pp;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int k = (i * 64 + lane) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < d) v = load4(p.at(k));
        store_mx8(v, k < d, y + row * d, k, scales, srows, row, lane);
    }
}

// The same patch rows as bf16 (round to nearest even): the patch embedding of the bf16-operand modes (FERN_PREC_BF16 / _MX8_MLP /
// _MX8_IMG, round 6) is a plain bf16 GEMM -- the im2col-loading fp32 GEMM took 166 us of a 4.9 ms step where this pair takes ~40.
__global__ __launch_bounds__(256) void im2col_bf16_kernel(const float* images, unsigned short* y, long rows, int img, int patch, int grid) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const PatchRow p = patch_row(images, row, img, patch, grid);
    const int d = 3 * p.pp;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int k = (i * 64 + lane) * 4;
        if (k < d) store4_bf16(y + row * d + k, load4(p.at(k)));
    }
}

// Patch sides the 16-byte patch loaders do not take (14: a patch row is 14 floats, K = 588 is not a multiple of 32): the patch rows as
// fp32 in the same (channel, y, x) order, zero padded to kp columns (588 -> 608), for the plain-loader fp32 GEMM against the equally
// padded conv1 weight.  Scalar reads: a patch row starts on no 16-byte boundary.
__global__ __launch_bounds__(256) void patch_rows_f32_kernel(const float* images, float* y, long rows, int img, int patch, int grid, int kp) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const PatchRow p = patch_row(images, row, img, patch, grid);
    const int d = 3 * p.pp;
    for (int k = lane; k < kp; k += 64) y[row * kp + k] = k < d ? *p.at(k) : 0.0f;
}

__global__ __launch_bounds__(256) void l2norm_kernel(const float* x, const float* x2, long ldx, float* y, long ldy, long rows, int d,
                                                     float eps, int mode) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    RowRegs r;
    row_load(r, x + row * ldx, d, lane);
    if (x2) {                                   // normalize(x + x2): utils.element_wise_sum
        RowRegs q;
        row_load(q, x2 + row * ldx, d, lane);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) r.v[i] += q.v[i];
    }
    row_l2_normalize(r, eps, mode);
    row_store(r, y + row * ldy, d, lane);
}

// Cross-entropy of `scale * logits[row, :]` against label = row (losses/loss.py:10-14): log-sum-exp minus the diagonal logit.
__global__ __launch_bounds__(256) void ce_diag_rows_kernel(const float* logits, long ld, int n, float scale, float* row_loss) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* x = logits + row * ld;
    float m = -INFINITY;
    for (int c = lane; c < n; c += 64) m = fmaxf(m, x[c] * scale);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < n; c += 64) sum += expf(x[c] * scale - m);
    sum = wave_sum(sum);
    if (lane == 0) row_loss[row] = (m + logf(sum)) - x[row] * scale;
}
// out[0] = mean(v[0..n)) in a fixed summation order (one wave)
__global__ __launch_bounds__(64) void mean_scalar_kernel(const float* v, int n, float* out) {
    float s = 0.f;
    for (int c = threadIdx.x; c < n; c += 64) s += v[c];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = s / (float)n;
}

// y[row] = mean_{p<P} x[row*group_stride + row_add + p]
// One wave per (row, 256-column chunk); the P rows are requested EIGHT at a time and added in order p = 0, 1, ... (the sum's order --
// and so its bits -- is that of the one-load-at-a-time loop it replaces: 64 query rows x 77 tokens took 30 us on 64 waves, each
// waiting for one row at a time).
__global__ __launch_bounds__(256) void mean_rows_kernel(const float* x, long ldx, float* y, long ldy, long n, int P, int d,
                                                        long group_stride, long row_add) {
    const int nchunk = (d + 255) / 256;
    const long item = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long row = item / nchunk;
    const int c = (int)(item % nchunk) * 256 + lane * 4;
    if (row >= n || c >= d) return;
    const float* src = x + (row * group_stride + row_add) * ldx + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int p = 0;
    for (; p + 32 <= P; p += 32) {      // round 5: 32 rows in flight (128 VGPRs) -- 77 tokens are 3 round trips instead of 10 (a round trip here is ~3 us:
        f32x4 t[32];                    // the rows were just written from other XCDs); same summation order, same bits
#pragma unroll
        for (int u = 0; u < 32; ++u) t[u] = *reinterpret_cast<const f32x4*>(src + (long)(p + u) * ldx);
#pragma unroll
        for (int u = 0; u < 32; ++u) acc += t[u];
    }
    for (; p + 8 <= P; p += 8) {
        f32x4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const f32x4*>(src + (long)(p + u) * ldx);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += t[u];
    }
    for (; p < P; ++p) acc += *reinterpret_cast<const f32x4*>(src + (long)p * ldx);
    const float invp = 1.0f / (float)P;
    *reinterpret_cast<f32x4*>(y + row * ldy + c) = acc * invp;
}

// y[i] = x[(i / group)*group_stride + (i % group) + (idx ? idx[i] : row_add)]
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* x, long ldx, float* y, long ldy, long n, int d, int group,
                                                          long group_stride, long row_add, const int* idx) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const long src = (row / group) * group_stride + (row % group) + (idx ? (long)idx[row] : row_add);
    RowRegs r;
    row_load(r, x + src * ldx, d, lane);
    row_store(r, y + row * ldy, d, lane);
}

// y[i] (fp32) = widen(x[i * row_stride]) for a bf16 source (the class rows of the block-scaled mode's bf16 residual stream): one thread per
// four columns, exact widening
__global__ __launch_bounds__(256) void gather_rows_bf16_kernel(const unsigned short* x, long ldx, float* y, long ldy, long n, int d, long row_stride) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int d4 = d >> 2;
    if (i >= n * d4) return;
    const long row = i / d4;
    const int c = (int)(i % d4) * 4;
    const ushort4 v = *reinterpret_cast<const ushort4*>(x + row * row_stride * ldx + c);
    float4 o;
    o.x = bf16_bits_to_f32(v.x); o.y = bf16_bits_to_f32(v.y); o.z = bf16_bits_to_f32(v.z); o.w = bf16_bits_to_f32(v.w);
    *reinterpret_cast<float4*>(y + row * ldy + c) = o;
}

__global__ __launch_bounds__(256) void bert_embed_kernel(const float* cls, const float* local, const float* seq, const float* type_emb,
                                                         const float* pos_emb, const float* gamma, const float* beta, float* X,
                                                         int B, int P, int T, int d, float eps) {
    const int S = 1 + P + T;
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)B * S) return;
    const int b = (int)(row / S), s = (int)(row % S);
    const float* src = s == 0 ? cls : (s <= P ? local + ((long)b * P + (s - 1)) * d : seq + ((long)b * T + (s - 1 - P)) * d);
    RowRegs r, t, q;
    row_load(r, src, d, lane);
    row_load(t, type_emb + (s > P ? d : 0), d, lane);
    row_load(q, pos_emb + (long)s * d, d, lane);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) r.v[i] = (r.v[i] + t.v[i]) + q.v[i];     // HF BertEmbeddings order: inputs + type, then + position
    row_layernorm(r, gamma, beta, d, lane, eps);
    row_store(r, X + row * d, d, lane);
}

__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* text, const float* tok_emb, const float* pos_emb, float* X,
                                                         int B, int T, int d, int vocab, int* bad_flag) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)B * T) return;
    const int s = (int)(row % T);
    const long tok = text[row];
    RowRegs r, q;
    if (tok < 0 || tok >= vocab) {
        // nn.Embedding raises on such an id (the reference's token_embedding lookup); a kernel cannot, so the row is poisoned
        // with NaN -- which reaches every feature of this caption -- and the host-visible flag records where it happened
        // (1 + flat position); fern_sync / the next fern_text_encode on this context report it as FERN_ERR_ARG
        if (lane == 0 && bad_flag) __hip_atomic_store(bad_flag, (int)(row < 0x7FFFFFFEL ? row + 1 : 0x7FFFFFFF), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) r.v[i] = __builtin_nanf("");
        row_store(r, X + row * d, d, lane);
        return;
    }
    row_load(r, tok_emb + tok * d, d, lane);
    row_load(q, pos_emb + (long)s * d, d, lane);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) r.v[i] += q.v[i];
    row_store(r, X + row * d, d, lane);
}

// eot[b] = first position of the maximum token id (torch.argmax semantics on the reference's EOT pooling).  One wave per caption:
// a single thread walking the 77 tokens is a chain of 77 dependent memory round trips (20 us for a kernel that moves 40 KB).
__global__ __launch_bounds__(256) void text_eot_kernel(const int64_t* text, int* eot, int B, int T) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    long long best = -0x7fffffffffffffffLL - 1;
    int pos = 0x7fffffff;
    for (int s = lane; s < T; s += 64) {      // ascending positions per lane: a lane keeps its first maximum
        const long long v = text[(long)b * T + s];
        if (v > best) { best = v; pos = s; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long ob = __shfl_xor(best, off);
        const int op = __shfl_xor(pos, off);
        if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    if (lane == 0) eot[b] = pos;
}

__global__ __launch_bounds__(256) void vit_cls_kernel(const float* cls, const float* pos, float* X, int B, int tokens, int d) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    RowRegs r, q;
    row_load(r, cls, d, lane);
    row_load(q, pos, d, lane);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) r.v[i] += q.v[i];
    row_store(r, X + row * tokens * d, d, lane);
}

// bias + partial[0] + partial[1] + ... in that order (the reduce epilogues' per-32-column partial sums of one row): the partials are
// fetched 64 at a time, one per lane, and added on the scalar path lane by lane -- the same chain of additions, bit for bit, as the
// one-dependent-load-per-step loop it replaces (which cost a memory round trip per partial on every wave)
__device__ __forceinline__ float ordered_partial_sum(float z, const float* partial, int nb, int lane) {
    for (int j0 = 0; j0 < nb; j0 += 64) {
        const float v = j0 + lane < nb ? partial[j0 + lane] : 0.0f;
        const int m = nb - j0 < 64 ? nb - j0 : 64;
        for (int j = 0; j < m; ++j) z += lane_f(v, j);
    }
    return z;
}

__global__ __launch_bounds__(256) void combiner_finalize_kernel(const float* partial, int nb, const float* b2, const float* image,
                                                                const float* text, const float* extra, float* out, long n, int d) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float z = ordered_partial_sum(b2[0], partial + row * nb, nb, lane);           // fixed order: deterministic
    const float s = 1.0f / (1.0f + expf(-z));
    RowRegs im, tx;
    row_load(im, image + row * d, d, lane);
    row_load(tx, text + row * d, d, lane);
    if (extra) {                                // CLIP4Cir Combiner: output_layer(...) + s*text + (1-s)*image (Combiner_Model.py:63-67)
        RowRegs ex;
        row_load(ex, extra + row * d, d, lane);
#pragma unroll
        for (int i = 0; i < MAXV; ++i) im.v[i] = (ex.v[i] + tx.v[i] * s) + im.v[i] * (1.0f - s);
    } else {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) im.v[i] = tx.v[i] * s + im.v[i] * (1.0f - s);
    }
    const float den = fmaxf(sqrtf(row_sumsq(im)), 1e-12f);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) im.v[i] = im.v[i] / den;
    row_store(im, out + row * d, d, lane);
}

__global__ __launch_bounds__(256) void sr_finalize_kernel(const float* partial, int nb, const float* bc, const float* local, float* out,
                                                          long n, int d) {
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    float w[13];
    float m = -INFINITY;
#pragma unroll
    for (int p = 0; p < 13; ++p) {
        const float z = ordered_partial_sum(bc[0], partial + (row * 13 + p) * nb, nb, lane);
        w[p] = z;
        m = fmaxf(m, z);
    }
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < 13; ++p) { w[p] = expf(w[p] - m); sum += w[p]; }
    RowRegs acc;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) acc.v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 13; ++p) {
        RowRegs r;
        row_load(r, local + (row * 13 + p) * d, d, lane);
        const float wp = w[p] / sum;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) acc.v[i] += r.v[i] * wp;
    }
    const float den = sqrtf(row_sumsq(acc)) + 1e-8f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) acc.v[i] = acc.v[i] / den;
    row_store(acc, out + row * d, d, lane);
}

// one wave per (query, named row): a coalesced d-wide dot product
__global__ __launch_bounds__(256) void gather_scores_kernel(const float* q, const float* gallery, const int* idx, float* out, int B, int m, int d) {
    const long item = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= (long)B * m) return;
    const int gi = idx[item];
    if (gi < 0) { if (lane == 0) out[item] = -INFINITY; return; }
    RowRegs a, g;
    row_load(a, q + (item / m) * d, d, lane);
    row_load(g, gallery + (long)gi * d, d, lane);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) s += a.v[i][0] * g.v[i][0] + a.v[i][1] * g.v[i][1] + a.v[i][2] * g.v[i][2] + a.v[i][3] * g.v[i][3];
    s = wave_sum(s);
    if (lane == 0) out[item] = s;
}

// ---- ModifiedResNet (open_clip RN50x4 image tower) helpers -------------------------------------------------------
// Stem conv1: 3 input channels -> K = 27, far too thin for MFMA; a direct convolution (0.1 % of the tower's flops).
// One thread = one output pixel x 4 output channels; NCHW image in, NHWC activation out, BatchNorm folded, ReLU.
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* img, const float* w, const float* bias, float* out, int B, int S,
                                                        int cout) {
    const int So = S / 2, c4n = cout / 4;
    const long total = (long)B * So * So * c4n;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c4 = (int)(t % c4n);
    const long pix = t / c4n;
    const int x = (int)(pix % So), y = (int)((pix / So) % So), b = (int)(pix / ((long)So * So));
    f32x4 acc = *reinterpret_cast<const f32x4*>(bias + c4 * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = 2 * y + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = 2 * x + kx - 1;
                float v = 0.f;
                if (yy >= 0 && yy < S && xx >= 0 && xx < S) v = img[(((long)b * 3 + c) * S + yy) * S + xx];
                const int k = (c * 3 + ky) * 3 + kx;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(v, w[(c4 * 4 + e) * 27 + k], acc[e]);
            }
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
    *reinterpret_cast<f32x4*>(out + pix * cout + c4 * 4) = acc;
}

// The same convolution with one thread = one output pixel x ALL output channels (C4N groups of 4): the 27 image taps are loaded once
// per pixel instead of once per channel group, the weights come from an LDS image laid out [tap][channel] (one broadcast
// ds_read_b128 per tap and channel group), and a thread stores its pixel's whole channel vector contiguously.  Each output is the
// same fma chain (bias, then taps in (c, ky, kx) order): bit-identical to the kernel above.
template <int C4N>
__global__ __launch_bounds__(256) void stem_conv_px_kernel(const float* img, const float* w, const float* bias, float* out, int B, int S) {
    constexpr int COUT = 4 * C4N;
    __shared__ f32x4 ws[27][C4N];
    for (int i = threadIdx.x; i < 27 * COUT; i += 256) {
        const int k = i / COUT, co = i % COUT;
        reinterpret_cast<float*>(&ws[0][0])[i] = w[co * 27 + k];
    }
    __syncthreads();
    const int So = S / 2;
    const long total = (long)B * So * So;
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= total) return;
    const int x = (int)(pix % So), y = (int)((pix / So) % So), b = (int)(pix / ((long)So * So));
    f32x4 acc[C4N];
#pragma unroll
    for (int c4 = 0; c4 < C4N; ++c4) acc[c4] = *reinterpret_cast<const f32x4*>(bias + c4 * 4);
    float v[27];      // the pixel's taps, all requested before the first is used
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = 2 * y + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = 2 * x + kx - 1;
                float t = 0.f;
                if (yy >= 0 && yy < S && xx >= 0 && xx < S) t = img[(((long)b * 3 + c) * S + yy) * S + xx];
                v[(c * 3 + ky) * 3 + kx] = t;
            }
        }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
#pragma unroll
        for (int c4 = 0; c4 < C4N; ++c4) {
            const f32x4 wv = ws[k][c4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[c4][e] = fmaf(v[k], wv[e], acc[c4][e]);
        }
        __builtin_amdgcn_sched_barrier(0);      // one tap's weight reads at a time (unfenced, all 270 are hoisted and spill)
    }
    float* o = out + pix * COUT;
#pragma unroll
    for (int c4 = 0; c4 < C4N; ++c4) {
        f32x4 r = acc[c4];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], 0.f);
        *reinterpret_cast<f32x4*>(o + c4 * 4) = r;
    }
}

__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const float* x, float* y, int B, int H, int W, int C, int k) {
    const int Ho = H / k, Wo = W / k, c4n = C / 4;
    const long total = (long)B * Ho * Wo * c4n;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c4 = (int)(t % c4n);
    const long pix = t / c4n;
    const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx)
            acc += *reinterpret_cast<const f32x4*>(x + (((long)b * H + yo * k + dy) * W + xo * k + dx) * C + c4 * 4);
    acc = acc * (1.0f / (float)(k * k));
    *reinterpret_cast<f32x4*>(y + pix * C + c4 * 4) = acc;
}

// mean over the HW tokens of each image (any width C % 4 == 0): one thread per (image, 4 channels)
__global__ __launch_bounds__(256) void mean_tokens_kernel(const float* x, float* mean, int B, int HW, int C) {
    const int c4n = C / 4;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * c4n) return;
    const int c4 = (int)(t % c4n), b = (int)(t / c4n);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < HW; ++i) acc += *reinterpret_cast<const f32x4*>(x + ((long)b * HW + i) * C + c4 * 4);
    *reinterpret_cast<f32x4*>(mean + (long)b * C + c4 * 4) = acc * (1.0f / (float)HW);
}

__global__ __launch_bounds__(256) void attnpool_tokens_kernel(const float* x, const float* mean, const float* pos, float* T, float* T0,
                                                              int B, int HW, int C) {
    const int c4n = C / 4;
    const long total = (long)B * (HW + 1) * c4n;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c4 = (int)(t % c4n);
    const long row = t / c4n;
    const int tok = (int)(row % (HW + 1)), b = (int)(row / (HW + 1));
    const float* src = tok == 0 ? mean + (long)b * C : x + ((long)b * HW + tok - 1) * C;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + c4 * 4) + *reinterpret_cast<const f32x4*>(pos + (long)tok * C + c4 * 4);
    *reinterpret_cast<f32x4*>(T + row * C + c4 * 4) = v;
    if (tok == 0) *reinterpret_cast<f32x4*>(T0 + (long)b * C + c4 * 4) = v;      // compact copy of the query (mean) token
}

static inline bool bad_width(int d) { return d <= 0 || (d & 3) || d > 64 * 4 * MAXV; }
static inline dim3 row_grid(long rows) { return dim3((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)); }

template <class T, class Out>
static hipError_t launch_ln_row(const T* x, const float* res, const float* gamma, const float* beta, Out out, long rows, int d, long ldx, float eps,
                                hipStream_t s) {
    hipLaunchKernelGGL((layernorm_kernel<T, Out>), row_grid(rows), dim3(256), 0, s, x, gamma, beta, out, rows, d, ldx, eps, res);
    return hipGetLastError();
}
hipError_t launch_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float* y, long rows, int d,
                            long ldx, long ldy, float eps, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (bad_width(d) || (ldx & 3) || (ldy & 3)) return hipErrorInvalidValue;
    if (!res && launch_ln_rows(x, gamma, beta, y, rows, d, ldx, ldy, eps, s)) return hipGetLastError();
    return launch_ln_row(x, res, gamma, beta, RowToF32{y, ldy}, rows, d, ldx, eps, s);
}
hipError_t launch_layernorm_bf16(const float* x, const float* gamma, const float* beta, unsigned short* y, long rows, int d, long ldx,
                                 long ldy, float eps, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (bad_width(d) || (ldx & 3) || (ldy & 3)) return hipErrorInvalidValue;
    return launch_ln_row(x, nullptr, gamma, beta, RowToBf16{y, ldy}, rows, d, ldx, eps, s);
}
hipError_t launch_layernorm_fp8(const float* x, const float* gamma, const float* beta, unsigned char* y, float* scale, long rows, int d,
                                long ldx, long ldy, float eps, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (bad_width(d) || (ldx & 3) || (ldy & 3)) return hipErrorInvalidValue;
    return launch_ln_row(x, nullptr, gamma, beta, RowToFp8{y, ldy, scale}, rows, d, ldx, eps, s);
}
// the half-wave kernel where it accepts the call (the towers' rows: d = 256 NV, contiguous, 16-byte aligned), else one row per wave
hipError_t launch_layernorm_mx8(const float* x, const float* gamma, const float* beta, unsigned char* y, unsigned char* scales, long srows,
                                long rows, int d, long ldx, long ldy, float eps, hipStream_t s, const unsigned short* x_bf16) {
    if (rows <= 0) return hipSuccess;
    if (d <= 0 || d % 128 || d > 256 * MAXV || (ldx & 3) || (ldy & 3) || srows < rows) return hipErrorInvalidValue;
    if (x_bf16 ? launch_ln_half(x_bf16, gamma, beta, y, scales, srows, rows, d, ldx, ldy, eps, s)
               : launch_ln_half(x, gamma, beta, y, scales, srows, rows, d, ldx, ldy, eps, s))
        return hipGetLastError();
    const RowToMx8 out{y, ldy, scales, srows};
    return x_bf16 ? launch_ln_row(x_bf16, nullptr, gamma, beta, out, rows, d, ldx, eps, s) : launch_ln_row(x, nullptr, gamma, beta, out, rows, d, ldx, eps, s);
}
hipError_t launch_im2col_mx8(const float* images, unsigned char* y, unsigned char* scales, long srows, int b, int img, int patch, int grid,
                             hipStream_t s) {
    const long rows = (long)b * grid * grid;
    if (rows <= 0) return hipSuccess;
    const int d = 3 * patch * patch;
    if (d % 128 || d > 256 * MAXV || (patch & 3) || (img & 3) || grid * patch != img || srows < rows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(im2col_mx8_kernel, row_grid(rows), dim3(256), 0, s, images, y, scales, srows, rows, img, patch, grid);
    return hipGetLastError();
}
hipError_t launch_im2col_bf16(const float* images, unsigned short* y, int b, int img, int patch, int grid, hipStream_t s) {
    const long rows = (long)b * grid * grid;
    if (rows <= 0) return hipSuccess;
    const int d = 3 * patch * patch;
    if (d % 32 || d > 256 * MAXV || (patch & 3) || (img & 3) || grid * patch != img) return hipErrorInvalidValue;
    hipLaunchKernelGGL(im2col_bf16_kernel, row_grid(rows), dim3(256), 0, s, images, y, rows, img, patch, grid);
    return hipGetLastError();
}
hipError_t launch_patch_rows_f32(const float* images, float* y, int b, int img, int patch, int grid, int kp, hipStream_t s) {
    const long rows = (long)b * grid * grid;
    if (rows <= 0) return hipSuccess;
    if (patch <= 0 || grid * patch != img || kp < 3 * patch * patch || (kp & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(patch_rows_f32_kernel, row_grid(rows), dim3(256), 0, s, images, y, rows, img, patch, grid, kp);
    return hipGetLastError();
}
hipError_t launch_quantize_mx8(const unsigned short* x_bf16, const float* x_f32, long ldx, unsigned char* y, long ldy, unsigned char* scales,
                               long srows, long rows, int d, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (d <= 0 || d % 128 || d > 4096 || (ldx & 7) || (ldy & 7) || srows < rows || (x_bf16 == nullptr) == (x_f32 == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quantize_mx8_kernel, row_grid(rows), dim3(256), 0, s, x_bf16, x_f32, ldx, y, ldy, scales, srows, rows, d);
    return hipGetLastError();
}
hipError_t launch_quantize_rows_fp8(const unsigned short* x_bf16, const float* x_f32, long ldx, unsigned char* y, long ldy, float* scale,
                                    long rows, int d, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if ((x_bf16 == nullptr) == (x_f32 == nullptr) || d <= 0 || (d & 7) || d > 4096 || (ldx & 7) || (ldy & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, row_grid(rows), dim3(256), 0, s, x_bf16, x_f32, ldx, y, ldy, scale, rows, d);
    return hipGetLastError();
}
hipError_t launch_l2norm(const float* x, long ldx, float* y, long ldy, long rows, int d, float eps, int mode, hipStream_t s,
                         const float* x2) {
    if (rows <= 0) return hipSuccess;
    if (bad_width(d) || (ldx & 3) || (ldy & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(l2norm_kernel, row_grid(rows), dim3(256), 0, s, x, x2, ldx, y, ldy, rows, d, eps, mode);
    return hipGetLastError();
}
hipError_t launch_mean_rows(const float* x, long ldx, float* y, long ldy, long n, int P, int d, long group_stride, long row_add,
                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (bad_width(d) || (ldx & 3) || (ldy & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mean_rows_kernel, row_grid(n * ((d + 255) / 256)), dim3(256), 0, s, x, ldx, y, ldy, n, P, d, group_stride, row_add);
    return hipGetLastError();
}
hipError_t launch_ce_diag_mean(const float* logits, long ld, int n, float scale, float* row_loss, float* out, hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ce_diag_rows_kernel, row_grid(n), dim3(256), 0, s, logits, ld, n, scale, row_loss);
    hipLaunchKernelGGL(mean_scalar_kernel, dim3(1), dim3(64), 0, s, row_loss, n, out);
    return hipGetLastError();
}
hipError_t launch_gather_rows(const float* x, long ldx, float* y, long ldy, long n, int d, int group, long group_stride, long row_add,
                              const int* idx, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (bad_width(d) || (ldx & 3) || (ldy & 3) || group < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_kernel, row_grid(n), dim3(256), 0, s, x, ldx, y, ldy, n, d, group, group_stride, row_add, idx);
    return hipGetLastError();
}
hipError_t launch_gather_rows_bf16(const unsigned short* x, long ldx, float* y, long ldy, long n, int d, long row_stride, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if ((d & 3) || (ldx & 3) || (ldy & 3) || row_stride < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_bf16_kernel, dim3((unsigned)((n * (d >> 2) + 255) / 256)), dim3(256), 0, s, x, ldx, y, ldy, n, d, row_stride);
    return hipGetLastError();
}
hipError_t launch_bert_embed(const float* cls, const float* local, const float* seq, const float* type_emb, const float* pos_emb,
                             const float* gamma, const float* beta, float* X, int B, int P, int T, int d, float eps, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (bad_width(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bert_embed_kernel, row_grid((long)B * (1 + P + T)), dim3(256), 0, s, cls, local, seq, type_emb, pos_emb, gamma,
                       beta, X, B, P, T, d, eps);
    return hipGetLastError();
}
// Split-K tail of the CombinerSimple hidden layer (kernels.h): one thread per (row, column); a 32-lane half wave owns one
// 32-column group and reduces it with the same xor tree as the GEMM's reduce epilogue.
__global__ __launch_bounds__(256) void splitk_relu_dot_kernel(const float* kpart, int S, long M, int N, const float* bias, const float* w2,
                                                              float* partial) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const long row = blockIdx.y;
    float v = 0.0f;
    if (col < N) {
        const float* src = kpart + row * N + col;
        for (int sl = 0; sl < S; ++sl) v += src[(long)sl * M * N];      // slices in ascending order, always
        v = fmaxf(v + bias[col], 0.0f) * w2[col];
    }
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    if ((threadIdx.x & 31) == 0 && col < N) partial[row * (N / 32) + col / 32] = v;
}
// Split-K tail of a bias + residual GEMM (kernels.h): C[row][col] = (sum of the S slices, ascending) + bias[col] + R[row][col]
__global__ __launch_bounds__(256) void splitk_bias_residual_kernel(const float* kpart, int S, long M, int N, const float* bias, const float* R,
                                                                   long ldr, float* C, long ldc) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const long row = blockIdx.y;
    if (col >= N) return;
    const float* src = kpart + row * N + col;
    float v = 0.0f;
    for (int sl = 0; sl < S; ++sl) v += src[(long)sl * M * N];          // slices in ascending order, always
    v += bias ? bias[col] : 0.0f;
    if (R) v += R[row * ldr + col];
    C[row * ldc + col] = v;
}
hipError_t launch_splitk_bias_residual(const float* kpart, int S, long M, int N, const float* bias, const float* R, long ldr, float* C, long ldc,
                                       hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (S < 1 || N < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(splitk_bias_residual_kernel, dim3((N + 255) / 256, (unsigned)M), dim3(256), 0, s, kpart, S, M, N, bias, R, ldr, C, ldc);
    return hipGetLastError();
}
hipError_t launch_splitk_relu_dot(const float* kpart, int S, long M, int N, const float* bias, const float* w2, float* partial, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (S < 1 || (N & 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(splitk_relu_dot_kernel, dim3((N + 255) / 256, (unsigned)M), dim3(256), 0, s, kpart, S, M, N, bias, w2, partial);
    return hipGetLastError();
}

hipError_t launch_text_embed(const int64_t* text, const float* tok_emb, const float* pos_emb, float* X, int* eot, int B, int T, int d,
                             int vocab, int* bad_flag, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (bad_width(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(text_embed_kernel, row_grid((long)B * T), dim3(256), 0, s, text, tok_emb, pos_emb, X, B, T, d, vocab, bad_flag);
    hipLaunchKernelGGL(text_eot_kernel, dim3((B + 3) / 4), dim3(256), 0, s, text, eot, B, T);
    return hipGetLastError();
}
hipError_t launch_vit_cls(const float* cls, const float* pos, float* X, int B, int tokens, int d, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (bad_width(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vit_cls_kernel, row_grid(B), dim3(256), 0, s, cls, pos, X, B, tokens, d);
    return hipGetLastError();
}
hipError_t launch_combiner_finalize(const float* partial, int nb, const float* b2, const float* image, const float* text, float* out,
                                    long n, int d, hipStream_t s, const float* extra) {
    if (n <= 0) return hipSuccess;
    if (bad_width(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(combiner_finalize_kernel, row_grid(n), dim3(256), 0, s, partial, nb, b2, image, text, extra, out, n, d);
    return hipGetLastError();
}
hipError_t launch_sr_finalize(const float* partial, int nb, const float* bc, const float* local, float* out, long n, int d, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (bad_width(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sr_finalize_kernel, row_grid(n), dim3(256), 0, s, partial, nb, bc, local, out, n, d);
    return hipGetLastError();
}
hipError_t launch_stem_conv(const float* img, const float* w, const float* bias, float* out, int B, int S, int cout_pad, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (S <= 0 || (S & 1) || cout_pad <= 0 || (cout_pad & 3)) return hipErrorInvalidValue;
    if (cout_pad == 48) {      // RN50x4's stem width (40 channels, padded to the next conv's k granularity): all channels of a pixel in one thread
        const long npix = (long)B * (S / 2) * (S / 2);
        hipLaunchKernelGGL(stem_conv_px_kernel<12>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, img, w, bias, out, B, S);
        return hipGetLastError();
    }
    const long total = (long)B * (S / 2) * (S / 2) * (cout_pad / 4);
    hipLaunchKernelGGL(stem_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, img, w, bias, out, B, S, cout_pad);
    return hipGetLastError();
}
hipError_t launch_avgpool_nhwc(const float* x, float* y, int B, int H, int W, int C, int k, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (C <= 0 || (C & 3) || k < 1 || H <= 0 || W <= 0 || H % k || W % k) return hipErrorInvalidValue;
    const long total = (long)B * (H / k) * (W / k) * (C / 4);
    hipLaunchKernelGGL(avgpool_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, y, B, H, W, C, k);
    return hipGetLastError();
}
hipError_t launch_attnpool_tokens(const float* x, float* mean, const float* pos, float* T, float* T0, int B, int HW, int C, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (C <= 0 || (C & 3) || HW <= 0) return hipErrorInvalidValue;      // HW == 0: the mean token would be 0 / 0
    hipLaunchKernelGGL(mean_tokens_kernel, dim3((unsigned)(((long)B * (C / 4) + 255) / 256)), dim3(256), 0, s, x, mean, B, HW, C);
    const long total = (long)B * (HW + 1) * (C / 4);
    hipLaunchKernelGGL(attnpool_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, mean, pos, T, T0, B, HW, C);
    return hipGetLastError();
}
hipError_t launch_gather_scores(const float* q, const float* gallery, const int* idx, float* out, int B, int m, int d, hipStream_t s) {
    if ((long)B * m <= 0) return hipSuccess;
    if (bad_width(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_scores_kernel, row_grid((long)B * m), dim3(256), 0, s, q, gallery, idx, out, B, m, d);
    return hipGetLastError();
}

}  // namespace fern
