// Lab bench of the block-scaled mode's LayerNorm (bf16 rows in, e4m3 + E8M0 block scales out; the four-rows-per-wave form
// elem.hip had before layernorm_half_kernel<3, unsigned short>, which came out of this bench):
// why does it take ~12 us for 29 MB?  Stand-alone.  Each variant runs in the chain  writer (rewrites the bf16 rows from another
// workgroup -> row mapping, as the GEMM epilogue before it does)  ->  LayerNorm variant  ->  reader (reads the fp8 bytes, as the next
// GEMM does), and is timed by its own start / stop events (hipExtLaunchKernelGGL).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe/ln_lab.hip -o tools/probe/ln_lab ;  tools/probe/ln_lab [rows 12608] [iters 30]
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_move<0xB1>(v); v += dpp_move<0x4E>(v); v += dpp_move<0x141>(v); v += dpp_move<0x140>(v);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { v = row16_sum(v); return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48)); }
__device__ __forceinline__ float quad_max(float v) { v = fmaxf(v, dpp_move<0xB1>(v)); return fmaxf(v, dpp_move<0x4E>(v)); }
__device__ __forceinline__ float oct_max(float v) { v = quad_max(v); return fmaxf(v, dpp_move<0x141>(v)); }
__device__ __forceinline__ unsigned pack4_fp8(float a, float b, float c, float d) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
}
__device__ __forceinline__ unsigned mx_scale_byte(float amax) {
    const unsigned u = __float_as_uint(amax);
    const int e = (int)(u >> 23) - 8 + ((u & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    return (unsigned)min(max(e, 1), 253);
}
__device__ __forceinline__ float mx_inv_scale(unsigned e) { return __uint_as_float((254u - e) << 23); }

template <int ST>
__device__ __forceinline__ void store_u32(unsigned* p, unsigned v) {
    if (ST == 1) __builtin_nontemporal_store(v, p);
    else if (ST == 2) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// the library kernel's structure: a wave owns RPW rows, a lane 4 consecutive elements of each 256-column chunk.
// ST: store flavour of the fp8 bytes (0 plain, 1 nt, 2 sc1).  LD: 0 plain loads, 1 nt loads.  NORED: statistics not reduced (diagnosis).  NOSC: no scale stores.
template <int NV, int RPW, int ST, int LD, bool NORED, bool NOSC>
__global__ __launch_bounds__(256) void ln_rows(const unsigned short* x, const float* gamma, const float* beta, unsigned char* y, unsigned char* scales, long srows, long rows,
                                               long ldx, long ldy, float eps) {
    constexpr int D = 256 * NV;
    const int lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    f32x4 v[RPW][NV];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long row = row0 + r < rows ? row0 + r : rows - 1;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            const uint2* src = reinterpret_cast<const uint2*>(x + row * ldx + c);
            uint2 w;
            if (LD == 1) { w.x = __builtin_nontemporal_load(&src->x); w.y = __builtin_nontemporal_load(&src->y); }
            else w = *src;
            v[r][i] = f32x4{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
        }
    }
    f32x4 g[NV], bb[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g[i] = *reinterpret_cast<const f32x4*>(gamma + (i * 64 + lane) * 4);
        bb[i] = *reinterpret_cast<const f32x4*>(beta + (i * 64 + lane) * 4);
    }
    float mean[RPW], rstd[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += v[r][i][0] + v[r][i][1] + v[r][i][2] + v[r][i][3];
        mean[r] = (NORED ? s * 64.f : wave_sum(s)) / (float)D;
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float t = v[r][i][e] - mean[r]; q += t * t; }
        rstd[r] = rsqrtf((NORED ? q * 64.f : wave_sum(q)) / (float)D + eps);
    }
    unsigned e8s[RPW][NV];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long row = row0 + r;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[r][i][e] - mean[r]) * rstd[r] * g[i][e] + bb[i][e];
            float am = fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3])));
            am = oct_max(am);
            const unsigned e8 = mx_scale_byte(am);
            const float inv = mx_inv_scale(e8);
            e8s[r][i] = e8;
            if (row < rows) store_u32<ST>(reinterpret_cast<unsigned*>(y + row * ldy + c), pack4_fp8(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv));
        }
    }
    if (!NOSC) {
        const bool whole = row0 + RPW <= rows && (srows & 3) == 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                unsigned dw[RPW];
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    const int e = (int)e8s[r][i];
                    dw[r] = (unsigned)__builtin_amdgcn_readlane(e, 32 * half) | ((unsigned)__builtin_amdgcn_readlane(e, 32 * half + 8) << 8) |
                            ((unsigned)__builtin_amdgcn_readlane(e, 32 * half + 16) << 16) | ((unsigned)__builtin_amdgcn_readlane(e, 32 * half + 24) << 24);
                }
                const long kt = 2 * i + half;
                unsigned* dst = reinterpret_cast<unsigned*>(scales + (kt * srows + row0) * 4);
                if (lane == 0) {
                    if (whole && RPW == 4) *reinterpret_cast<uint4*>(dst) = uint4{dw[0], dw[1], dw[2], dw[3]};
                    else
#pragma unroll
                        for (int r = 0; r < RPW; ++r)
                            if (row0 + r < rows) dst[r] = dw[r];
                }
            }
    }
}

// Half-wave per row: a lane holds 8 consecutive elements (ONE 16-byte load, one 8-byte store) of each of D / 256 chunks of its row; a
// wave owns 2 * PASSES rows.  A 32-element block is 4 lanes.  (Different summation order from ln_rows: the row's 32 lanes, then chunks.)
template <int NV, int PASSES, int ST, bool GATHER = false>
__global__ __launch_bounds__(256) void ln_half(const unsigned short* x, const float* gamma, const float* beta, unsigned char* y, unsigned char* scales, long srows, long rows,
                                               long ldx, long ldy, float eps) {
    constexpr int D = 256 * NV;
    const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
    const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (2 * PASSES);
    if (row0 >= rows) return;
    float v[PASSES][NV][8];
#pragma unroll
    for (int r = 0; r < PASSES; ++r) {
        long row = row0 + 2 * r + lh;
        row = row < rows ? row : rows - 1;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const uint4 w = *reinterpret_cast<const uint4*>(x + row * ldx + (i * 32 + l31) * 8);
            const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[r][i][2 * e] = __uint_as_float(ww[e] << 16); v[r][i][2 * e + 1] = __uint_as_float(ww[e] & 0xffff0000u); }
        }
    }
    float g[NV][8], bb[NV][8];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + (i * 32 + l31) * 8), g1 = *reinterpret_cast<const f32x4*>(gamma + (i * 32 + l31) * 8 + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + (i * 32 + l31) * 8), b1 = *reinterpret_cast<const f32x4*>(beta + (i * 32 + l31) * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { g[i][e] = g0[e]; g[i][4 + e] = g1[e]; bb[i][e] = b0[e]; bb[i][4 + e] = b1[e]; }
    }
    auto half_sum = [&](float s) {      // sum over the 32 lanes of this lane's half
        s = row16_sum(s);
        const float a = lane_f(s, 0) + lane_f(s, 16), b = lane_f(s, 32) + lane_f(s, 48);
        return lh ? b : a;
    };
    float mean[PASSES], rstd[PASSES];
#pragma unroll
    for (int r = 0; r < PASSES; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[r][i][e];
        mean[r] = half_sum(s) / (float)D;
    }
#pragma unroll
    for (int r = 0; r < PASSES; ++r) {
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float t = v[r][i][e] - mean[r]; q += t * t; }
        rstd[r] = rsqrtf(half_sum(q) / (float)D + eps);
    }
#pragma unroll
    for (int r = 0; r < PASSES; ++r) {
        const long row = row0 + 2 * r + lh;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float o[8];
            float am = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { o[e] = (v[r][i][e] - mean[r]) * rstd[r] * g[i][e] + bb[i][e]; am = fmaxf(am, fabsf(o[e])); }
            am = quad_max(am);
            const unsigned e8 = mx_scale_byte(am);
            const float inv = mx_inv_scale(e8);
            if (row < rows) {
                uint2 pk = {pack4_fp8(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv), pack4_fp8(o[4] * inv, o[5] * inv, o[6] * inv, o[7] * inv)};
                uint2* dst = reinterpret_cast<uint2*>(y + row * ldy + (i * 32 + l31) * 8);
                if (ST == 1) { __builtin_nontemporal_store(pk.x, &dst->x); __builtin_nontemporal_store(pk.y, &dst->y); }
                else *dst = pk;
                // blocks 8i .. 8i+7 of the row (4 lanes each): the dword of k tile kt = 2i + (l31 >> 4) holds blocks 4kt .. 4kt+3
                if (!GATHER) { if ((l31 & 3) == 0) scales[((long)(2 * i + (l31 >> 4)) * srows + row) * 4 + ((l31 >> 2) & 3)] = (unsigned char)e8; }
            }
            if (GATHER) {      // lanes 0 / 16 of a half collect the bytes of lanes +4, +8, +12 of their 16-lane row: one dword per (row, k tile)
                const unsigned dw = e8 | ((unsigned)__builtin_amdgcn_update_dpp(0, (int)e8, 0x104, 0xf, 0xf, false) << 8) |
                                    ((unsigned)__builtin_amdgcn_update_dpp(0, (int)e8, 0x108, 0xf, 0xf, false) << 16) |
                                    ((unsigned)__builtin_amdgcn_update_dpp(0, (int)e8, 0x10C, 0xf, 0xf, false) << 24);
                if (row < rows && (l31 & 15) == 0) *reinterpret_cast<unsigned*>(scales + ((long)(2 * i + (l31 >> 4)) * srows + row) * 4) = dw;
            }
        }
    }
}

// floors: bytes only.  W = bytes per lane and load (8 or 16); the store is half as wide
template <int W>
__global__ __launch_bounds__(256) void copy_half(const unsigned char* x, unsigned char* y, long n_in) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    for (long o = t * W; o < n_in; o += stride * W) {
        if (W == 16) {
            const uint4 w = *reinterpret_cast<const uint4*>(x + o);
            *reinterpret_cast<uint2*>(y + o / 2) = uint2{w.x ^ w.y, w.z ^ w.w};
        } else {
            const uint2 w = *reinterpret_cast<const uint2*>(x + o);
            *reinterpret_cast<unsigned*>(y + o / 2) = w.x ^ w.y;
        }
    }
}

// the kernel before (rewrites the bf16 rows in 2-byte stores of 32-column runs, lane = column: a GEMM epilogue's store shape) and after
template <int ST>
__global__ __launch_bounds__(256) void writer(unsigned short* x, long rows, long ldx, unsigned seed) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tile = (long)blockIdx.x * 4 + wave;              // 32 x 32 tiles, column-major over the matrix
    const long tiles_m = (rows + 31) / 32;
    const long tm = tile % tiles_m, tn = tile / tiles_m;
    if (tn * 32 >= ldx) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long row = tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < rows) {
            const unsigned h = (unsigned)(row * 2654435761u) ^ (unsigned)((tn * 32 + (lane & 31)) * 40503u) ^ seed;
            const unsigned short val = (unsigned short)(0x3f00u + (h & 0xff) + ((h >> 3) & 0x8000u));
            if (ST == 1) __builtin_nontemporal_store(val, &x[row * ldx + tn * 32 + (lane & 31)]);
            else if (ST == 2) __hip_atomic_store(&x[row * ldx + tn * 32 + (lane & 31)], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else x[row * ldx + tn * 32 + (lane & 31)] = val;
        }
    }
}
__global__ __launch_bounds__(256) void reader(const uint4* y, long n16, unsigned* sink) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    unsigned a = 0;
    for (long o = t; o < n16; o += (long)gridDim.x * 256) { const uint4 w = y[o]; a ^= w.x ^ w.y ^ w.z ^ w.w; }
    if (a == 0x12345679u) *sink = a;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

int main(int argc, char** argv) {
    const long rows = argc > 1 ? atol(argv[1]) : 12608;
    const int iters = argc > 2 ? atoi(argv[2]) : 30;
    constexpr int D = 768;
    unsigned short* x; float *gamma, *beta; unsigned char *y, *sc, *y2, *sc2; unsigned* sink;
    CK(hipMalloc(&x, rows * D * 2)); CK(hipMalloc(&gamma, D * 4)); CK(hipMalloc(&beta, D * 4));
    CK(hipMalloc(&y, rows * D)); CK(hipMalloc(&sc, rows * D / 32 + 64)); CK(hipMalloc(&y2, rows * D)); CK(hipMalloc(&sc2, rows * D / 32 + 64)); CK(hipMalloc(&sink, 4));
    std::vector<float> h(D);
    for (int i = 0; i < D; ++i) h[i] = 1.0f + 0.001f * (i % 17);
    CK(hipMemcpy(gamma, h.data(), D * 4, hipMemcpyHostToDevice));
    for (int i = 0; i < D; ++i) h[i] = 0.01f * (i % 5);
    CK(hipMemcpy(beta, h.data(), D * 4, hipMemcpyHostToDevice));
    hipStream_t s; CK(hipStreamCreate(&s));
    const int wgrid = (int)(((rows + 31) / 32) * (D / 32) + 3) / 4;
    struct Var { const char* name; int id; };
    const Var vars[] = {{"rows RPW4 plain (library)", 0}, {"rows RPW4 nt stores", 1}, {"rows RPW4 sc1 stores", 2}, {"rows RPW4 nt loads", 3}, {"rows RPW4 nt loads+stores", 4},
                        {"rows RPW4 no reductions", 5}, {"rows RPW4 no scale stores", 6}, {"rows RPW2 plain", 7}, {"rows RPW1 plain", 8}, {"half-wave/row 2 passes (4 rows/wave)", 9},
                        {"half-wave/row 1 pass (2 rows/wave)", 10}, {"half-wave/row 2 passes nt stores", 11}, {"copy 8B->4B", 12}, {"copy 16B->8B", 13},
                        {"copy 16B->8B, 2048 workgroups", 14}, {"half-wave/row 4 passes (8 rows/wave)", 15},
                        {"half-wave/row 1 pass nt stores", 16}, {"half-wave/row 1 pass nt, scale dwords by dpp", 17}, {"half-wave/row 2 passes nt, scale dwords by dpp", 18}};
    auto launch = [&](int id, hipEvent_t e0, hipEvent_t e1, unsigned char* yy, unsigned char* ss) {
        const float eps = 1e-5f;
        const dim3 b(256);
        auto g = [&](int rpw) { return dim3((unsigned)((rows + 4 * rpw - 1) / (4 * rpw))); };
#define LNROWS(RPW, ST, LD, NR, NS) hipExtLaunchKernelGGL((ln_rows<3, RPW, ST, LD, NR, NS>), g(RPW), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps)
        switch (id) {
            case 0: LNROWS(4, 0, 0, false, false); break;
            case 1: LNROWS(4, 1, 0, false, false); break;
            case 2: LNROWS(4, 2, 0, false, false); break;
            case 3: LNROWS(4, 0, 1, false, false); break;
            case 4: LNROWS(4, 1, 1, false, false); break;
            case 5: LNROWS(4, 0, 0, true, false); break;
            case 6: LNROWS(4, 0, 0, false, true); break;
            case 7: LNROWS(2, 0, 0, false, false); break;
            case 8: LNROWS(1, 0, 0, false, false); break;
            case 9: hipExtLaunchKernelGGL((ln_half<3, 2, 0>), g(4), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
            case 10: hipExtLaunchKernelGGL((ln_half<3, 1, 0>), g(2), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
            case 11: hipExtLaunchKernelGGL((ln_half<3, 2, 1>), g(4), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
            case 12: hipExtLaunchKernelGGL((copy_half<8>), dim3((unsigned)(rows * D * 2 / 8 / 256)), b, 0, s, e0, e1, 0, (const unsigned char*)x, yy, rows * D * 2); break;
            case 13: hipExtLaunchKernelGGL((copy_half<16>), dim3((unsigned)(rows * D * 2 / 16 / 256)), b, 0, s, e0, e1, 0, (const unsigned char*)x, yy, rows * D * 2); break;
            case 14: hipExtLaunchKernelGGL((copy_half<16>), dim3(2048), b, 0, s, e0, e1, 0, (const unsigned char*)x, yy, rows * D * 2); break;
            case 16: hipExtLaunchKernelGGL((ln_half<3, 1, 1>), g(2), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
            case 17: hipExtLaunchKernelGGL((ln_half<3, 1, 1, true>), g(2), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
            case 18: hipExtLaunchKernelGGL((ln_half<3, 2, 1, true>), g(4), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
            case 15: hipExtLaunchKernelGGL((ln_half<3, 4, 0>), g(8), b, 0, s, e0, e1, 0, x, gamma, beta, yy, ss, rows, rows, (long)D, (long)D, eps); break;
        }
    };
    // correctness of the half-wave form against the library form: bytes and scales may differ where the statistics round differently
    {
        launch(0, nullptr, nullptr, y, sc);
        launch(17, nullptr, nullptr, y2, sc2);
        CK(hipStreamSynchronize(s));
        std::vector<unsigned char> a(rows * D), b2(rows * D), sa(rows * D / 32), sb(rows * D / 32);
        CK(hipMemcpy(a.data(), y, a.size(), hipMemcpyDeviceToHost)); CK(hipMemcpy(b2.data(), y2, b2.size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(sa.data(), sc, sa.size(), hipMemcpyDeviceToHost)); CK(hipMemcpy(sb.data(), sc2, sb.size(), hipMemcpyDeviceToHost));
        long db = 0, ds = 0;
        for (size_t i = 0; i < a.size(); ++i) db += a[i] != b2[i];
        for (size_t i = 0; i < sa.size(); ++i) ds += sa[i] != sb[i];
        printf("half-wave form (dpp-gathered scales) vs library form: %ld of %zu bytes differ, %ld of %zu scale bytes differ\n", db, a.size(), ds, sa.size());
    }
    std::vector<hipEvent_t> ev(2 * iters);
    for (auto& e : ev) CK(hipEventCreate(&e));
    for (int ctx = 0; ctx < 2; ++ctx) {
        printf("== %s\n", ctx == 0 ? "in the chain writer -> LayerNorm -> reader" : "back to back (same launch repeated)");
        for (const Var& v : vars) {
            for (int it = 0; it < 3; ++it) launch(v.id, nullptr, nullptr, y, sc);
            hipEvent_t t0, t1; CK(hipEventCreate(&t0)); CK(hipEventCreate(&t1));
            CK(hipEventRecord(t0, s));
            for (int it = 0; it < iters; ++it) {
                if (ctx == 0) hipLaunchKernelGGL(writer<0>, dim3(wgrid), dim3(256), 0, s, x, rows, (long)D, (unsigned)it);
                launch(v.id, ev[2 * it], ev[2 * it + 1], y, sc);
                if (ctx == 0) hipLaunchKernelGGL(reader, dim3(1024), dim3(256), 0, s, (const uint4*)y, rows * D / 16, sink);
            }
            CK(hipEventRecord(t1, s));
            CK(hipStreamSynchronize(s));
            float tot = 0.f, sum = 0.f, mn = 1e9f;
            CK(hipEventElapsedTime(&tot, t0, t1));
            for (int it = 0; it < iters; ++it) { float ms; CK(hipEventElapsedTime(&ms, ev[2 * it], ev[2 * it + 1])); sum += ms; mn = ms < mn ? ms : mn; }
            printf("%-40s kernel avg %6.2f us  min %6.2f us   loop %7.2f us/iter\n", v.name, sum / iters * 1e3, mn * 1e3, tot / iters * 1e3);
            CK(hipEventDestroy(t0)); CK(hipEventDestroy(t1));
        }
    }
    // the writer itself (a GEMM epilogue's store shape, 19 MB of 2-byte stores), by store flavour, followed by the library LayerNorm: does
    // the flavour move the writer's own duration (dirty lines flushed at its end) or the reader's?
    for (int st = 0; st < 3; ++st) {
        std::vector<hipEvent_t> ev2(2 * iters);
        for (auto& e : ev2) CK(hipEventCreate(&e));
        for (int it = 0; it < iters; ++it) {
            if (st == 0) hipExtLaunchKernelGGL(writer<0>, dim3(wgrid), dim3(256), 0, s, ev2[2 * it], ev2[2 * it + 1], 0, x, rows, (long)D, (unsigned)it);
            if (st == 1) hipExtLaunchKernelGGL(writer<1>, dim3(wgrid), dim3(256), 0, s, ev2[2 * it], ev2[2 * it + 1], 0, x, rows, (long)D, (unsigned)it);
            if (st == 2) hipExtLaunchKernelGGL(writer<2>, dim3(wgrid), dim3(256), 0, s, ev2[2 * it], ev2[2 * it + 1], 0, x, rows, (long)D, (unsigned)it);
            launch(0, ev[2 * it], ev[2 * it + 1], y, sc);
            hipLaunchKernelGGL(reader, dim3(1024), dim3(256), 0, s, (const uint4*)y, rows * D / 16, sink);
        }
        CK(hipStreamSynchronize(s));
        float sw = 0.f, sl = 0.f;
        for (int it = 0; it < iters; ++it) { float ms; CK(hipEventElapsedTime(&ms, ev2[2 * it], ev2[2 * it + 1])); sw += ms; CK(hipEventElapsedTime(&ms, ev[2 * it], ev[2 * it + 1])); sl += ms; }
        printf("writer stores %-6s writer avg %6.2f us   LayerNorm after it avg %6.2f us\n", st == 0 ? "plain" : st == 1 ? "nt" : "sc1", sw / iters * 1e3, sl / iters * 1e3);
    }
    return 0;
}
