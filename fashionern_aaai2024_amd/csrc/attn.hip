// fp32 / bf16 MFMA attention: softmax(scale * Q K^T [+causal]) V.  Up to 224 keys K / V stay resident in LDS; longer
// (non-causal, <= 4096 keys) sequences stream them through LDS in chunks (the key-streaming kernels below).
//
// Replaces nn.MultiheadAttention / HF BertSelfAttention / CLIP attention on the hot path
// (SURVEY.md 2.2 rows K2-K4): ViT-B/16 (197 tokens, 12 heads x 64), CLIP text (77, causal, 8 x 64),
// the fusion BERT block (91 tokens, 8 heads x 64 or 80) and the 13 x 13 cross attention.
//
// Every tiled kernel is one of two WALKERS over one of two operand FORMS:
//   * a form (F32Form, Bf16Form) defines, once, the LDS image of a run of keys, the Q fragment load, the stager and the
//     key-tile step: one 32-key tile of online (running max / running sum) softmax and P V, so only one score tile is live
//     in registers at a time;
//   * the resident walker keeps all keys of a (batch, head) in LDS and gives each wave 32-query tiles in turn (causal allowed);
//     the chunk walker gives each wave one query tile, stages the keys in chunks and carries (m, sum, O) across them.
// The five __global__ kernels pick a form, a walker and their constants, nothing else.  Arithmetic per (query, key) is therefore
// the same code in every kernel of a form, applied to key tiles in ascending order: resident, chunked and streaming results are
// bit-identical by construction (tests/test_gpu_attention_long.py still checks it).
//
// The tile step, fp32 form:
//   * S^T = K Q^T on v_mfma_f32_32x32x2_f32 with K as the A operand: the accumulator then has the
//     QUERY on the lane and the KEYS in registers, so the softmax row reduction is lane-local plus
//     one cross-half shuffle, and
//   * the un-normalised P^T accumulator registers are, as they stand, the B operand of
//     O^T = V^T P^T (register r of lane half h holds key (r&3) + 8(r>>2) + 4h -- exactly the k pair
//     one 32x32x2 step consumes), so P never leaves registers.
// K rows are padded to HDP+4 floats so the ds_read_b128 fragment reads are bank-conflict free.
#include "kernels.h"

#include <cstdlib>

namespace fern {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) char attn_smem[];      // the K / V image of the form, ROWS padded keys

// A lane's place in its wave: query l31 of the tile, half lh of the head dimension / key pairs; tr_off is the bf16 form's
// transposing-read address inside a [4 keys][32 columns] block: lane 4q+p of a 16-lane group -> row q, columns 4p..4p+3
struct LanePos { int l31, lh, tr_off; };
__device__ __forceinline__ LanePos lane_pos() {
    const int lane = threadIdx.x & 63, lh = lane >> 5;
    return {lane & 31, lh, ((lane & 15) >> 2) * 64 + (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2 + lh * 4 * 64};
}

// ---- fp32 operand form -----------------------------------------------------------------------------------------------
// Image: K [ROWS][HDP + 4] floats, then V [ROWS][HDP] floats.
template <int HDP_>
struct F32Form {
    static constexpr int HDP = HDP_;
    static constexpr bool BF16 = false;
    static constexpr int KS = HDP + 4;          // K row stride in LDS (floats)
    typedef f32x4 Q[HDP / 8];
    static constexpr size_t image_bytes(int rows) { return (size_t)rows * (KS + HDP) * sizeof(float); }

    // Q fragment (B operand): lane (query, half) holds d = 8*kk + 4*half + e, pre-scaled
    static __device__ __forceinline__ void load_q(Q& qf, const AttnParams& p, int b, int h, int qrow, int lh, bool active) {
        const float* qb = p.q + ((long)b * p.s_q + qrow) * p.ldq + (long)h * p.hd;
#pragma unroll
        for (int kk = 0; kk < HDP / 8; ++kk) {
            const int d = kk * 8 + 4 * lh;
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (active && d < p.hd) t = *reinterpret_cast<const f32x4*>(qb + d);
            qf[kk] = t * p.scale;
        }
    }

    // keys [key0, key0 + rows) of (b, h) into image rows [0, rows), zero past s_k and past hd
    template <int ROWS>
    static __device__ __forceinline__ void stage(const AttnParams& p, int b, int h, int key0, int rows, int tid, int stride) {
        constexpr int C4 = HDP / 4;
        float* Ks = reinterpret_cast<float*>(attn_smem);
        float* Vs = Ks + ROWS * KS;
        const float* kb = p.k + (long)b * p.s_k * p.ldk + (long)h * p.hd;
        const float* vb = p.v + (long)b * p.s_k * p.ldv + (long)h * p.hd;
        for (int i = tid; i < rows * C4; i += stride) {
            const int row = i / C4, c = (i % C4) * 4, key = key0 + row;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (key < p.s_k && c < p.hd) {
                kv = *reinterpret_cast<const f32x4*>(kb + (long)key * p.ldk + c);
                vv = *reinterpret_cast<const f32x4*>(vb + (long)key * p.ldv + c);
            }
            *reinterpret_cast<f32x4*>(&Ks[row * KS + c]) = kv;
            *reinterpret_cast<f32x4*>(&Vs[row * HDP + c]) = vv;
        }
    }

    // key tile t of the image = tile ta of the head: st[r] = score(key 32 ta + (r&3) + 8(r>>2) + 4*half, query qi)
    template <bool CAUSAL, int ROWS>
    static __device__ __forceinline__ void key_tile(int t, int ta, int qi, const LanePos& lp, const AttnParams& p, const Q& qf,
                                                    float& m, float& sum, f32x16 (&o)[HDP / 32]) {
        const float* Ks = reinterpret_cast<const float*>(attn_smem);
        const float* Vs = Ks + ROWS * KS;
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < HDP / 8; ++kk) {
            const f32x4 kf = *reinterpret_cast<const f32x4*>(&Ks[(t * 32 + lp.l31) * KS + kk * 8 + 4 * lp.lh]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[kk][e], st, 0, 0, 0);
        }
        float mt = -INFINITY;
        if (CAUSAL || (ta + 1) * 32 > p.s_k) {            // only the last key tile (or a causal one) has keys to mask: wave-uniform
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = ta * 32 + (r & 3) + 8 * (r >> 2) + 4 * lp.lh;
                const bool ok = key < p.s_k && (!CAUSAL || key <= qi);
                st[r] = ok ? st[r] : -INFINITY;
                mt = fmaxf(mt, st[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, st[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m, mt);      // finite from tile 0 on: key 0 is valid for every query
        const float alpha = __expf(m - m_new);   // exp(-inf) = 0 on the first tile
        float ps = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __expf(st[r] - m_new);   // masked entries: exp(-inf) = 0
            st[r] = e;
            ps += e;
        }
        sum = sum * alpha + ps;                  // sum: this lane half's partial; halves share m
        m = m_new;
        // O^T = alpha * O^T + V_t^T P_t^T: A = V^T[d][key]; B = the P^T registers as they stand
#pragma unroll
        for (int db = 0; db < HDP / 32; ++db) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lp.lh;
                const float vf = Vs[row * HDP + db * 32 + lp.l31];
                o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf, st[r], o[db], 0, 0, 0);
            }
        }
    }
};

// ---- bf16 operand form ---------------------------------------------------------------------------------------------
// Same structure on v_mfma_f32_32x32x16_bf16 (perf mode of the CLIP towers): S^T = K Q^T with K as the A operand, so the
// accumulator has the query on the lane and 16 keys in registers; registers 8s..8s+7, rounded to bf16, ARE the B operand
// of k-step s of O^T = V^T P^T -- with the k order permuted: element j of lane half h is key 16s + 8(j>>2) + 4h + (j&3).
// The matching V^T fragment (d on the lane, those 8 keys in the elements) comes from two ds_read_b64_tr_b16 transposing
// reads of the row-major V image.  K image: rows padded to HDP*2+16 bytes (conflict-free ds_read_b128); V image:
// [HDP/32][ROWS keys][32 columns] with 64-byte rows (the 4 x 64-byte block one half-wave transposes covers all 64 banks once).
// Q is not scaled: the scores are, after the MFMA.
template <int HDP_>
struct Bf16Form {
    static constexpr int HDP = HDP_;
    static constexpr bool BF16 = true;
    static constexpr int KSB = HDP * 2 + 16;    // K row stride in LDS (bytes)
    typedef bf16x8 Q[HDP / 16];
    static constexpr size_t image_bytes(int rows) { return (size_t)rows * (KSB + HDP * 2); }

    static __device__ __forceinline__ void load_q(Q& qf, const AttnParams& p, int b, int h, int qrow, int lh, bool active) {
        const unsigned short* qb = p.qb + ((long)b * p.s_q + qrow) * p.ldq + (long)h * p.hd;
#pragma unroll
        for (int kk = 0; kk < HDP / 16; ++kk) {
            const int d = kk * 16 + 8 * lh;
            bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
            if (active && d < p.hd) t = *reinterpret_cast<const bf16x8*>(qb + d);
            qf[kk] = t;
        }
    }

    template <int ROWS>
    static __device__ __forceinline__ void stage(const AttnParams& p, int b, int h, int key0, int rows, int tid, int stride) {
        constexpr int C8 = HDP / 8;      // 16-byte pieces per row
        char* Ks = attn_smem;
        char* Vs = attn_smem + ROWS * KSB;
        const unsigned short* kb = p.kb + (long)b * p.s_k * p.ldk + (long)h * p.hd;
        const unsigned short* vb = p.vb + (long)b * p.s_k * p.ldv + (long)h * p.hd;
        for (int i = tid; i < rows * C8; i += stride) {
            const int row = i / C8, c = i % C8, key = key0 + row;
            bf16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (key < p.s_k && c * 8 < p.hd) {
                kv = *reinterpret_cast<const bf16x8*>(kb + (long)key * p.ldk + c * 8);
                vv = *reinterpret_cast<const bf16x8*>(vb + (long)key * p.ldv + c * 8);
            }
            *reinterpret_cast<bf16x8*>(Ks + row * KSB + c * 16) = kv;
            *reinterpret_cast<bf16x8*>(Vs + ((c >> 2) * ROWS + row) * 64 + (c & 3) * 16) = vv;
        }
    }

    template <bool CAUSAL, int ROWS>
    static __device__ __forceinline__ void key_tile(int t, int ta, int qi, const LanePos& lp, const AttnParams& p, const Q& qf,
                                                    float& m, float& sum, f32x16 (&o)[HDP / 32]) {
        const char* Ks = attn_smem;
        const char* Vs = attn_smem + ROWS * KSB;
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < HDP / 16; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (t * 32 + lp.l31) * KSB + (kk * 16 + 8 * lp.lh) * 2);
            st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], st, 0, 0, 0);
        }
        float mt = -INFINITY;
        if (CAUSAL || (ta + 1) * 32 > p.s_k) {            // only the last key tile (or a causal one) has keys to mask: wave-uniform
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = ta * 32 + (r & 3) + 8 * (r >> 2) + 4 * lp.lh;
                const bool ok = key < p.s_k && (!CAUSAL || key <= qi);
                st[r] = ok ? st[r] * p.scale : -INFINITY;
                mt = fmaxf(mt, st[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                st[r] *= p.scale;
                mt = fmaxf(mt, st[r]);
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m, mt);
        const float alpha = __expf(m - m_new);
        float ps = 0.0f;
        bf16x8 pf[2];
        {
            unsigned pw[8];
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float e0 = __expf(st[r] - m_new), e1 = __expf(st[r + 1] - m_new);
                ps += e0;                              // the normaliser sums the un-rounded weights (same order as one by one)
                ps += e1;
                pw[r >> 1] = f32x2_to_bf16x2_bits(e0, e1);
            }
            pf[0] = __builtin_bit_cast(bf16x8, u32x4_t{pw[0], pw[1], pw[2], pw[3]});
            pf[1] = __builtin_bit_cast(bf16x8, u32x4_t{pw[4], pw[5], pw[6], pw[7]});
        }
        sum = sum * alpha + ps;
        m = m_new;
#pragma unroll
        for (int db = 0; db < HDP / 32; ++db) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const char* vblk = Vs + (db * ROWS + t * 32 + 16 * s) * 64 + lp.tr_off;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vblk));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vblk + 8 * 64));
                const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], o[db], 0, 0, 0);
            }
        }
    }
};

// ---- stores: lane (query, half) holds d = 32*db + 8*g + 4*half + {0..3} in registers 4g..4g+3 of o[db] ----------------------
template <int NB>
__device__ __forceinline__ void store_f32(const f32x16 (&o)[NB], float inv, int b, int h, int qi, int lh, const AttnParams& p) {
    if (qi >= p.s_q) return;
    float* ob = p.out + ((long)b * p.s_q + qi) * p.ldo + (long)h * p.hd;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = db * 32 + 8 * g + 4 * lh;
            if (d < p.hd) {
                f32x4 t = {o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv};
                *reinterpret_cast<f32x4*>(ob + d) = t;
            }
        }
}

template <int NB>
__device__ __forceinline__ void store_bf16(const f32x16 (&o)[NB], float inv, int b, int h, int qi, int lh, const AttnParams& p) {
    if (qi >= p.s_q) return;
    unsigned short* ob = p.out_b + ((long)b * p.s_q + qi) * p.ldo + (long)h * p.hd;
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = db * 32 + 8 * g + 4 * lh;
            if (d < p.hd) {
                ushort4 t;
                t.x = f32_to_bf16_bits(o[db][4 * g] * inv); t.y = f32_to_bf16_bits(o[db][4 * g + 1] * inv);
                t.z = f32_to_bf16_bits(o[db][4 * g + 2] * inv); t.w = f32_to_bf16_bits(o[db][4 * g + 3] * inv);
                *reinterpret_cast<ushort4*>(ob + d) = t;
            }
        }
}

// block-scaled fp8 output (the out-projection's MX operand): the two lanes of a query (halves 0 / 1) hold the 32 values of a d block
// between them -- block maximum, E8M0 byte, 16 e4m3fn bytes per lane (hd % 32 == 0 on this path).  Both lanes reach the shuffle,
// whatever qi is: the bounds test comes after it.
template <int NB>
__device__ __forceinline__ void store_mx(const f32x16 (&o)[NB], float inv, int b, int h, int qi, int lh, const AttnParams& p) {
    const long orow = (long)b * p.s_q + qi;
#pragma unroll
    for (int db = 0; db < NB; ++db) {
        float am = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) am = fmaxf(am, fabsf(o[db][r] * inv));
        am = fmaxf(am, __shfl_xor(am, 32));
        const unsigned e8 = mx_scale_byte(am);
        const float qs = mx_inv_scale(e8);
        if (qi < p.s_q && db * 32 < p.hd) {
            unsigned char* o8 = p.out_q8 + orow * p.ldo + (long)h * p.hd + db * 32 + 4 * lh;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<unsigned*>(o8 + 8 * g) = pack4_fp8(o[db][4 * g] * inv * qs, o[db][4 * g + 1] * inv * qs,
                                                                     o[db][4 * g + 2] * inv * qs, o[db][4 * g + 3] * inv * qs);
            if (lh == 0) p.out_scales[mx_scale_offset(orow, (h * p.hd + db * 32) >> 5, p.out_srows)] = (unsigned char)e8;
        }
    }
}

// the form's outputs: fp32 operands store fp32; bf16 operands store bf16 or, when out_q8 is set, e4m3fn + E8M0 scales
template <class F>
__device__ __forceinline__ void store_out(const f32x16 (&o)[F::HDP / 32], float inv, int b, int h, int qi, int lh, const AttnParams& p) {
    if constexpr (!F::BF16) store_f32(o, inv, b, h, qi, lh, p);
    else if (p.out_q8) store_mx(o, inv, b, h, qi, lh, p);
    else store_bf16(o, inv, b, h, qi, lh, p);
}

template <int NB>
__device__ __forceinline__ void zero_acc(f32x16 (&o)[NB]) {
#pragma unroll
    for (int db = 0; db < NB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
}

// ---- resident walker -----------------------------------------------------------------------------------------------
// One workgroup = one (batch, head).  K and V of the head live in LDS for the whole workgroup (NT key tiles), each of the NW waves
// owns 32-query tiles qt = wave, wave + NW, ...
template <class F, int NT, bool CAUSAL, int NW>
__device__ __forceinline__ void resident_walk(const AttnParams& p) {
    constexpr int ROWS = NT * 32;        // padded key count
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x / p.heads, h = blockIdx.x % p.heads;
    F::template stage<ROWS>(p, b, h, 0, ROWS, threadIdx.x, NW * 64);
    __syncthreads();
    const LanePos lp = lane_pos();

    const int nqt = (p.s_q + 31) / 32;
    for (int qt = wave; qt < nqt; qt += NW) {
        const int qi = qt * 32 + lp.l31;                 // this lane's query
        typename F::Q qf;
        F::load_q(qf, p, b, h, qi < p.s_q ? qi : p.s_q - 1, lp.lh, true);
        f32x16 o[F::HDP / 32];
        zero_acc(o);
        float m = -INFINITY, sum = 0.0f;
        const int nt = CAUSAL ? (qt + 1 < NT ? qt + 1 : NT) : NT;   // causal: later tiles are all in the future
#pragma unroll 1
        for (int t = 0; t < nt; ++t) F::template key_tile<CAUSAL, ROWS>(t, t, qi, lp, p, qf, m, sum, o);
        sum += __shfl_xor(sum, 32);
        store_out<F>(o, 1.0f / sum, b, h, qi, lp.lh, p);
    }
}

// ---- chunk walker --------------------------------------------------------------------------------------------------
// One workgroup = one (batch, head, GROUP of query tiles): wave w owns query tile sg.qt0 + w (waves beyond sg.gn only help
// staging), so a head's K / V are staged once per group.  The nkt key tiles are staged in chunks of CT tiles, `stride` threads
// copying; the online softmax simply carries (m, sum, O) across the chunk boundary.  whole_image: stage all CT tiles of every
// chunk (zero rows past s_k), not only the tiles the chunk has.  Non-causal; s_q and s_k are independent.
struct StreamGroup { int bh, qt0, gn; };

template <class F, int CT>
__device__ __forceinline__ void chunk_walk(const AttnParams& p, const StreamGroup sg, const int nkt, const int stride, const bool whole_image) {
    constexpr int ROWS = CT * 32;
    const LanePos lp = lane_pos();
    const int wave = threadIdx.x >> 6;
    const int b = sg.bh / p.heads, h = sg.bh % p.heads;
    const bool active = wave < sg.gn;
    const int qi = (sg.qt0 + (active ? wave : 0)) * 32 + lp.l31;
    typename F::Q qf;
    F::load_q(qf, p, b, h, qi < p.s_q ? qi : p.s_q - 1, lp.lh, active);
    f32x16 o[F::HDP / 32];
    zero_acc(o);
    float m = -INFINITY, sum = 0.0f;
#pragma unroll 1
    for (int t0 = 0; t0 < nkt; t0 += CT) {
        const int nt = nkt - t0 < CT ? nkt - t0 : CT;
        if (t0) __syncthreads();                                     // every wave is done with the previous chunk
        F::template stage<ROWS>(p, b, h, t0 * 32, whole_image ? ROWS : nt * 32, threadIdx.x, stride);
        __syncthreads();                                             // (outside anything predicated on `active`)
        if (!active) continue;
#pragma unroll 1
        for (int t = 0; t < nt; ++t) F::template key_tile<false, ROWS>(t, t0 + t, qi, lp, p, qf, m, sum, o);
    }
    if (!active) return;                                             // whole waves: both lanes of a query stay together
    sum += __shfl_xor(sum, 32);
    store_out<F>(o, 1.0f / sum, b, h, qi, lp.lh, p);
}

// ---- the kernels ---------------------------------------------------------------------------------------------------
template <int HDP, int NT, bool CAUSAL, int NW>
__global__ __launch_bounds__(NW * 64) void attn_f32_kernel(AttnParams p) {
    resident_walk<F32Form<HDP>, NT, CAUSAL, NW>(p);
}

template <int HDP, int NT, bool CAUSAL, int NW>
__global__ __launch_bounds__(NW * 64) void attn_bf16_kernel(AttnParams p) {
    resident_walk<Bf16Form<HDP>, NT, CAUSAL, NW>(p);
}

// Key-chunked form (197-token ViT heads).  attn_f32_kernel keeps ALL keys of a head in LDS: 224 padded rows x (68 + 64) floats =
// 118 KB, so one workgroup fills a CU (160 KB) and its phases -- staging (memory), S^T and P V (MFMA), softmax (VALU) -- run back
// to back with nothing beside them: the phases of the 197 x 197 x 64 shape add up (32 + 42 + 34 + 13 us measured with parts
// switched off), and while an attention workgroup is resident only one 32 KB GEMM workgroup of another stream fits next to it.
// Here the NT key tiles are staged in KH chunks (4 + 3 tiles for 197 keys: 68 KB) and TWO workgroups (or one and two GEMM
// workgroups) share a CU: one's staging overlaps the other's MFMAs, four waves per SIMD cover each other's softmax.  One group
// per head: each wave owns at most one 32-query tile (launch condition: s_q <= 32 NW).
template <int HDP, int NT, int NW, int KH>
__global__ __launch_bounds__(NW * 64, 2) void attn_f32_chunked_kernel(AttnParams p) {
    chunk_walk<F32Form<HDP>, (NT + KH - 1) / KH>(p, StreamGroup{(int)blockIdx.x, 0, (p.s_q + 31) / 32}, NT, NW * 64, true);
}

// Key-streaming forms (any key count: ViT-L/14 has 257 tokens, 577 at 336 px).  The resident kernels end at 7 key tiles; here
// K / V are staged in chunks of STREAM_CT 32-key tiles (fp32: 68 KB at head_dim 64, bf16: 35 KB -- sized so that two workgroups
// fit a CU by LDS and registers, the intent being that one's staging overlaps the other's MFMAs; DESIGN.md 4 has what was
// measured).  Groups are balanced: ceil(nqt / 8) groups whose sizes differ by at most one (9 query tiles = 5 + 4, 19 = 7 + 6 + 6).
// On the shapes both take, the results equal the resident kernels' bit for bit: the same tile step on the same tiles in the same
// order (the resident kernels' all-padding tiles contribute alpha = 1, weights 0: nothing).
constexpr int STREAM_CT = 4;           // key tiles per staged chunk
constexpr int STREAM_MAX_WAVES = 8;    // query tiles per group at most

__device__ __forceinline__ StreamGroup stream_group(int s_q) {
    const int nqt = (s_q + 31) / 32, ng = (nqt + STREAM_MAX_WAVES - 1) / STREAM_MAX_WAVES;
    const int base = nqt / ng, rem = nqt % ng, grp = blockIdx.x % ng;
    return {(int)(blockIdx.x / ng), grp * base + (grp < rem ? grp : rem), base + (grp < rem ? 1 : 0)};
}

// (second launch bound = minimum waves per SIMD: 4 = two 8-wave workgroups per CU where the chunk's LDS allows two, head_dim <= 64)
template <int HDP>
__global__ __launch_bounds__(STREAM_MAX_WAVES * 64, HDP <= 64 ? 4 : 2) void attn_f32_stream_kernel(AttnParams p) {
    chunk_walk<F32Form<HDP>, STREAM_CT>(p, stream_group(p.s_q), (p.s_k + 31) / 32, blockDim.x, false);
}

template <int HDP>
__global__ __launch_bounds__(STREAM_MAX_WAVES * 64, 4) void attn_bf16_stream_kernel(AttnParams p) {
    chunk_walk<Bf16Form<HDP>, STREAM_CT>(p, stream_group(p.s_q), (p.s_k + 31) / 32, blockDim.x, false);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// One launcher: opts the kernel in to its LDS size once (needed past 48 KB), then launches.  Keyed on the kernel POINTER: the
// kernels all share one type, so a flag per type would be one flag for all of them.
template <auto Kern>
static hipError_t launch_kernel(const AttnParams& p, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set && lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    FERN_LAUNCH(Kern, grid, block, lds, s, p);
    return hipGetLastError();
}

template <class F, int NT, bool CAUSAL>
static hipError_t launch_resident(const AttnParams& p, hipStream_t s) {
    // 197-token ViT heads: 7 query tiles -> 8 waves (two per SIMD) so one wave's softmax VALU work overlaps its partner's MFMAs
    constexpr int NW = NT >= 7 ? 8 : 4;
    const dim3 grid(p.batch * p.heads), block(NW * 64);
    if constexpr (F::BF16) return launch_kernel<attn_bf16_kernel<F::HDP, NT, CAUSAL, NW>>(p, grid, block, F::image_bytes(NT * 32), s);
    else return launch_kernel<attn_f32_kernel<F::HDP, NT, CAUSAL, NW>>(p, grid, block, F::image_bytes(NT * 32), s);
}

template <class F>
static hipError_t launch_stream(const AttnParams& p, hipStream_t s) {
    const int nqt = (p.s_q + 31) / 32, ng = (nqt + STREAM_MAX_WAVES - 1) / STREAM_MAX_WAVES;
    const int gmax = nqt / ng + (nqt % ng ? 1 : 0);
    const dim3 grid((unsigned)(p.batch * p.heads * ng)), block((gmax < 4 ? 4 : gmax) * 64);      // at least four waves stage a chunk
    if constexpr (F::BF16) return launch_kernel<attn_bf16_stream_kernel<F::HDP>>(p, grid, block, F::image_bytes(STREAM_CT * 32), s);
    else return launch_kernel<attn_f32_stream_kernel<F::HDP>>(p, grid, block, F::image_bytes(STREAM_CT * 32), s);
}

// A/B switches (tests, profiling), each read once per process: FERN_ATTN_STREAM=1 sends every non-causal tiled shape through the
// streaming form; FERN_ATTN_CHUNKED=0 keeps the 197-token fp32 heads on the resident kernel
static bool stream_forced() {
    static const bool on = [] { const char* e = getenv("FERN_ATTN_STREAM"); return e && e[0] == '1'; }();
    return on;
}
static bool chunked_allowed() {
    static const bool on = [] { const char* e = getenv("FERN_ATTN_CHUNKED"); return !(e && e[0] == '0'); }();
    return on;
}

template <class F>
static hipError_t launch_form(const AttnParams& p, hipStream_t s) {
    const int nt = (p.s_k + 31) / 32;
    if (p.causal) {
        if (nt <= 1) return launch_resident<F, 1, true>(p, s);
        if (nt <= 3) return launch_resident<F, 3, true>(p, s);
        return hipErrorInvalidValue;
    }
    if (nt > 7 || stream_forced()) return launch_stream<F>(p, s);
    if (nt <= 1) return launch_resident<F, 1, false>(p, s);
    if (nt <= 3) return launch_resident<F, 3, false>(p, s);
    if constexpr (!F::BF16) {
        if (chunked_allowed() && nt > 4 && p.s_q <= 256)      // the key-chunked form: every wave owns one query tile
            return launch_kernel<attn_f32_chunked_kernel<F::HDP, 7, 8, 2>>(p, dim3(p.batch * p.heads), dim3(8 * 64), F::image_bytes(4 * 32), s);
    }
    return launch_resident<F, 7, false>(p, s);
}

template <template <int> class Form>
static hipError_t launch_hd(const AttnParams& p, hipStream_t s) {
    if (p.hd <= 32) return launch_form<Form<32>>(p, s);
    if (p.hd <= 64) return launch_form<Form<64>>(p, s);
    if (p.hd <= 96) return launch_form<Form<96>>(p, s);
    return hipErrorInvalidValue;
}

// ---- ONE query per (batch, head) (the class token of the last ViT block: clip_block_cls_only) ------------------------------------------
// The tiled kernels stage the head's whole K / V image in LDS and then use one query row of one MFMA tile: 47.9 us for 64 x 12 heads of
// 197 keys (77 MB of fp32 K / V at 1.6 TB/s).  Here a workgroup (4 waves) reads K and V straight from memory, lane = head dimension:
// wave w takes keys w, w + 4, ...; a key's score is a 64-lane product + xor-tree sum, its weight exp(score - max) over all keys, the output
// sum_j weight_j v_j[d] per lane, the four waves' partial outputs added in wave order.  UNR row loads stay in flight per wave.
constexpr int SQ1_MAX_KEYS = 1024;
template <int UNR>
__global__ __launch_bounds__(256) void attn_f32_single_query_kernel(AttnParams p) {
    __shared__ float sc[SQ1_MAX_KEYS];
    __shared__ float red[4][64];
    __shared__ float wred[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / p.heads, h = blockIdx.x % p.heads, hd = p.hd;
    const int lc = lane < hd ? lane : 0;                                     // clamped: every load is unconditional
    const float* kb = p.k + (long)b * p.s_k * p.ldk + (long)h * hd + lc;
    const float* vb = p.v + (long)b * p.s_k * p.ldv + (long)h * hd + lc;
    const float qd = lane < hd ? p.q[(long)b * p.ldq + (long)h * hd + lane] * p.scale : 0.0f;      // s_q == 1
    for (int j0 = wave; j0 < p.s_k; j0 += 4 * UNR) {
        float kv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int j = j0 + 4 * u;
            kv[u] = kb[(long)(j < p.s_k ? j : p.s_k - 1) * p.ldk];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float sdot = qd * kv[u];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sdot += __shfl_xor(sdot, m);
            const int j = j0 + 4 * u;
            if (lane == 0 && j < p.s_k) sc[j] = sdot;
        }
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int j = tid; j < p.s_k; j += 256) mx = fmaxf(mx, sc[j]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if (lane == 0) wred[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    float sum = 0.0f;
    for (int j = tid; j < p.s_k; j += 256) {
        const float e = __expf(sc[j] - mx);
        sc[j] = e;
        sum += e;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    if (lane == 0) wred[4 + wave] = sum;
    __syncthreads();
    sum = (wred[4] + wred[5]) + (wred[6] + wred[7]);
    float acc = 0.0f;
    for (int j0 = wave; j0 < p.s_k; j0 += 4 * UNR) {
        float vv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int j = j0 + 4 * u;
            vv[u] = vb[(long)(j < p.s_k ? j : p.s_k - 1) * p.ldv];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int j = j0 + 4 * u;
            acc = __builtin_fmaf(j < p.s_k ? sc[j] : 0.0f, vv[u], acc);
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && lane < hd)
        p.out[(long)b * p.ldo + (long)h * hd + lane] = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * (1.0f / sum);
}

// ---- ONE query per (image, head) over UNPROJECTED tokens (clip_block_cls_only in the fp32 forms, the ResNet's attention pool) ---------
// With a single query the K / V projections of every token fold into the query and into the output:
//   q_h . (Wk_h t_j + bk_h) = (Wk_h^T q_h) . t_j + const   (softmax drops the constant: no key bias anywhere below)
//   sum_j p_j (Wv_h t_j + bv_h) = Wv_h (sum_j p_j t_j) + bv_h   (sum_j p_j = 1)
// Three dispatches: fold (qt = scale Wk_h^T q_h), scores + softmax + weighted token sum (u), value projection (out = bv + Wv_h u).
// Every sum has one order, a function of (S, E, heads) alone: a lane adds its columns (keys, d) in ascending order, 64 lanes combine in
// the xor tree (lane_fold), waves combine in wave order.  Rows of a batch tile share loads and nothing else, so a row's bits do not
// depend on the batch.
static_assert(POOLED_MAX_KEYS == SQ1_MAX_KEYS, "the pooled form takes the key counts of the single-query kernel");

// The xor-tree sum over 64 lanes of N values per lane at once: a step exchanges half of the values and keeps the other half, so N values
// cost N - 1 + (steps left at one value) shuffles instead of 6 N.  Each value's tree is the one of `v += __shfl_xor(v, m)`, m = 32 .. 1
// (an addition's two operands only swap sides).  Afterwards v[0] of lane L is the total of value index
// (L & 32 ? N/2 : 0) + (L & 16 ? N/4 : 0) + ... (terms while the count is above one).
template <int N, int M>
__device__ __forceinline__ void lane_fold(float* v, int lane) {
    if constexpr (M >= 1) {
        if constexpr (N > 1) {
            constexpr int H = N / 2;
            const bool up = (lane & M) != 0;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const float send = up ? v[i] : v[i + H];
                const float keep = up ? v[i + H] : v[i];
                v[i] = keep + __shfl_xor(send, M);
            }
            lane_fold<H, M / 2>(v, lane);
        } else {
            v[0] += __shfl_xor(v[0], M);
            lane_fold<1, M / 2>(v, lane);
        }
    }
}
__device__ __forceinline__ float dot4_acc(const float4& a, const float4& b, float acc) {      // ascending column order
    acc = __builtin_fmaf(a.x, b.x, acc);
    acc = __builtin_fmaf(a.y, b.y, acc);
    acc = __builtin_fmaf(a.z, b.z, acc);
    return __builtin_fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ void axpy4(float a, const float4& x, float4& y) {
    y.x = __builtin_fmaf(a, x.x, y.x);
    y.y = __builtin_fmaf(a, x.y, y.y);
    y.z = __builtin_fmaf(a, x.z, y.z);
    y.w = __builtin_fmaf(a, x.w, y.w);
}

constexpr int POOL_BT = 16;      // images per workgroup of the fold and of the value projection: they share one read of the weight rows
constexpr int POOL_HG = 4;       // heads per workgroup of the token passes: they share one read of the image's tokens
constexpr int POOL_NW = 8;       // waves of a token-pass workgroup

// Fold: qt[b, h, e] = scale * sum_d q[b, h hd + d] Wk[h hd + d, e], d ascending.  One wave per (batch tile, 256 columns, head); lane = 4
// columns, so a weight row is read as it lies.
__global__ __launch_bounds__(64) void pooled_fold_kernel(PooledAttnParams p) {
    __shared__ float qs[POOL_BT * 128];
    const int lane = threadIdx.x, b0 = blockIdx.x * POOL_BT, h = blockIdx.z, hd = p.hd, E = p.heads * hd;
    for (int idx = lane; idx < POOL_BT * hd; idx += 64) {
        const int i = idx / hd, d = idx - i * hd;
        const int b = b0 + i < p.batch ? b0 + i : p.batch - 1;
        qs[idx] = p.q[(long)b * p.ldq + (long)h * hd + d];
    }
    __syncthreads();
    const int col = blockIdx.y * 256 + lane * 4;
    if (col >= E) return;
    float4 acc[POOL_BT];
#pragma unroll
    for (int i = 0; i < POOL_BT; ++i) acc[i] = float4{0.f, 0.f, 0.f, 0.f};
    const float* w = p.wk + (long)h * hd * p.ldw + col;
#pragma unroll 4
    for (int d = 0; d < hd; ++d) {
        const float4 w4 = *reinterpret_cast<const float4*>(w + (long)d * p.ldw);
#pragma unroll
        for (int i = 0; i < POOL_BT; ++i) axpy4(qs[i * hd + d], w4, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < POOL_BT; ++i) {
        if (b0 + i >= p.batch) break;
        const float4 r{acc[i].x * p.scale, acc[i].y * p.scale, acc[i].z * p.scale, acc[i].w * p.scale};
        *reinterpret_cast<float4*>(p.qt + ((long)(b0 + i) * p.heads + h) * E + col) = r;
    }
}

// Scores, softmax and the weighted token sum of one (image, group of POOL_HG heads): u[b, h, :] = sum_j p_j t[b, j, :].  Lane = 4 columns
// of a 256-column chunk.  Scores: a wave takes four keys at a time and walks the chunks in ascending order against the group's folded
// queries (LDS); the 16 (key, head) partials of a lane go through one lane_fold.  Weighted sum: per chunk wave w adds keys w, w + 8, ...
// in ascending order, the eight partial rows are added in wave order and scaled by 1 / sum.  Both passes read the image's tokens
// (0.6 - 0.8 MB: L2) once per head group.
__global__ __launch_bounds__(POOL_NW * 64) void pooled_tokens_kernel(PooledAttnParams p) {
    extern __shared__ __align__(16) float pool_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, h0 = blockIdx.y * POOL_HG, S = p.S, E = p.heads * p.hd;
    float* qs = pool_lds;                                  // [POOL_HG][E]
    float* red = qs + (size_t)POOL_HG * E;                 // [POOL_NW][POOL_HG][256]
    float* sc = red + POOL_NW * POOL_HG * 256;             // [POOL_HG][S]
    float* sinv = sc + (size_t)POOL_HG * S;                // [POOL_HG]
    // a group past the last head repeats it (loads stay unconditional); its rows are not stored
    for (int idx = tid * 4; idx < POOL_HG * E; idx += POOL_NW * 256) {
        const int g = idx / E, e = idx - g * E;
        const int h = h0 + g < p.heads ? h0 + g : p.heads - 1;
        *reinterpret_cast<float4*>(qs + idx) = *reinterpret_cast<const float4*>(p.qt + ((long)b * p.heads + h) * E + e);
    }
    __syncthreads();
    const float* tb = p.tok + (long)b * p.img_stride;
    for (int j0 = wave * 4; j0 < S; j0 += POOL_NW * 4) {
        float acc[4 * POOL_HG];
#pragma unroll
        for (int i = 0; i < 4 * POOL_HG; ++i) acc[i] = 0.f;
        const float* tr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tr[u] = tb + (long)(j0 + u < S ? j0 + u : S - 1) * p.ldt;
        for (int c = lane * 4; c < E; c += 256) {
            float4 t4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t4[u] = *reinterpret_cast<const float4*>(tr[u] + c);
#pragma unroll
            for (int g = 0; g < POOL_HG; ++g) {
                const float4 q4 = *reinterpret_cast<const float4*>(qs + (size_t)g * E + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u * POOL_HG + g] = dot4_acc(q4, t4[u], acc[u * POOL_HG + g]);
            }
        }
        lane_fold<4 * POOL_HG, 32>(acc, lane);
        const int idx = (lane >> 2) & 15, j = j0 + idx / POOL_HG;
        if ((lane & 3) == 0 && j < S) sc[(idx % POOL_HG) * S + j] = acc[0];
    }
    __syncthreads();
    if (wave < POOL_HG) {      // softmax statistics of head `wave`: lane-strided, then the xor tree
        float* s = sc + (size_t)wave * S;
        float mx = -INFINITY;
        for (int j = lane; j < S; j += 64) mx = fmaxf(mx, s[j]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
        float sum = 0.f;
        for (int j = lane; j < S; j += 64) {
            const float e = expf(s[j] - mx);
            s[j] = e;
            sum += e;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
        if (lane == 0) sinv[wave] = 1.0f / sum;
    }
    __syncthreads();
    for (int c0 = 0; c0 < E; c0 += 256) {
        const int c = c0 + lane * 4;
        float4 acc[POOL_HG];
#pragma unroll
        for (int g = 0; g < POOL_HG; ++g) acc[g] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < E) {
#pragma unroll 4
            for (int j = wave; j < S; j += POOL_NW) {
                const float4 t4 = *reinterpret_cast<const float4*>(tb + (long)j * p.ldt + c);
#pragma unroll
                for (int g = 0; g < POOL_HG; ++g) axpy4(sc[g * S + j], t4, acc[g]);
            }
        }
#pragma unroll
        for (int g = 0; g < POOL_HG; ++g) *reinterpret_cast<float4*>(red + ((wave * POOL_HG + g) * 256 + lane * 4)) = acc[g];
        __syncthreads();
        for (int o = tid; o < POOL_HG * 256; o += POOL_NW * 64) {
            const int g = o >> 8, cl = o & 255;
            if (c0 + cl < E && h0 + g < p.heads) {
                float sum = red[g * 256 + cl];
#pragma unroll
                for (int w = 1; w < POOL_NW; ++w) sum += red[(w * POOL_HG + g) * 256 + cl];
                p.u[((long)b * p.heads + h0 + g) * E + c0 + cl] = sum * sinv[g];
            }
        }
        __syncthreads();
    }
}

// Value projection: out[b, h hd + d] = bv[h hd + d] + Wv[h hd + d, :] . u[b, h, :].  A wave holds 4 weight rows x POOL_BT images; lane = 4
// columns of a 256-column chunk, chunks ascending; the 64 partials of a lane go through one lane_fold, which leaves value (row r, image i)
// in lane 16 r + i.
__global__ __launch_bounds__(256) void pooled_vproj_kernel(PooledAttnParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.x * POOL_BT, d0 = blockIdx.y * 16 + wave * 4, h = blockIdx.z, hd = p.hd, E = p.heads * hd;
    if (d0 >= hd) return;
    float acc[4 * POOL_BT];
#pragma unroll
    for (int i = 0; i < 4 * POOL_BT; ++i) acc[i] = 0.f;
    const float* wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wr[r] = p.wv + ((long)h * hd + (d0 + r < hd ? d0 + r : hd - 1)) * p.ldw;
    const float* ur[POOL_BT];
#pragma unroll
    for (int i = 0; i < POOL_BT; ++i) ur[i] = p.u + ((long)(b0 + i < p.batch ? b0 + i : p.batch - 1) * p.heads + h) * E;
    for (int c = lane * 4; c < E; c += 256) {
        float4 w4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) w4[r] = *reinterpret_cast<const float4*>(wr[r] + c);
#pragma unroll
        for (int i = 0; i < POOL_BT; ++i) {
            const float4 u4 = *reinterpret_cast<const float4*>(ur[i] + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r * POOL_BT + i] = dot4_acc(w4[r], u4, acc[r * POOL_BT + i]);
        }
    }
    lane_fold<4 * POOL_BT, 32>(acc, lane);
    const int d = d0 + lane / POOL_BT, b = b0 + lane % POOL_BT;
    if (d < hd && b < p.batch) p.out[(long)b * p.ldo + (long)h * hd + d] = p.bv[h * hd + d] + acc[0];
}

hipError_t launch_pooled_attention(const PooledAttnParams& p, hipStream_t s) {
    const long E = (long)p.heads * p.hd;
    if (p.batch <= 0 || p.heads <= 0 || p.hd <= 0 || (p.hd & 3) || p.hd > 128 || E > POOLED_MAX_E || p.S <= 0 || p.S > POOLED_MAX_KEYS)
        return hipErrorInvalidValue;
    if ((p.ldq & 3) || (p.ldt & 3) || (p.img_stride & 3) || (p.ldw & 3) || (p.ldo & 3) || p.ldq < E || p.ldt < E || p.ldw < E || p.ldo < E)
        return hipErrorInvalidValue;
    for (const void* ptr : {(const void*)p.q, (const void*)p.tok, (const void*)p.wk, (const void*)p.wv, (const void*)p.bv, (const void*)p.out,
                            (const void*)p.qt, (const void*)p.u})
        if (!ptr || (reinterpret_cast<uintptr_t>(ptr) & 15)) return hipErrorInvalidValue;
    const unsigned bt = (p.batch + POOL_BT - 1) / POOL_BT, ec = (unsigned)((E + 255) / 256);
    const size_t lds = sizeof(float) * ((size_t)POOL_HG * E + POOL_NW * POOL_HG * 256 + (size_t)POOL_HG * p.S + POOL_HG);
    static size_t lds_allowed = 48 * 1024;
    if (lds > lds_allowed) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pooled_tokens_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        lds_allowed = lds;
    }
    FERN_LAUNCH(pooled_fold_kernel, dim3(bt, ec, p.heads), dim3(64), 0, s, p);
    FERN_LAUNCH(pooled_tokens_kernel, dim3(p.batch, (p.heads + POOL_HG - 1) / POOL_HG), dim3(POOL_NW * 64), lds, s, p);
    FERN_LAUNCH(pooled_vproj_kernel, dim3(bt, (p.hd + 15) / 16, p.heads), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_attention(const AttnParams& p, hipStream_t s) {
    if (p.batch <= 0 || p.heads <= 0 || p.s_q <= 0 || p.s_k <= 0 || p.s_k > ATTN_MAX_KEYS) return hipErrorInvalidValue;
    if (p.causal && p.s_q != p.s_k) return hipErrorInvalidValue;
    if (p.qb || p.kb || p.vb) {
        if (!p.qb || !p.kb || !p.vb || (!p.out_b && !p.out_q8) || (p.out_q8 && (!p.out_scales || (p.hd & 31))) || (p.hd & 7) || (p.ldq & 7) || (p.ldk & 7) || (p.ldv & 7) || (p.ldo & 3)) return hipErrorInvalidValue;
        return launch_hd<Bf16Form>(p, s);
    }
    if (p.out_b || p.out_q8) return hipErrorInvalidValue;      // fp32 operands store fp32 only
    if ((p.hd & 3) || (p.ldq & 3) || (p.ldk & 3) || (p.ldv & 3) || (p.ldo & 3)) return hipErrorInvalidValue;
    if (p.s_q == 1 && !p.causal && p.hd <= 64 && p.s_k <= SQ1_MAX_KEYS) {      // one query per head: no K / V image, no MFMA tile
        FERN_LAUNCH(attn_f32_single_query_kernel<25>, dim3(p.batch * p.heads), dim3(256), 0, s, p);
        return hipGetLastError();
    }
    return launch_hd<F32Form>(p, s);
}

}  // namespace fern
