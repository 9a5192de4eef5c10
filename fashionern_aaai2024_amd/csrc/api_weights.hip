// C-ABI layer of libfern.so: weight upload and repacking.  fern_load_tensor keeps host copies by key; fern_finalize_fusion, fern_finalize_clip and
// fern_finalize_clip4cir turn them into the device buffers and bf16 / fp8 / MX copies that the launch sequences of api_fusion.hip and api_towers.hip read.
#include <cmath>
#include <cstring>
#include "ctx.h"

using namespace fern;
using namespace fern::api;

// ---- host tensors -> device buffers of the weight group being finalised ---------------------------------------------------------
// `count` elements that the current weight group owns: released when the group is finalised again, or with the context
template <class T>
static int owned_alloc(fern_ctx* c, size_t count, T** out) {
    HIP_TRY(hipMalloc(out, count * sizeof(T)));
    c->owned[c->cur_group].push_back(*out);
    return FERN_OK;
}
static int upload(fern_ctx* c, const float* h, size_t n, const float** out) {
    float* d = nullptr;
    FERN_TRY(owned_alloc(c, std::max<size_t>(n, 4), &d));
    HIP_TRY(hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice));
    *out = d;
    return FERN_OK;
}
static int need(fern_ctx* c, const std::string& key, std::vector<int64_t> shape, const HostTensor** out) {
    auto it = c->host.find(key);
    if (it == c->host.end()) return fail(FERN_ERR_STATE, "missing weight: " + key);
    if (!shape.empty() && it->second.shape != shape) {
        std::string got, want;
        for (auto s : it->second.shape) got += std::to_string(s) + ",";
        for (auto s : shape) want += std::to_string(s) + ",";
        return fail(FERN_ERR_STATE, "weight " + key + " has shape [" + got + "] expected [" + want + "]");
    }
    *out = &it->second;
    return FERN_OK;
}
// the four [n] tensors of an eval-mode BatchNorm
static int need_bn(fern_ctx* c, const std::string& p, int n, const HostTensor** w, const HostTensor** b, const HostTensor** rm, const HostTensor** rv) {
    FERN_TRY(need(c, p + ".weight", {n}, w));
    FERN_TRY(need(c, p + ".bias", {n}, b));
    FERN_TRY(need(c, p + ".running_mean", {n}, rm));
    return need(c, p + ".running_var", {n}, rv);
}
static int up_key(fern_ctx* c, const std::string& key, std::vector<int64_t> shape, const float** out) {
    const HostTensor* t;
    FERN_TRY(need(c, key, shape, &t));
    return upload(c, t->f.data(), t->f.size(), out);
}
static int up_linear(fern_ctx* c, const std::string& prefix, int out_f, int in_f, LinearW* L) {
    FERN_TRY(up_key(c, prefix + ".weight", {out_f, in_f}, &L->w));
    FERN_TRY(up_key(c, prefix + ".bias", {out_f}, &L->b));
    L->out = out_f; L->in = in_f;
    return FERN_OK;
}
static int up_ln(fern_ctx* c, const std::string& prefix, int n, LNW* L) {
    FERN_TRY(up_key(c, prefix + ".weight", {n}, &L->g));
    return up_key(c, prefix + ".bias", {n}, &L->b);
}
// concat several [rows_i, in] weights (+ biases) into one packed Linear
static int up_packed(fern_ctx* c, const std::vector<std::string>& prefixes, int out_each, int in_f, LinearW* L) {
    std::vector<float> w, b;
    for (auto& p : prefixes) {
        const HostTensor *tw, *tb;
        FERN_TRY(need(c, p + ".weight", {out_each, in_f}, &tw));
        FERN_TRY(need(c, p + ".bias", {out_each}, &tb));
        w.insert(w.end(), tw->f.begin(), tw->f.end());
        b.insert(b.end(), tb->f.begin(), tb->f.end());
    }
    FERN_TRY(upload(c, w.data(), w.size(), &L->w));
    FERN_TRY(upload(c, b.data(), b.size(), &L->b));
    L->out = out_each * (int)prefixes.size(); L->in = in_f;
    return FERN_OK;
}
static int up_transposed(fern_ctx* c, const std::string& key, int rows, int cols, const float** out) {   // [rows, cols] -> [cols, rows]
    const HostTensor* t;
    FERN_TRY(need(c, key, {rows, cols}, &t));
    std::vector<float> tr((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
        for (int q = 0; q < cols; ++q) tr[(size_t)q * rows + r] = t->f[(size_t)r * cols + q];
    return upload(c, tr.data(), tr.size(), out);
}

// bf16 (round-to-nearest-even) device copy of an uploaded fp32 weight matrix, for the perf-mode GEMMs
static int make_bf16(fern_ctx* c, LinearW* L) {
    const size_t n = (size_t)L->out * L->in;
    unsigned short* d = nullptr;
    FERN_TRY(owned_alloc(c, n, &d));
    HIP_TRY(launch_f32_to_bf16(L->w, d, (long)n, nullptr));
    L->wb = d;
    return FERN_OK;
}

// fp8 (e4m3fn) device copy with one scale per output channel (row of the [out, in] matrix)
static int make_fp8(fern_ctx* c, LinearW* L) {
    if (L->in % 64 || L->in > 4096) return FERN_OK;      // shape outside the fp8 GEMM: the layer keeps bf16 / fp32 only
    unsigned char* d = nullptr;
    float* sw = nullptr;
    FERN_TRY(owned_alloc(c, (size_t)L->out * L->in, &d));
    FERN_TRY(owned_alloc(c, (size_t)L->out, &sw));
    HIP_TRY(launch_quantize_rows_fp8(nullptr, L->w, L->in, d, L->in, sw, L->out, L->in, nullptr));
    L->w8 = d;
    L->sw = sw;
    return FERN_OK;
}

// MX (block-scaled) e4m3fn device copy: one E8M0 byte per (output channel, 32 consecutive k), kernels.h: mx_scale_offset layout
static int make_mx8(fern_ctx* c, LinearW* L) {
    if (L->in % 128 || L->in > 4096) return FERN_OK;     // shape outside the MX GEMM
    unsigned char *d = nullptr, *sc = nullptr;
    FERN_TRY(owned_alloc(c, (size_t)L->out * L->in, &d));
    FERN_TRY(owned_alloc(c, (size_t)L->out * (L->in / 32), &sc));
    HIP_TRY(launch_quantize_mx8(nullptr, L->w, L->in, d, L->in, sc, L->out, L->out, L->in, nullptr));
    L->wm = d;
    L->swm = sc;
    L->swm_rows = L->out;
    return FERN_OK;
}

static int up_sr(fern_ctx* c, const std::string& p, int D, SRW* W) {
    FERN_TRY(up_linear(c, p + ".embedding_local.0", D, D, &W->local));
    FERN_TRY(up_linear(c, p + ".embedding_global.0", D, D, &W->global));
    const HostTensor *w, *b, *rm, *rv;
    // BatchNorm1d(13) over the PATCH axis (fusion_model.py:117-123 applied to [n,13,D])
    FERN_TRY(need_bn(c, p + ".embedding_local.1", 13, &w, &b, &rm, &rv));
    std::vector<float> inv(13);
    for (int i = 0; i < 13; ++i) inv[i] = w->f[i] / std::sqrt(rv->f[i] + 1e-5f);
    FERN_TRY(upload(c, rm->f.data(), 13, &W->bn13_mean));
    FERN_TRY(upload(c, inv.data(), 13, &W->bn13_inv));
    FERN_TRY(upload(c, b->f.data(), 13, &W->bn13_beta));
    // BatchNorm1d(D) over the feature axis, folded to scale/shift
    FERN_TRY(need_bn(c, p + ".embedding_global.1", D, &w, &b, &rm, &rv));
    std::vector<float> sc(D), sh(D);
    for (int i = 0; i < D; ++i) {
        sc[i] = w->f[i] / std::sqrt(rv->f[i] + 1e-5f);
        sh[i] = b->f[i] - rm->f[i] * sc[i];
    }
    FERN_TRY(upload(c, sc.data(), D, &W->bnd_scale));
    FERN_TRY(upload(c, sh.data(), D, &W->bnd_shift));
    FERN_TRY(up_key(c, p + ".embedding_common.weight", {1, D}, &W->wc));
    return up_key(c, p + ".embedding_common.bias", {1}, &W->bc);
}
static int up_combiner(fern_ctx* c, const std::string& p, int D, CombinerW* W) {
    // CombinerSimple(clip_feature_dim=D, projection_dim=Pj, hidden_dim=Hd) (fusion_model.py:63-84); ERN uses Pj=4D, Hd=8D
    const HostTensor *tp, *hw;
    FERN_TRY(need(c, p + ".text_projection_layer.0.weight", {}, &tp));
    FERN_TRY(need(c, p + ".dynamic_scalar.0.weight", {}, &hw));
    if (tp->shape.size() != 2 || hw->shape.size() != 2) return fail(FERN_ERR_STATE, "combiner weights must be 2-D: " + p);
    const int Pj = (int)tp->shape[0], Hd = (int)hw->shape[0];
    if (Pj % 4 || (2 * Pj) % 32 || Hd <= 0) return fail(FERN_ERR_ARG, "combiner: projection_dim must be a multiple of 16: " + p);
    FERN_TRY(up_linear(c, p + ".text_projection_layer.0", Pj, D, &W->text));
    FERN_TRY(up_linear(c, p + ".image_projection_layer.0", Pj, D, &W->image));
    FERN_TRY(up_linear(c, p + ".dynamic_scalar.0", Hd, 2 * Pj, &W->hidden));
    FERN_TRY(up_key(c, p + ".dynamic_scalar.3.weight", {1, Hd}, &W->w2));
    return up_key(c, p + ".dynamic_scalar.3.bias", {1}, &W->b2);
}

// Start (re-)finalising one weight group: everything that may still read the previous generation is drained, the old
// buffers are released, and forks created before this point become stale (they hold pointers into the freed memory).
static int begin_group(fern_ctx* c, int group) {
    if (c->parent) return fail(FERN_ERR_STATE, "weights are finalised on the root context, not on a fork");
    c->cur_group = group;
    if (!c->owned[group].empty()) {
        HIP_TRY(hipDeviceSynchronize());
        for (void* p : c->owned[group]) HIP_TRY(hipFree(p));
        c->owned[group].clear();
    }
    c->generation++;
    return FERN_OK;
}

// ---- exported: fern_load_tensor, fern_finalize_fusion ---------------------------------------------------------------------------
extern "C" int fern_load_tensor(fern_ctx* c, const char* key, const void* host_ptr, int dtype, int ndim, const int64_t* shape) {
    if (!c || !key) return fail(FERN_ERR_ARG, "fern_load_tensor: NULL argument");
    if (ndim < 0 || ndim > 8 || (ndim > 0 && !shape)) return fail(FERN_ERR_ARG, "fern_load_tensor: bad ndim/shape");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return fail(FERN_ERR_ARG, "fern_load_tensor: negative dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    if (n && !host_ptr) return fail(FERN_ERR_ARG, "fern_load_tensor: host_ptr is NULL");
    t.f.resize(n);
    if (dtype == FERN_F32) std::memcpy(t.f.data(), host_ptr, n * sizeof(float));
    else if (dtype == FERN_I64) for (size_t i = 0; i < n; ++i) t.f[i] = (float)((const int64_t*)host_ptr)[i];
    else return fail(FERN_ERR_ARG, "fern_load_tensor: unsupported dtype");
    c->host[key] = std::move(t);
    return FERN_OK;
}

extern "C" int fern_finalize_fusion(fern_ctx* c, int D, int parts) {
    if (!c) return fail(FERN_ERR_ARG, "fern_finalize_fusion: ctx is NULL");
    if (D <= 0 || D % 32 || D > 768) return fail(FERN_ERR_ARG, "fern_finalize_fusion: feature_dim must be a multiple of 32, <= 768");
    if (parts <= 0 || (parts & ~FERN_PART_ALL)) return fail(FERN_ERR_ARG, "fern_finalize_fusion: bad parts mask");
    HIP_TRY(hipSetDevice(c->device));
    FusionW& F = c->fusion;
    if (F.parts && F.D != D) return fail(FERN_ERR_ARG, "fern_finalize_fusion: feature_dim differs from the already finalised parts");
    F.D = D;
    if (parts & FERN_PART_DVR) {
        F.parts &= ~FERN_PART_DVR;
        FERN_TRY(begin_group(c, fern_ctx::G_DVR));
        const std::string tl = "DVR.transformer_layer";
        const std::string bm = tl + ".bert_encoder.bert_model";
        if (c->host.count(tl + ".cls_token")) FERN_TRY(up_key(c, tl + ".cls_token", {1, 1, D}, &F.cls));
        else {   // absent in GPU-trained checkpoints: `nn.Parameter(...).to(device)` is not registered (fusion_model.py:185)
            std::vector<float> z(D, 0.f);
            FERN_TRY(upload(c, z.data(), D, &F.cls));
        }
        const HostTensor* pos;
        FERN_TRY(need(c, bm + ".embeddings.position_embeddings.weight", {}, &pos));
        if (pos->shape.size() != 2 || pos->shape[1] != D || pos->shape[0] < 96) return fail(FERN_ERR_STATE, "position_embeddings has the wrong shape");
        FERN_TRY(upload(c, pos->f.data(), pos->f.size(), &F.pos));
        FERN_TRY(up_key(c, bm + ".embeddings.token_type_embeddings.weight", {2, D}, &F.type));
        FERN_TRY(up_ln(c, bm + ".embeddings.LayerNorm", D, &F.emb_ln));
        for (int i = 0; i < 2; ++i) {
            const std::string lp = bm + ".encoder.layer." + std::to_string(i);
            BertLayerW& L = F.layer[i];
            FERN_TRY(up_packed(c, {lp + ".attention.self.query", lp + ".attention.self.key", lp + ".attention.self.value"}, D, D, &L.qkv));
            FERN_TRY(up_linear(c, lp + ".attention.output.dense", D, D, &L.attn_out));
            FERN_TRY(up_ln(c, lp + ".attention.output.LayerNorm", D, &L.ln1));
            const HostTensor* iw;
            FERN_TRY(need(c, lp + ".intermediate.dense.weight", {}, &iw));
            const int inter = (int)iw->shape[0];
            if (inter % 32) return fail(FERN_ERR_ARG, "BERT intermediate size must be a multiple of 32");
            FERN_TRY(up_linear(c, lp + ".intermediate.dense", inter, D, &L.inter));
            FERN_TRY(up_linear(c, lp + ".output.dense", D, inter, &L.out));
            FERN_TRY(up_ln(c, lp + ".output.LayerNorm", D, &L.ln2));
            // bf16 copies for the reduced-precision modes (the fusion BERT blocks follow the towers' bf16 recipe)
            for (LinearW* W : {&L.qkv, &L.attn_out, &L.inter, &L.out}) FERN_TRY(make_bf16(c, W));
        }
        HIP_TRY(hipStreamSynchronize(nullptr));
        {   // nn.MultiheadAttention packed in-proj: rows [0,D) = q, [D,3D) = k,v
            const float *w, *b;
            FERN_TRY(up_key(c, "DVR.MR_component.in_proj_weight", {3 * D, D}, &w));
            FERN_TRY(up_key(c, "DVR.MR_component.in_proj_bias", {3 * D}, &b));
            F.mha_q = {w, b, D, D};
            F.mha_kv = {w + (size_t)D * D, b + D, 2 * D, D};
            FERN_TRY(up_linear(c, "DVR.MR_component.out_proj", D, D, &F.mha_out));
        }
        FERN_TRY(up_sr(c, "DVR.SR_module", D, &F.sr[FERN_SR_DVR]));
        FERN_TRY(up_combiner(c, "DVR.combiner_global", D, &F.comb[FERN_COMBINER_DVR_GLOBAL]));
        FERN_TRY(up_combiner(c, "DVR.combiner_local", D, &F.comb[FERN_COMBINER_DVR_LOCAL]));
        FERN_TRY(up_combiner(c, "DVR.combiner", D, &F.comb[FERN_COMBINER_DVR_FINAL]));
        for (int w : {FERN_COMBINER_DVR_GLOBAL, FERN_COMBINER_DVR_LOCAL, FERN_COMBINER_DVR_FINAL}) {
            CombinerW& Cw = F.comb[w];      // a function of the layer's (N, K) only
            Cw.ksplit = (Cw.hidden.in >= 2048 && Cw.hidden.in % 512 == 0 && Cw.hidden.out % 32 == 0) ? Cw.hidden.in / 512 : 1;
        }
        F.parts |= FERN_PART_DVR;
    }
    if (parts & FERN_PART_TARGET_SR) {
        F.parts &= ~FERN_PART_TARGET_SR;
        FERN_TRY(begin_group(c, fern_ctx::G_TARGET_SR));
        FERN_TRY(up_sr(c, "SR_module", D, &F.sr[FERN_SR_TARGET]));
        F.parts |= FERN_PART_TARGET_SR;
    }
    if (parts & FERN_PART_TARGET_COMBINER) {
        F.parts &= ~FERN_PART_TARGET_COMBINER;
        FERN_TRY(begin_group(c, fern_ctx::G_TARGET_COMBINER));
        FERN_TRY(up_combiner(c, "Combiner_module", D, &F.comb[FERN_COMBINER_TARGET]));
        F.parts |= FERN_PART_TARGET_COMBINER;
    }
    return FERN_OK;
}

// ---- exported: fern_finalize_clip (the ViT / ModifiedResNet image tower, the text tower) ----------------------------------------
static int up_clip_block(fern_ctx* c, const std::string& p, int width, int mlp, ClipBlockW* B) {
    FERN_TRY(up_ln(c, p + ".ln_1", width, &B->ln1));
    FERN_TRY(up_key(c, p + ".attn.in_proj_weight", {3 * width, width}, &B->qkv.w));
    FERN_TRY(up_key(c, p + ".attn.in_proj_bias", {3 * width}, &B->qkv.b));
    B->qkv.out = 3 * width; B->qkv.in = width;
    FERN_TRY(up_linear(c, p + ".attn.out_proj", width, width, &B->out));
    FERN_TRY(up_ln(c, p + ".ln_2", width, &B->ln2));
    FERN_TRY(up_linear(c, p + ".mlp.c_fc", mlp, width, &B->fc));
    FERN_TRY(up_linear(c, p + ".mlp.c_proj", width, mlp, &B->proj));
    // every bf16 copy, then every fp8 copy, then every MX copy: the order of the allocations
    for (auto make : {make_bf16, make_fp8, make_mx8})
        for (LinearW* L : {&B->qkv, &B->out, &B->fc, &B->proj}) FERN_TRY(make(c, L));
    return FERN_OK;
}

// conv (no bias) + BatchNorm(eval) -> [cout_pad][kh*kw*cin_pad] weights in (ky, kx, ci) order (or the original (ci, ky, kx)
// order for the direct stem kernel) with the BN scale folded in, and a bias vector; padded rows / channels are zero.
static int up_conv_bn(fern_ctx* c, const std::string& conv, const std::string& bn, int cout, int cin, int ks, int cout_pad, int cin_pad,
                      bool tap_major, ConvW* out) {
    const HostTensor *w, *g, *b, *rm, *rv;
    FERN_TRY(need(c, conv + ".weight", {cout, cin, ks, ks}, &w));
    FERN_TRY(need_bn(c, bn, cout, &g, &b, &rm, &rv));
    const int K = ks * ks * cin_pad;
    std::vector<float> wf((size_t)cout_pad * K, 0.f), bf(cout_pad, 0.f);
    for (int o = 0; o < cout; ++o) {
        const float sc = g->f[o] / std::sqrt(rv->f[o] + 1e-5f);
        bf[o] = b->f[o] - rm->f[o] * sc;
        for (int i = 0; i < cin; ++i)
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx) {
                    const float v = w->f[(((size_t)o * cin + i) * ks + ky) * ks + kx] * sc;
                    const size_t k = tap_major ? ((size_t)(ky * ks + kx) * cin_pad + i) : (((size_t)i * ks + ky) * ks + kx);
                    wf[(size_t)o * K + k] = v;
                }
    }
    FERN_TRY(upload(c, wf.data(), wf.size(), &out->w));
    FERN_TRY(upload(c, bf.data(), bf.size(), &out->b));
    out->cout = cout_pad;
    out->k = K;
    return FERN_OK;
}

static int finalize_resnet(fern_ctx* c, const fern_clip_config* cfg) {
    ResNetW& R = c->clip.res;
    R = ResNetW();
    const int w = cfg->r_width, half = w / 2;
    if (w <= 0 || w % 16 || cfg->image_size % 32 || cfg->r_heads <= 0) return fail(FERN_ERR_ARG, "clip: unsupported ModifiedResNet shape");
    const int embed = w * 32, hd = embed / cfg->r_heads, tokens = (cfg->image_size / 32) * (cfg->image_size / 32) + 1;
    if (embed % cfg->r_heads || hd % 4 || hd > 96 || tokens > 224) return fail(FERN_ERR_ARG, "clip: unsupported attention-pool shape");
    R.stem_c = (half + 15) / 16 * 16;
    std::vector<float> z(64, 0.f);
    FERN_TRY(upload(c, z.data(), z.size(), &R.zeros));
    FERN_TRY(up_conv_bn(c, "visual.conv1", "visual.bn1", half, 3, 3, R.stem_c, 3, false, &R.stem1));
    FERN_TRY(up_conv_bn(c, "visual.conv2", "visual.bn2", half, half, 3, R.stem_c, R.stem_c, true, &R.stem2));
    FERN_TRY(up_conv_bn(c, "visual.conv3", "visual.bn3", w, half, 3, w, R.stem_c, true, &R.stem3));
    int inplanes = w;
    for (int li = 0; li < 4; ++li) {
        const int planes = w << li;
        for (int bi = 0; bi < cfg->r_layers[li]; ++bi) {
            const std::string p = "visual.layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            BottleneckW B;
            B.stride = (bi == 0 && li > 0) ? 2 : 1;
            B.cin = inplanes;
            B.planes = planes;
            FERN_TRY(up_conv_bn(c, p + ".conv1", p + ".bn1", planes, inplanes, 1, planes, inplanes, true, &B.c1));
            FERN_TRY(up_conv_bn(c, p + ".conv2", p + ".bn2", planes, planes, 3, planes, planes, true, &B.c2));
            FERN_TRY(up_conv_bn(c, p + ".conv3", p + ".bn3", planes * 4, planes, 1, planes * 4, planes, true, &B.c3));
            B.has_down = B.stride > 1 || inplanes != planes * 4;
            if (B.has_down)
                FERN_TRY(up_conv_bn(c, p + ".downsample.0", p + ".downsample.1", planes * 4, inplanes, 1, planes * 4, inplanes, true, &B.down));
            R.blocks.push_back(B);
            inplanes = planes * 4;
        }
    }
    if (inplanes != embed) return fail(FERN_ERR_ARG, "clip: ModifiedResNet needs four non-empty stages");
    FERN_TRY(up_key(c, "visual.attnpool.positional_embedding", {tokens, embed}, &R.pos));
    FERN_TRY(up_linear(c, "visual.attnpool.q_proj", embed, embed, &R.q));
    FERN_TRY(up_packed(c, {"visual.attnpool.k_proj", "visual.attnpool.v_proj"}, embed, embed, &R.kv));
    FERN_TRY(up_linear(c, "visual.attnpool.c_proj", cfg->embed_dim, embed, &R.cproj));
    return FERN_OK;
}

extern "C" int fern_finalize_clip(fern_ctx* c, const fern_clip_config* cfg) {
    if (!c || !cfg) return fail(FERN_ERR_ARG, "fern_finalize_clip: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    ClipW& W = c->clip;
    W = ClipW();
    FERN_TRY(begin_group(c, fern_ctx::G_CLIP));
    W.cfg = *cfg;
    auto bad = [](int w, int heads) { return w <= 0 || w % 32 || w > 1024 || heads <= 0 || w % heads || (w / heads) % 4 || w / heads > 96; };
    if (cfg->embed_dim <= 0 || cfg->embed_dim % 4 || cfg->embed_dim > 1024) return fail(FERN_ERR_ARG, "clip: unsupported embed_dim");
    if (cfg->t_layers > 0 && (bad(cfg->t_width, cfg->t_heads) || cfg->t_mlp % 32 || cfg->context_length > 96))
        return fail(FERN_ERR_ARG, "clip: unsupported text tower shape");
    if (cfg->v_arch == 1) {
        FERN_TRY(finalize_resnet(c, cfg));
    } else if (cfg->v_layers > 0) {
        const int g = cfg->patch_size > 0 ? cfg->image_size / cfg->patch_size : 0;
        if (bad(cfg->v_width, cfg->v_heads) || cfg->v_mlp % 32 || g <= 0 || g * cfg->patch_size != cfg->image_size || g * g + 1 > ATTN_MAX_KEYS)
            return fail(FERN_ERR_ARG, "clip: unsupported image tower shape");
        const int vw = cfg->v_width, P = cfg->patch_size, tokens = g * g + 1;
        FERN_TRY(up_key(c, "visual.conv1.weight", {vw, 3, P, P}, &W.conv_w));
        W.conv_mx = LinearW{W.conv_w, nullptr, vw, 3 * P * P};
        if (P % 4 || (3 * P * P) % 32) {      // e.g. patch 14: fp32 patch rows + this padded copy, in every precision mode (vit_front): no bf16 / MX copy
            const HostTensor* hw;
            FERN_TRY(need(c, "visual.conv1.weight", {vw, 3, P, P}, &hw));
            const int K = 3 * P * P, Kp = (K + 31) / 32 * 32;
            std::vector<float> wp((size_t)vw * Kp, 0.f);
            for (int o = 0; o < vw; ++o) std::copy(hw->f.data() + (size_t)o * K, hw->f.data() + (size_t)(o + 1) * K, wp.begin() + (size_t)o * Kp);
            FERN_TRY(upload(c, wp.data(), wp.size(), &W.conv_wp));
            W.conv_kp = Kp;
        } else {
            FERN_TRY(make_mx8(c, &W.conv_mx));
            FERN_TRY(make_bf16(c, &W.conv_mx));
        }
        FERN_TRY(up_key(c, "visual.class_embedding", {vw}, &W.cls));
        FERN_TRY(up_key(c, "visual.positional_embedding", {tokens, vw}, &W.vpos));
        FERN_TRY(up_ln(c, "visual.ln_pre", vw, &W.ln_pre));
        FERN_TRY(up_ln(c, "visual.ln_post", vw, &W.ln_post));
        FERN_TRY(up_transposed(c, "visual.proj", vw, cfg->embed_dim, &W.vproj_t));
        W.vblocks.resize(cfg->v_layers);
        for (int i = 0; i < cfg->v_layers; ++i)
            FERN_TRY(up_clip_block(c, "visual.transformer.resblocks." + std::to_string(i), vw, cfg->v_mlp, &W.vblocks[i]));
    }
    if (cfg->t_layers > 0) {
        const int tw = cfg->t_width;
        FERN_TRY(up_key(c, "token_embedding.weight", {cfg->vocab_size, tw}, &W.tok_emb));
        FERN_TRY(up_key(c, "positional_embedding", {cfg->context_length, tw}, &W.tpos));
        FERN_TRY(up_ln(c, "ln_final", tw, &W.ln_final));
        FERN_TRY(up_transposed(c, "text_projection", tw, cfg->embed_dim, &W.tproj_t));
        W.tblocks.resize(cfg->t_layers);
        for (int i = 0; i < cfg->t_layers; ++i)
            FERN_TRY(up_clip_block(c, "transformer.resblocks." + std::to_string(i), tw, cfg->t_mlp, &W.tblocks[i]));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));      // bf16 weight copies are converted on the null stream
    W.ready = true;
    return FERN_OK;
}

// ---- exported: fern_finalize_clip4cir -------------------------------------------------------------------------------------------
// models/others/Combiner_Model.py (CLIP4Cir Combiner, CVPR'22): the variant of CombinerSimple with a residual
// output_layer(relu(combiner_layer(cat))) branch; its Linear layers take inputs of width 2 * clip_feature_dim.
extern "C" int fern_finalize_clip4cir(fern_ctx* c) {
    if (!c) return fail(FERN_ERR_ARG, "fern_finalize_clip4cir: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    Clip4CirW& W = c->c4c;
    W = Clip4CirW();
    FERN_TRY(begin_group(c, fern_ctx::G_CLIP4CIR));
    const std::string p = "clip4cir.";
    const HostTensor *tp, *cl;
    FERN_TRY(need(c, p + "text_projection_layer.weight", {}, &tp));
    FERN_TRY(need(c, p + "combiner_layer.weight", {}, &cl));
    if (tp->shape.size() != 2 || cl->shape.size() != 2) return fail(FERN_ERR_STATE, "clip4cir: weights must be 2-D");
    const int Pj = (int)tp->shape[0], Wd = (int)tp->shape[1], Hd = (int)cl->shape[0];
    if (Wd % 32 || Wd > 1280 || Pj % 16 || Hd % 32) return fail(FERN_ERR_ARG, "clip4cir: need 2*clip_dim % 32 == 0 (<= 1280), projection % 16, hidden % 32");
    FERN_TRY(up_linear(c, p + "text_projection_layer", Pj, Wd, &W.text));
    FERN_TRY(up_linear(c, p + "image_projection_layer", Pj, Wd, &W.image));
    FERN_TRY(up_linear(c, p + "combiner_layer", Hd, 2 * Pj, &W.comb));
    FERN_TRY(up_linear(c, p + "output_layer", Wd, Hd, &W.outl));
    FERN_TRY(up_linear(c, p + "dynamic_scalar.0", Hd, 2 * Pj, &W.hidden));
    FERN_TRY(up_key(c, p + "dynamic_scalar.3.weight", {1, Hd}, &W.w2));
    FERN_TRY(up_key(c, p + "dynamic_scalar.3.bias", {1}, &W.b2));
    W.width = Wd;
    W.ready = true;
    return FERN_OK;
}
