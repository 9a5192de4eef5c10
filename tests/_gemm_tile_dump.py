"""Raw results of the GEMM tile kernels (csrc/gemm.hip, gemm_bf16.hip, gemm_pp.h and the headers they share) and of what rides on them
(the 3x3 convolution's stager, the two sweep epilogues, sweep_bf16.hip's DMA ring) on seeded inputs, for comparing two BUILDS of the
library bit for bit: a change to those files that is meant to move no bit is run once on each build and every array compared.  A script,
not a collected test.  Usage: python tests/_gemm_tile_dump.py out.npz

Every tile configuration of every family is forced in turn (fern_tuner_force_config, in process) and runs every stored epilogue form of
the family -- test_gpu_frames.FORMS, through that module's own launcher -- on contiguous operands:
  <fam>_c<cfg>_<M>x<N>x<K>_e<epi>_b<bf16 out>_i<in place>      fam = f32, f32x3 (M >= 256 only), bf16, fp8, mx8 (with its bf16 residual
                                                                 stream forms), mx8q (fern_gemm_mx8_quant: `.q` bytes and `.s` scales)
(M, N): (33, 65) -- fewer than 8 workgroups on every tile, both operands clamped; (300, 520) -- 45, 15 and 6 workgroups on the 64-, 128-
and 256-tiles (remainders 5, 7, 6 of the 8-way workgroup map); (700, 800) -- 12 workgroups on the 256-tile (quotient 1, remainder 4).
The quantising entry wants N % 128 == 0: (33, 128), (300, 384), (700, 768).  K = KMIN x {1, 2, 3, 5}: one tile, a ring shorter than,
equal to and longer than its depth, and for the 64-byte-row block-scaled tiles both halves of a scale dword.  A configuration whose k
tile does not divide K falls back by design (its arrays then repeat another configuration's).
  conv3x3            conv3x3_nhwc, b = 1, 5 x 5, cin 32, cout 48 (the CONV stager of glds_tile)
  topk_prepared.*    sim_topk on a PreparedGallery, B = 3, N = 1000, D = 64 (the bf16 sweep's DMA ring, then the rescoring)
  topk_f32.*         sim_topk on the fp32 tensor (EPI_TOPK_FILTER epilogue of glds_tile)
  rankof             rank_of on the fp32 tensor (EPI_RANK_COUNT epilogue)
An array of up to 64 KiB is saved as its raw bytes, a larger one as its SHA-256 digest (tests/_dump.py: raw): all of them raw are gigabytes.
Two files are compared with `python tests/_dump.py diff`.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import _dump  # noqa: E402
import test_gpu_frames as F  # noqa: E402

SHAPES = [(33, 65), (300, 520), (700, 800)]
QUANT_SHAPES = [(33, 128), (300, 384), (700, 768)]
KMULS = (1, 2, 3, 5)
FORCED = dict(F.FORCED, f32x3=list(range(8)))      # f32x3: all of gemm_tuner.h's kCfgsS (kNumCfgsS = 8), as test_every_forced_f32x3_tile_honours_the_frame


def _operands(eng, fam, M, N, K):
    """Seeded contiguous device operands in the layout test_gpu_frames._contiguous_call takes (no reference value: nothing is judged here)."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    o = {"sa": None, "sw": None, "b": torch.randn(N, generator=g).to(F.DEV), "r32": torch.randn(M, N, generator=g).to(F.DEV)}
    if fam == "bf16":
        a, w = a.bfloat16(), w.bfloat16()
    elif fam == "fp8":
        (a, o["sa"]), (w, o["sw"]) = eng.quantize_rows_fp8(a), eng.quantize_rows_fp8(w)
    elif fam in ("mx8", "mx8q"):
        a = a * torch.logspace(-1, 1, K // 32).repeat_interleave(32)      # blocks of different magnitude
        (a, o["sa"]), (w, o["sw"]) = eng.quantize_mx8(a), eng.quantize_mx8(w)
    o.update(a=a.to(F.DEV).contiguous(), w=w.to(F.DEV).contiguous())
    return o


def _family(eng, out, family, fams):
    for cfg in FORCED[family]:
        eng.tuner_force_config(family, cfg)
        for fam in fams:
            shapes = QUANT_SHAPES if fam == "mx8q" else [s for s in SHAPES if fam != "f32x3" or s[0] >= 256]
            for M, N in shapes:
                for kmul in KMULS:
                    K = F.KMIN[fam] * kmul
                    o = _operands(eng, fam, M, N, K)
                    for epi, out_bf16, inplace in F.FORMS[fam]:
                        o["r"] = o["r32"].bfloat16() if fam == "mx8" and epi == 3 and out_bf16 else o["r32"]
                        c, sc = F._contiguous_call(eng, fam, o, M, N, K, epi, out_bf16, inplace)
                        name = f"{fam}_c{cfg}_{M}x{N}x{K}_e{epi}_b{int(out_bf16)}_i{int(inplace)}"
                        if sc is None:
                            out[name] = _dump.raw(c)
                        else:
                            out[name + ".q"], out[name + ".s"] = _dump.raw(c), _dump.raw(sc)
    eng.tuner_force_config(family, -1)


def compute(eng):
    out = {}
    _family(eng, out, "f32", ["f32"])
    _family(eng, out, "bf16", ["bf16"])
    _family(eng, out, "fp8", ["fp8"])
    _family(eng, out, "mx8", ["mx8", "mx8q"])
    eng.set_precision("f32x3")
    _family(eng, out, "f32x3", ["f32x3"])
    eng.set_precision("fp32")

    g = torch.Generator().manual_seed(11)
    out["conv3x3"] = _dump.raw(eng.conv3x3_nhwc(torch.randn(1, 5, 5, 32, generator=g), torch.randn(48, 9 * 32, generator=g) * 0.06, torch.randn(48, generator=g)))
    unit = lambda n, d: torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)      # noqa: E731
    q, gal = unit(3, 64), unit(1000, 64)
    for name, gallery in (("topk_prepared", eng.prepare_gallery(gal.to(F.DEV))), ("topk_f32", gal)):
        s, i = eng.sim_topk(q, gallery, 50)[:2]
        out[name + ".s"], out[name + ".i"] = _dump.raw(s), _dump.raw(i)
    out["rankof"] = _dump.raw(eng.rank_of(q, gal, torch.randint(0, 1000, (3, 16), generator=g).to(torch.int32)))
    return out


if __name__ == "__main__":
    _dump.main(compute)
