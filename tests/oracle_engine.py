"""TEST-ONLY engine: the FernEngine protocol implemented with the CPU oracle, so host-side logic (ERN dispatch,
harness, sharding) can be exercised without a GPU.  Lives under tests/ -- the product never imports it."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import clip as oclip
from oracle import fusion as ofusion
from oracle import rank as orank

_SLOT = {0: "Combiner_module", 1: "DVR.combiner_global", 2: "DVR.combiner_local", 3: "DVR.combiner"}
_SR = {0: "SR_module", 1: "DVR.SR_module"}


class OracleEngine:
    def __init__(self, device="cpu"):
        self.device = torch.device("cpu")
        self.sd = {}
        self.feature_dim = None
        self.clip_cfg = None
        self.precision = "fp32"

    def set_precision(self, precision):
        # every name here is restated by oracle.clip (mx8mlp / mx8img: _block_mixed and the bf16 text tower); anything else is refused,
        # never computed in another mode
        if precision not in ("fp32", "f32x3", "bf16", "fp8", "mx8", "mx8mlp", "mx8img"):
            raise ValueError(f"the oracle does not restate precision {precision!r}")
        self.precision = "fp32" if precision == "f32x3" else precision      # f32x3 is fp32-accurate: the fp32 oracle is its checker

    def close(self):
        pass

    def load_tensors(self, state_dict, prefix=""):
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            self.sd[prefix + k] = torch.from_numpy(np.ascontiguousarray(a))

    def finalize_fusion(self, feature_dim, parts=7):
        self.feature_dim = int(feature_dim)

    def finalize_clip(self, cfg):
        self.clip_cfg = cfg

    def encode_image(self, images):
        return oclip.encode_image(self.sd, self.clip_cfg, images.float().cpu(), precision=self.precision)

    def encode_text(self, tokens, want_global=True, want_seq=True, visual_emb=None):
        g, s = oclip.encode_text(self.sd, self.clip_cfg, tokens.cpu(), precision=self.precision)
        return (g if want_global else None), (s if want_seq else None)

    def dvr_fuse(self, ref_global, ref_local, text_global, text_seq):
        return ofusion.dvr_fuse(self.sd, ref_local.float().cpu(), text_seq.float().cpu(), ref_global.float().cpu(), text_global.float().cpu(),
                                precision=self.precision)

    def index_fuse(self, tar_feats, tar_local, normalize_input=False):
        tf = tar_feats.float().cpu()
        if normalize_input:
            tf = F.normalize(tf, dim=-1)
        return ofusion.index_fuse(self.sd, tf, tar_local.float().cpu())

    def combiner(self, which, image, text):
        return ofusion.combiner_simple(self.sd, _SLOT[which], image.float().cpu(), text.float().cpu())

    def visual_sr(self, which, local):
        return ofusion.visual_sr(self.sd, _SR[which], local.float().cpu())

    def batch_classification_loss(self, predicted, target):
        return ofusion.batch_classification_loss(predicted.float().cpu(), target.float().cpu())

    def l2_normalize(self, x):
        return F.normalize(x.float().cpu(), dim=-1)

    def prepare_gallery(self, gallery, out=None):
        """CPU restatement of fern_gallery_prepare (include/fern.h): bf16 copy (round to nearest even) + {max ||g - bf16(g)||,
        max ||bf16(g)||, max ||g||, 0} -- so that the distributed helpers that move PREPARED galleries run under gloo."""
        from fashionern_aaai2024_amd.engine import PreparedGallery
        g = gallery.float().cpu().contiguous()
        b = g.bfloat16()
        bf = b.float()
        zero = torch.zeros(())
        meta = torch.stack([(g - bf).norm(dim=-1).max() if len(g) else zero, bf.norm(dim=-1).max() if len(g) else zero,
                            g.norm(dim=-1).max() if len(g) else zero, zero]).float()
        return PreparedGallery(g, b, meta)

    @staticmethod
    def _rows(gallery):
        return gallery.f32 if hasattr(gallery, "bf16") and hasattr(gallery, "meta") else gallery

    def sim_topk(self, q, gallery, k, idx_offset=0, exclude_idx=None):
        return orank.cosine_topk(q.float().cpu(), self._rows(gallery).float().cpu(), k, idx_offset, exclude_idx)

    def gather_scores(self, q, gallery, idx):
        return orank.gather_scores(q.float().cpu(), self._rows(gallery).float().cpu(), torch.as_tensor(idx))

    def topk_merge(self, scores, idx):
        return orank.topk_merge(scores.float().cpu(), torch.as_tensor(idx).cpu())
