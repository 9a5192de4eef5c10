"""Raw results of the ranking kernels (csrc/topk.hip, topk_deep.hip, rank.hip, items.hip, page.hip, candidates.hip and the headers they
share) on seeded inputs, for comparing two BUILDS of the library bit for bit: a change to those files that is meant to move no bit is
run once on each build and every array compared.  A script, not a collected test.  Usage: python tests/_rank_select_dump.py out.npz

Every case saves `<name>.s` (the scores' bits as uint32) and `<name>.i` (the indices), or `<name>.r` (ranks, keys) for the calls that
return one integer array.  The results are deterministic: keys are
distinct and places come from counting or sorting, so a difference between two builds is a bug, never noise.

With FERN_RANK_CAP set in the environment (the candidate lists' test hook, read once per process: tiny lists overflow) only the cases
that go through candidate lists run, as `cap_<name>`: their queries then take the gated exact pass (rank_exact_kernel, fp32 and bf16).

Which case reaches which path (api.hip: rank_plan, rank_strategy_for, rank_dense_chunk, sim_topk_deep_impl):
  plain_*     fp32 tensor gallery: topk_sample_bound_kernel without a margin (<4, 256> for N <= 1024, <16, 256> up to a 4096-row sample,
              <16, 1024> from N = 300 000, <32, 1024> from N = 1 100 000), topk_candidates_kernel (gather; fewer than K candidates at
              N = 40), rank_exact_kernel<false> when lists overflow (all-equal gallery)
  bf16_*      bf16 tensor gallery: the same kernels on the bf16 sweep, rank_exact_kernel<true> on overflow
  lists_*     prepared gallery, strategy lists: the bound with its margin, topk_rescore_kernel (rescoring rings 8 at D = 512, 10 at
              D = 640, 4 at D = 128, 2 at D = 64), list overflow -> rank_exact_kernel<false> (all-equal), a NaN row (no certificate)
  dense_*     prepared gallery, strategy dense, N < 16 384 or a two-block sweep (B = 65, D = 64): topk_dense_rescore_kernel<1> (N <= 16 384:
              N = 7 and N = 40 have l0 == 0 -> inline exact ranking; the N % 4 tail at 1001 / 1003 / 16 383), <2> (N = 20 000), <3>
              (N = 40 000), <0> (N = 60 000); K = 1 and 64; the excluded row
  tiles_*     prepared gallery, strategy dense, N >= 16 384, B <= 64: topk_tiles_rescore_kernel<true> (16 384, 16 411), <false> (262 145);
              `exclude` for every query (K' = K + 1)
  equal_*     all-equal galleries: 1025 rows (row walk: 1025 survivors > RESC_MAX -> inline exact behind T~ - margin), 65 537 rows (tile list
              overflow -> inline exact at D = 64; at D = 512 the gallery is past the inline limit -> flagged, rank_exact_kernel<false>)
  ties_*      2000 / 5000 identical best rows in a random gallery: survivors > RESC_MAX (fallback bound T~ - margin) / a wave segment
              overflow (fallback bound l0 - margin), through the row walk (N = 9000), the tiles (N = 20 000) and, at 70 000 x 512, the
              gated exact pass with a non-zero bound
  filt_*      RowFilter calls: masked dense row walk (N = 1000), masked tiles (N = 16 411), the deep stage (K = 100); there is no filtered
              lists form (fern_sim_topk_filtered runs the dense form or the deep stage)
  nan_*       one NaN gallery row (meta is poisoned: the margin is NaN): row walk, tiles, lists, deep
  deep_*      deep_exact_scores_kernel + deep_select_kernel: exact (fp32 tensor) and pre-filtered (prepared gallery; rings 4 at D = 128, 8 at
              D = 768) forms at (3, 1000, 128, K = 1024) and (2, 70 000, 768, K = 100); the bf16 form; 5000 all-equal rows (more than the
              4096 collected keys: flagged -> gated deep_exact_scores_kernel<true> + deep_fallback_kernel); a cursor page and an offset
              page (deep_select_kernel<true> / page.hip)
  merge_*     topk_merge_kernel (K <= 64) and topk_merge_deep_kernel
  rankof_*    rank_of (`.r` = the ranks): fp32 rows -> rank_keys_kernel (m = 1: one lane of a wave, 16: a full group, 17: a group of one;
              D = 288: two 256-k steps, the second partial -- the engine takes D % 32 == 0, so 264 is not a shape) + the EPI_RANK_COUNT
              epilogue + rank_finalize_kernel; bf16 rows (D = 64 and 320) -> rank_gather_bf16_kernel, the sweep, rank_keys_scores_kernel,
              rank_count_rows_kernel.  Each with the query's excluded row among the targets, a target outside the gallery, a shard
              (idx_offset = 1000) and a RowFilter (the filtered count)
  items_*     sim_topk_items (`.x` = the item ids) and item_rank_of on fp32 and bf16 rows: item_best_kernel, item_keep_best_kernel,
              item_gather_kernel, item_keys_kernel, item_count_kernel (nine targets: two groups).  N = 1030 in runs of 1, 3, 5 and 300
              rows (inside a lane, across lanes, across the 256-row wave step), two ids outside [0, G), every query's best row excluded,
              a filter on a shard; N = 1027 with the ids one element off 16-byte alignment (item_quad's scalar id loads)
  select_*    rank_select, eight places (place 0, a negative one, the last row, one past the rows): select_init / pass / emit.  Random
              scores (walks end early through `single`), all rows equal (all eight digits), one row; the excluded row on a shard
  cand_*      sim_topk_candidates with places (`.x`): candidates_kernel<ring> (D = 64), <lane> (D = 96: chain_rows_lane), <bf16>; M = 1,
              33, 600 (every row named twice, a negative entry, one outside the shard, the excluded row), K = 5 and 700, a filter on a shard

With FERN_RANK_DEEP_CAP set (the deep stage's test hook, read once per process: a collection of a few keys overflows) only the `dcap_*`
cases run: all-equal and random score rows through deep_fallback_kernel (exact, pre-filtered -> the gated deep_exact_scores_kernel<true>),
and sim_topk_from on them (deep_select_kernel<true> -> deep_fallback_kernel with a ceiling), plain and with an excluded row on a shard.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from support import unit  # noqa: E402


def _ties(n, d, nt, seed):
    """(queries [3, d], gallery [n, d]): rows 0 .. nt - 1 are one row, and it is every query's best."""
    gal = unit(n, d, seed)
    gal[:nt] = gal[0]
    q = torch.nn.functional.normalize(gal[0][None, :] + 0.1 * unit(3, d, seed + 1), dim=-1)
    return q, gal


def _item_ids(n):
    """[n] item ids in runs of 1, 3, 5 and 300 rows, and the number of items."""
    lens = torch.tensor([1, 3, 5, 300]).repeat(n // 309 + 1)
    ids = torch.repeat_interleave(torch.arange(lens.numel()), lens)[:n].to(torch.int32)
    return ids, int(ids.max()) + 1


def compute(eng, lists_only=False, deep_cap=False):
    """{name: int array}; the same seeded inputs in every process."""
    from fashionern_aaai2024_amd.engine import ItemMap, RowFilter, next_from
    out = {}
    pre = "cap_" if lists_only else "dcap_" if deep_cap else ""

    def put(name, res):
        s, i = res[0], res[1]
        out[f"{pre}{name}.s"] = s.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
        out[f"{pre}{name}.i"] = i.cpu().numpy()
        if len(res) > 2:            # item ids / places
            out[f"{pre}{name}.x"] = res[2].cpu().numpy()

    def puti(name, t):
        out[f"{pre}{name}.r"] = t.cpu().numpy()

    def prepared(gal):
        return eng.prepare_gallery(gal.cuda())

    if deep_cap:
        # ---- the radix fallback of the deep stage, with and without a ceiling ------------------------------------------------------
        for tag, q, gal in [("equal", unit(2, 64, 171), unit(1, 64, 172).repeat(5000, 1)), ("random", unit(3, 128, 173), unit(1000, 128, 174))]:
            first = eng.sim_topk_deep(q, gal, 100)
            put(f"deep_{tag}_exact", first)
            put(f"deep_{tag}_prefiltered", eng.sim_topk_deep(q, prepared(gal), 100))
            put(f"deep_{tag}_from", eng.sim_topk_from(q, gal, 100, next_from(*first)))
            ex = torch.tensor([1003, -1, 1000][:q.shape[0]], dtype=torch.int32)
            first = eng.sim_topk_deep(q, gal, 100, idx_offset=1000, exclude_idx=ex)
            put(f"deep_{tag}_offset", first)
            put(f"deep_{tag}_from_offset", eng.sim_topk_from(q, gal, 100, next_from(*first), idx_offset=1000, exclude_idx=ex))
        return out

    ex5 = torch.tensor([3, -1, 999, 0, 17], dtype=torch.int32)

    # ---- candidate lists: plain, bf16, pre-filtered -------------------------------------------------------------------------------
    eng.set_rank_strategy("lists")
    for b, n, d, k in [(3, 1000, 64, 50), (64, 9001, 640, 50), (3, 40, 64, 50), (4, 5000, 512, 1), (4, 5000, 128, 64)] + \
                      ([] if lists_only else [(2, 300_000, 64, 10), (2, 1_100_000, 64, 10)]):
        q, gal = unit(b, d, 10 + n), unit(n, d, 20 + n)
        put(f"plain_{b}_{n}_{d}_{k}", eng.sim_topk(q, gal, k))
        if n <= 9001:
            put(f"bf16_{b}_{n}_{d}_{k}", eng.sim_topk_bf16(q, eng.gallery_to_bf16(gal.cuda()), k))
        if n <= 300_000:
            put(f"lists_{b}_{n}_{d}_{k}", eng.sim_topk(q, prepared(gal), k))
    q, gal = unit(5, 128, 31), unit(3000, 128, 32)
    put("plain_exclude", eng.sim_topk(q, gal, 10, exclude_idx=ex5))
    put("lists_exclude", eng.sim_topk(q, prepared(gal), 10, exclude_idx=ex5))
    put("lists_exclude_offset", eng.sim_topk(q, prepared(gal), 10, idx_offset=1000, exclude_idx=ex5 + 1000))
    q, gal = unit(2, 64, 33), unit(1, 64, 34).repeat(1025, 1)
    put("plain_equal_1025", eng.sim_topk(q, gal, 50))
    put("bf16_equal_1025", eng.sim_topk_bf16(q, eng.gallery_to_bf16(gal.cuda()), 50))
    put("lists_equal_1025", eng.sim_topk(q, prepared(gal), 50))
    q, gal = unit(3, 64, 35), unit(9001, 64, 36)
    gal[4321] = float("nan")
    put("nan_lists", eng.sim_topk(q, prepared(gal), 10))
    if lists_only:
        return out

    # ---- dense: the row walk ------------------------------------------------------------------------------------------------------
    eng.set_rank_strategy("dense")
    for b, n, d, k in [(3, 40, 64, 10), (3, 40, 64, 50), (2, 7, 64, 10), (3, 1000, 64, 50), (3, 1000, 512, 1), (3, 1000, 640, 64), (3, 1001, 128, 50),
                       (3, 1003, 64, 50), (4, 16383, 64, 50), (65, 20000, 64, 50), (65, 40000, 64, 50), (65, 60000, 64, 50)]:
        q, gal = unit(b, d, 40 + n), unit(n, d, 50 + n)
        put(f"dense_{b}_{n}_{d}_{k}", eng.sim_topk(q, prepared(gal), k))
    q, gal = unit(5, 64, 61), unit(1003, 64, 62)
    put("dense_exclude", eng.sim_topk(q, prepared(gal), 10, exclude_idx=torch.tensor([3, -1, 999, 1002, 1001], dtype=torch.int32)))
    # ---- dense: tile maxima -------------------------------------------------------------------------------------------------------
    for b, n, d, k in [(3, 16384, 64, 50), (64, 16411, 128, 50), (3, 16411, 64, 1), (3, 16411, 64, 64), (2, 262145, 64, 50)]:
        q, gal = unit(b, d, 70 + n), unit(n, d, 80 + n)
        pg = prepared(gal)
        put(f"tiles_{b}_{n}_{d}_{k}", eng.sim_topk(q, pg, k))
        if b == 3 and k == 64:      # every query excludes its own best row
            best = eng.sim_topk(q, pg, 1)[1][:, 0].cpu()
            put(f"tiles_exclude_{n}", eng.sim_topk(q, pg, 50, exclude_idx=best))
    # ---- floods of ties -----------------------------------------------------------------------------------------------------------
    q = unit(3, 64, 91)
    put("equal_1025", eng.sim_topk(q, prepared(unit(1, 64, 92).repeat(1025, 1)), 50))
    put("equal_65537", eng.sim_topk(q, prepared(unit(1, 64, 92).repeat(65537, 1)), 50))
    put("equal_65537_gated", eng.sim_topk(unit(3, 512, 93), prepared(unit(1, 512, 94).repeat(65537, 1)), 50))
    for n, d, nt in [(9000, 64, 2000), (9000, 64, 5000), (20000, 64, 2000), (20000, 64, 5000), (70000, 512, 2000)]:
        q, gal = _ties(n, d, nt, 100 + nt)
        put(f"ties_{n}_{d}_{nt}", eng.sim_topk(q, prepared(gal), 10))
    # ---- row filters --------------------------------------------------------------------------------------------------------------
    for n in (1000, 16411):
        q, gal = unit(4, 64, 110 + n), unit(n, 64, 120 + n)
        tags = torch.arange(n, dtype=torch.int32) % 7
        filt = RowFilter(tags, mask=torch.tensor([0xFF, 0xFF, 0, 0xFF], dtype=torch.int32), value=torch.tensor([3, 5, 0, 9], dtype=torch.int32))
        put(f"filt_{n}", eng.sim_topk(q, prepared(gal), 50, row_filter=filt))
        put(f"filt_exclude_{n}", eng.sim_topk(q, prepared(gal), 50, exclude_idx=torch.tensor([3, 5, -1, 0], dtype=torch.int32), row_filter=filt))
        if n == 1000:
            put("filt_deep_prefiltered", eng.sim_topk_deep(q, prepared(gal), 100, row_filter=filt))
            put("filt_deep_exact", eng.sim_topk_deep(q, gal, 100, row_filter=filt))
    # ---- a NaN row ----------------------------------------------------------------------------------------------------------------
    for n in (1000, 20000):
        q, gal = unit(3, 64, 130 + n), unit(n, 64, 140 + n)
        gal[n // 3] = float("nan")
        put(f"nan_dense_{n}", eng.sim_topk(q, prepared(gal), 10))
        if n == 1000:
            put("nan_deep", eng.sim_topk_deep(q, prepared(gal), 100))
    # ---- deep ranking -------------------------------------------------------------------------------------------------------------
    eng.set_rank_strategy("auto")
    for b, n, d, k in [(3, 1000, 128, 1024), (2, 70000, 768, 100)]:
        q, gal = unit(b, d, 150 + n), unit(n, d, 160 + n)
        put(f"deep_exact_{b}_{n}_{d}_{k}", eng.sim_topk_deep(q, gal, k))
        put(f"deep_prefiltered_{b}_{n}_{d}_{k}", eng.sim_topk_deep(q, prepared(gal), k))
        if n == 1000:
            put("deep_bf16", eng.sim_topk_deep(q, eng.gallery_to_bf16(gal.cuda()), 100))
            put("deep_exclude", eng.sim_topk_deep(q, prepared(gal), 100, exclude_idx=torch.tensor([3, -1, 999], dtype=torch.int32)))
            first = eng.sim_topk_deep(q, gal, 100)
            put("deep_cursor_page", eng.sim_topk_from(q, gal, 100, next_from(*first)))
            put("deep_offset_page", eng.rank_page(q, gal, 37, 100))
    q, gal = unit(2, 64, 171), unit(1, 64, 172).repeat(5000, 1)
    put("deep_equal_exact", eng.sim_topk_deep(q, gal, 100))
    put("deep_equal_prefiltered", eng.sim_topk_deep(q, prepared(gal), 100))
    # ---- merges of ranked lists ---------------------------------------------------------------------------------------------------
    for k in (10, 100):
        q = unit(4, 64, 180 + k)
        parts = [eng.sim_topk_deep(q, unit(60 + 50 * r, 64, 190 + r), k, idx_offset=1000 * r) for r in range(3)]      # 60 rows < K = 100: -1 slots
        put(f"merge_{k}", eng.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])))
    # ---- exact target ranks ---------------------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(300)
    # (the engine takes D % 32 == 0 for fp32 rows and D % 64 == 0 for bf16 rows: D = 288 is the smallest second, partial 256-k step)
    for b, n, d in [(3, 1000, 64), (2, 300, 288), (2, 300, 320)]:
        q, gal = unit(b, d, 200 + n + d), unit(n, d, 210 + n + d)
        tags = torch.arange(n, dtype=torch.int32) % 7
        filt = RowFilter(tags, mask=torch.tensor([0xFF, 0, 0xFF][:b], dtype=torch.int32), value=torch.tensor([3, 0, 5][:b], dtype=torch.int32))
        ex = torch.tensor([3, -1, 7][:b], dtype=torch.int32)
        forms = ([("f32", gal)] if d != 320 else []) + ([("bf16", eng.gallery_to_bf16(gal.cuda()))] if d % 64 == 0 else [])
        for form, g in forms:
            for m in (1, 16, 17):
                tg = torch.randint(0, n, (b, m), generator=gen, dtype=torch.int32)
                tg[0, 0] = 3                                                                # query 0's excluded row
                tg[b - 1, m - 1] = n + 5                                                    # outside the gallery
                puti(f"rankof_{form}_{n}_{d}_{m}", eng.rank_of(q, g, tg))
                puti(f"rankof_{form}_{n}_{d}_{m}_exclude_offset", eng.rank_of(q, g, tg + 1000, idx_offset=1000, exclude_idx=ex + 1000))
                puti(f"rankof_{form}_{n}_{d}_{m}_filt", eng.rank_of(q, g, tg, exclude_idx=ex, row_filter=filt))
    # ---- items ----------------------------------------------------------------------------------------------------------------------
    for n, shift in [(1030, 0), (1027, 1)]:
        q, gal = unit(3, 64, 220 + n), unit(n, 64, 230 + n)
        ids, G = _item_ids(n)
        ids[10], ids[500] = -1, G + 5                                                       # rows of no item
        buf = torch.cat([torch.zeros(shift, dtype=torch.int32), ids]).cuda()
        items = ItemMap(buf[shift:], n_items=G)                                             # shift = 1: ids that are not 16-byte aligned
        tg = torch.tensor([[0, 1, 2, 3, 4, 5, G - 1, -1, G + 5]] * 3, dtype=torch.int32)    # nine targets: two groups of the count kernel
        filt = RowFilter(torch.arange(n, dtype=torch.int32) % 7, mask=torch.tensor([0xFF, 0, 0xFF], dtype=torch.int32),
                         value=torch.tensor([3, 0, 5], dtype=torch.int32))
        for form, g in [("f32", gal), ("bf16", eng.gallery_to_bf16(gal.cuda()))]:
            first = eng.sim_topk_items(q, g, items, 10)
            put(f"items_{form}_{n}", first)
            puti(f"items_{form}_{n}_rank", eng.item_rank_of(q, g, items, tg))
            best = first[1][:, 0].cpu().to(torch.int32)                                     # every query excludes the row that is its best item's best
            put(f"items_{form}_{n}_exclude", eng.sim_topk_items(q, g, items, 10, exclude_idx=best))
            puti(f"items_{form}_{n}_exclude_rank", eng.item_rank_of(q, g, items, tg, exclude_idx=best))
            put(f"items_{form}_{n}_filt_offset", eng.sim_topk_items(q, g, items, 10, idx_offset=1000, exclude_idx=best + 1000, row_filter=filt))
            puti(f"items_{form}_{n}_filt_offset_rank", eng.item_rank_of(q, g, items, tg, idx_offset=1000, exclude_idx=best + 1000, row_filter=filt))
    # ---- pages: the row at a place ----------------------------------------------------------------------------------------------------
    q = unit(3, 64, 240)
    for tag, gal in [("random_3000", unit(3000, 64, 241)), ("equal_3000", unit(1, 64, 242).repeat(3000, 1)), ("one_row", unit(1, 64, 243))]:
        n = gal.shape[0]
        places = torch.tensor([[0, -1, n - 1, n, 5, 100, n // 2, n - 2]] * 3, dtype=torch.int32)      # the last row, one past the rows
        puti(f"select_{tag}", eng.rank_select(q, gal, places))
        puti(f"select_{tag}_exclude_offset", eng.rank_select(q, gal, places, idx_offset=1000, exclude_idx=torch.tensor([1003, -1, 1000], dtype=torch.int32)))
    # ---- candidates -------------------------------------------------------------------------------------------------------------------
    n = 2000
    tags = torch.arange(n, dtype=torch.int32) % 7
    filt = RowFilter(tags, mask=torch.tensor([0xFF, 0, 0xFF], dtype=torch.int32), value=torch.tensor([3, 0, 5], dtype=torch.int32))
    ex = torch.tensor([3, -1, 7], dtype=torch.int32)
    for form, d in [("ring", 64), ("lane", 96), ("bf16", 64)]:
        q, gal = unit(3, d, 250 + d), unit(n, d, 260 + d)
        g = eng.gallery_to_bf16(gal.cuda()) if form == "bf16" else gal
        for m in (1, 33, 600):
            cd = torch.randint(0, n, (3, m), generator=gen, dtype=torch.int32)
            if m > 1:
                cd[:, 3], cd[:, 5], cd[:, 7], cd[0, 9] = cd[:, 2], -1, n + 50, 3            # named twice, negative, outside, the excluded row
            if m == 600:
                cd[:, 300:] = cd[:, :300]                                                   # every row twice
            for k in (5, 700):
                put(f"cand_{form}_{m}_{k}", eng.sim_topk_candidates(q, g, cd, k, places=True))
                if m > 1:
                    put(f"cand_{form}_{m}_{k}_filt_offset",
                        eng.sim_topk_candidates(q, g, cd + 1000, k, idx_offset=1000, exclude_idx=ex + 1000, row_filter=filt, places=True))
    return out


if __name__ == "__main__":
    import _dump
    _dump.main(lambda eng: compute(eng, lists_only="FERN_RANK_CAP" in os.environ, deep_cap="FERN_RANK_DEEP_CAP" in os.environ))
