"""Rank metrics of the evaluation harness: where the target LANDED in each query's full ranking, not only whether it is in the top 50.

The reference argsorts the whole ``1 - Q @ G.T`` row (run/test/test_fiq.py:49-50) and keeps Recall@10/50 of it; the same ranking also
holds Recall@K for any K, the median and mean rank and MRR.  The functions below take the argument lists of their
``compute_*_val_metrics`` counterparts plus ``ks=`` and return `_common.retrieval_metrics`' dictionary; the recalls in it equal the
counterpart's tuple bit for bit.  The engine counts the gallery rows that outrank each target (FernEngine.rank_of): exact at any depth.
"""
from __future__ import annotations

import numpy as np

from . import _common, test_200k, test_cirr, test_fiq


def compute_fiq_rank_metrics(relative_val_dataset, clip_model, index_features, index_local_features, index_names, model, device,
                             feature_dim, batch_size, num_workers, clip_model_name, ks=(10, 50)):
    predicted, target_names = test_fiq.generate_fiq_val_predictions(clip_model, relative_val_dataset, model, index_names, index_features,
                                                                     device, feature_dim, batch_size, num_workers, clip_model_name)
    index_fused = _common.fuse_index(model, index_features, index_local_features, prepared=True)
    tgt = _common._unique_rows(index_names, target_names, "target")
    return _common.retrieval_metrics(_common.target_ranks(model, predicted, index_fused, tgt), ks)


def compute_cirr_rank_metrics(relative_val_dataset, clip_model, index_features, index_local_features, index_names, model, device,
                              feature_dim, batch_size, num_workers, clip_model_name, ks=(1, 5, 10, 50)):
    """Global ranking with the reference image removed from each query's ranking (test_cirr.py:55-62)."""
    predicted, reference_names, target_names, _ = test_cirr.generate_cirr_val_predictions(
        clip_model, relative_val_dataset, model, index_names, index_features, device, feature_dim, batch_size, num_workers,
        clip_model_name)
    index_fused = _common.fuse_index(model, index_features, index_local_features, prepared=True)
    tgt = _common._unique_rows(index_names, target_names, "target")
    ref = _common._unique_rows(index_names, reference_names, "reference")
    return _common.retrieval_metrics(_common.target_ranks(model, predicted, index_fused, tgt, exclude=ref), ks)


def compute_200k_rank_metrics(relative_val_dataset, clip_model, index_features, index_local_features, index_names, model, device,
                              feature_dim, batch_size, num_workers, clip_model_name, ks=(10, 50)):
    """Gallery names are caption ids with duplicates: a query's rank is the best rank of ANY row carrying the target name
    (test_200k.py:59-60)."""
    predicted, target_names = test_200k.generate_200k_val_predictions(clip_model, relative_val_dataset, model, index_names, index_features,
                                                                      device, feature_dim, batch_size, num_workers, clip_model_name)
    index_fused = _common.fuse_index(model, index_features, index_local_features, prepared=True)
    rows_of = {}
    for i, n in enumerate(index_names):
        rows_of.setdefault(n, []).append(i)
    per_query = [rows_of.get(n, []) for n in target_names]
    width = max([len(r) for r in per_query] + [1])
    rows = np.full((len(per_query), width), -1, dtype=np.int32)
    for i, r in enumerate(per_query):
        rows[i, :len(r)] = r
    return _common.retrieval_metrics(_common.target_ranks(model, predicted, index_fused, rows), ks)


def compute_200k_item_metrics(relative_val_dataset, clip_model, index_features, index_local_features, index_names, model, device,
                              feature_dim, batch_size, num_workers, clip_model_name, ks=(10, 50)):
    """--item-level: the gallery's items are its distinct names, every item takes one place in a query's ranking, and the metrics are
    those of the target ITEM's place (`_common.recalls_items`): item-level Recall@10 / Recall@50 and the median place, next to the
    row-level numbers of `compute_200k_val_metrics`, which stay what the reference prints."""
    predicted, target_names = test_200k.generate_200k_val_predictions(clip_model, relative_val_dataset, model, index_names, index_features,
                                                                      device, feature_dim, batch_size, num_workers, clip_model_name)
    index_fused = _common.fuse_index(model, index_features, index_local_features, prepared=True)
    return _common.recalls_items(model, predicted, index_fused, index_names, target_names, ks)


def ranking_dump(kind, relative_val_dataset, clip_model, index_features, index_local_features, index_names, model, device, feature_dim,
                 batch_size, num_workers, clip_model_name, depth: int) -> np.ndarray:
    """--dump-ranking: the first `depth` gallery rows of every query's full ranking, int32 [Q, depth] with -1 past the end
    (`_common.ranking_to_depth`) -- the reference's sorted_index_names (test_fiq.py:49-51) as row numbers, to any depth.  CIRR's
    rankings are without the query's reference image (test_cirr.py:55-62)."""
    out = _common.generate_predictions(kind, clip_model, relative_val_dataset, model, index_names, index_features, device, feature_dim,
                                       batch_size, num_workers, clip_model_name)
    index_fused = _common.fuse_index(model, index_features, index_local_features, prepared=True)
    ex = _common._unique_rows(index_names, out["references"], "reference").astype(np.int32) if kind == "cirr" else None
    return _common.ranking_to_depth(_common._engine_of(model), out["predicted"], index_fused, depth, exclude_idx=ex)
