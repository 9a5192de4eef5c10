"""The CPU oracle of filtered ranking: tests/rank_oracle.py under the name its first users import.  TEST INFRASTRUCTURE.

``filtered_oracle()`` returns ``RankOracle``, whose ranking methods accept ``row_filter=`` (``fashionern_aaai2024_amd.engine.RowFilter``):
a filtered ranking is the unfiltered one of ``oracle.rank.cosine_topk`` with the ineligible rows' scores set to -inf, so the tie rule
(score descending, index ascending) and the (-inf, -1) padding are the oracle's own.
"""
from rank_oracle import RankOracle, eligible      # noqa: F401


def filtered_oracle():
    return RankOracle
