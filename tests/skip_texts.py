"""Texts shared by the skip-table tests (test_skip_table.py, test_skip_search.py)."""
from functools import lru_cache

import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)


@lru_cache(maxsize=None)
def texts() -> dict:
    rng = np.random.default_rng(808)
    aligned = ACGT[rng.integers(0, 4, size=4_095)]          # n + 1 = 4096: a multiple of d and 2d at d = 64
    plain = ACGT[rng.integers(0, 4, size=5_000)]
    atail = ACGT[rng.integers(0, 4, size=5_000)]
    atail[-40:] = ord("A")                                   # AltCounters intervals drift past n + 1 here
    dup = ACGT[rng.integers(0, 4, size=5_000)]
    dup[3_100:3_400] = dup[700:1_000]                        # two-row intervals persist, narrowing late
    return {"aligned": aligned, "plain": plain, "atail": atail, "dup": dup}
