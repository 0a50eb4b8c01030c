"""The one-directional-edge fixture (tests/_asym.py) proves its own premise on the CPU: the oracle's neighbor list of
the crafted window holds every promised pair in one direction only, in both geometry dtypes, 2D and 3D, in every
trajectory of the batch, with both index orders of sender and receiver and one particle with two such edges.  The GPU
tests of tests/test_asym_lists_gpu.py are worth something only if this holds."""
from collections import Counter

import numpy as np
import pytest

from tests._asym import asym_case, check_premise, oracle_edges


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["tgv2d", "tgv3d", "rpf2d"])
def test_fixture_lists_hold_one_directional_edges(name, dtype):
    ds, pos, pt, pairs = asym_case(name, dtype=dtype)
    B, isl = pos.shape[0], ds.input_seq_length
    assert B >= 2 and len(pairs) >= 3
    assert {b for b, _, _ in pairs} == set(range(B))                       # every trajectory, so the b*N offsets count
    assert any(s < r for _, r, s in pairs) and any(s > r for _, r, s in pairs)   # both index orders
    ends = Counter((b, i) for b, r, s in pairs for i in (r, s))
    assert max(ends.values()) >= 2                                         # a particle with two one-directional edges
    assert np.array_equal(pos, pos.astype(np.dtype(dtype)).astype(np.float64))
    for b in range(B):
        for end in (isl, isl + 1, pos.shape[2]):   # allocation window, the update's, the last one
            check_premise(oracle_edges(ds, pos[b], pt[b], end, dtype=dtype), pairs, b)
