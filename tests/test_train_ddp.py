"""Data-parallel training, the parts that need no GPU: the batch split over the ranks, the Trainer's refusal of a batch
that does not divide, and the agreement of header, ctypes table and INTEGRATION.md on the two entry points of the
rank-ordered gradient sum (lb_gns_train_device_blob, lb_adamw_step_gathered).  The device side is tests/test_train_ddp_gpu.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lb_gns_train_device_blob", "lb_adamw_step_gathered")


@pytest.mark.parametrize("batch,world", [(1, 1), (2, 2), (8, 2), (12, 4), (16, 16), (6, 3)])
def test_shard_batch_slices_are_disjoint_ordered_and_cover_the_batch(batch, world):
    from lagrangebench_amd.dist import shard_batch
    slices = [shard_batch(batch, r, world) for r in range(world)]
    assert all(isinstance(s, slice) and s.step in (None, 1) for s in slices)
    assert slices[0].start == 0 and slices[-1].stop == batch
    for a, b in zip(slices, slices[1:]):
        assert a.stop == b.start                                  # ordered, disjoint, no gap
    assert len({s.stop - s.start for s in slices}) == 1           # equal shards
    items = list(range(batch))
    assert sum((items[s] for s in slices), []) == items


def test_shard_batch_refuses_an_indivisible_batch():
    from lagrangebench_amd.dist import shard_batch
    with pytest.raises(ValueError, match="batch_size"):
        shard_batch(3, 0, 2)
    with pytest.raises(ValueError, match="batch_size"):
        shard_batch(3, 1, 2)
    with pytest.raises(ValueError):
        shard_batch(4, 2, 2)                                      # no such rank


def test_trainer_refuses_an_indivisible_batch_before_touching_anything(monkeypatch):
    """WORLD_SIZE=2 in the environment (torchrun's), batch_size 3: the Trainer raises in __init__ - case and datasets
    are None here, as in the refusal tests of the models, so nothing else can have been touched first."""
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.train import Trainer
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(ValueError, match="batch_size"):
        Trainer(GNS(3, 128, 2, 2, 16), None, None, None, cfg_train={"batch_size": 3})
    # a model that cannot train at all is still refused for that reason first
    with pytest.raises(NotImplementedError, match="latent_size <= 128"):
        Trainer(GNS(3, 256, 2, 2, 16), None, None, None, cfg_train={"batch_size": 3})


def test_all_gather_rows_is_a_view_on_one_rank():
    import torch
    from lagrangebench_amd.dist import all_gather_rows, gather_scalars
    t = torch.arange(7, dtype=torch.float32)
    rows = all_gather_rows(t)
    assert rows.shape == (1, 7) and rows.data_ptr() == t.data_ptr()
    assert gather_scalars(0.25) == [0.25]
    with pytest.raises(ValueError):
        all_gather_rows(torch.zeros((2, 3)))


def test_header_ctypes_table_and_integration_notes_name_the_new_entry_points():
    from lagrangebench_amd import _lib
    header = open(os.path.join(ROOT, "include", "lbhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"include/lbhip.h does not declare {name}"
        assert name in _lib._SIGS, f"_lib._SIGS does not bind {name}"
        assert name in notes, f"INTEGRATION.md does not mention {name}"
    # the signatures the header states: (t, which, float**, int64_t*) and (t, rows, world, grad_scale, lr, b1, b2, eps, wd)
    assert len(_lib._SIGS["lb_gns_train_device_blob"][1]) == 4
    assert len(_lib._SIGS["lb_adamw_step_gathered"][1]) == 9


def test_the_library_exports_the_new_entry_points():
    from lagrangebench_amd import build
    build.build()
    from lagrangebench_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    # argument validation that does not touch the device
    assert lib.lb_gns_train_device_blob(None, 1, None, None) == -1
    assert lib.lb_adamw_step_gathered(None, None, 1, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0) == -1
