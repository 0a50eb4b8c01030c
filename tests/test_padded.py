"""Padded trajectories on the host side: the variable-N reader (`nl_backend="matscipy"`), the case builder's acceptance of the
backend name, the synthetic padded datasets and their H5 writer.  (The engine side is tests/test_padded_gpu.py.)"""
import numpy as np
import pytest

from lagrangebench_amd.utils import NodeType, get_kinematic_mask


def _padded(name="waterdrop2d", counts=(300, 190), **kw):
    from lagrangebench_amd.data import make_padded_case
    return make_padded_case(name, counts, extra_seq_length=4, **kw)


@pytest.mark.parametrize("name,counts,n_max", [("waterdrop2d", (300, 190), None), ("small3d", (512, 300), 640)])
def test_variable_n_h5_reader_pads_to_num_particles_max(tmp_path, name, counts, n_max):
    """A dataset whose trajectories have different particle counts, written with per-trajectory shapes, read back with
    nl_backend="matscipy": every sample has num_particles_max rows, the real rows are what was written, the pad rows are
    position 0 / particle type -1 - for the training windows and for the evaluation trajectories."""
    from lagrangebench_amd.data import H5Dataset, h5, write_padded_h5
    ds = _padded(name, counts, n_max=n_max)
    N = int(ds.metadata["num_particles_max"])
    assert N == (n_max or max(counts)) and min(counts) <= 0.7 * N      # one trajectory with >= 30 % pads
    root = write_padded_h5(ds, str(tmp_path / "ds"))
    with h5.open_file(str(tmp_path / "ds" / "valid.h5")) as f:          # per-trajectory shapes on disk: no pads stored
        for i, n in enumerate(counts):
            assert tuple(f[f"{i:05d}/position"].shape) == (10, n, len(ds.box))
            assert tuple(f[f"{i:05d}/particle_type"].shape) == (n,)
    valid = H5Dataset("valid", root, name=name, input_seq_length=6, extra_seq_length=4, nl_backend="matscipy")
    assert valid.metadata["num_particles_max"] == N and len(valid) == len(counts)
    for i, n in enumerate(counts):
        pos, pt = valid[i]
        want_pos, want_pt = ds[i]
        assert pos.shape == (N, 10, len(ds.box)) and pt.shape == (N,)
        assert np.array_equal(pos[:n], want_pos[:n]) and np.array_equal(pt[:n], want_pt[:n]) and (pt[:n] != -1).all()
        assert (pos[n:] == 0).all() and (pt[n:] == NodeType.PAD_VALUE).all()
        assert np.array_equal(get_kinematic_mask(pt)[n:], np.ones(N - n, bool))
    train = H5Dataset("train", root, name=name, input_seq_length=6, extra_seq_length=1, nl_backend="matscipy")
    assert train.subseq_length == 8 and len(train) == 3 * len(counts)
    for idx in (0, 2, 3, len(train) - 1):
        i, t0 = divmod(idx, 3)
        pos, pt = train[idx]
        n = counts[i]
        assert pos.shape == (N, 8, len(ds.box)) and np.array_equal(pos[:n], ds[i][0][:n, t0:t0 + 8])
        assert (pos[n:] == 0).all() and (pt[n:] == -1).all() and np.array_equal(pt[:n], ds[i][1][:n])
    # every other backend name keeps reading the stored shapes
    plain = H5Dataset("valid", root, name=name, input_seq_length=6, extra_seq_length=4)
    assert plain[1][0].shape[0] == counts[1]


def test_case_builder_accepts_matscipy_backend_and_pads_are_kinematic():
    from lagrangebench_amd.case_setup import case_builder
    ds = _padded()
    case = case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"backend": "matscipy", "multiplier": 1.25},
                        cfg_model={"isotropic_norm": False, "magnitude_features": False}, noise_std=3e-4)
    assert case.N == 300 and not case.periodic and case.cfg_neighbors["backend"] == "matscipy"
    _, pt = ds[1]
    kin = get_kinematic_mask(pt)
    assert kin[190:].all() and not kin[:190].any()
    with pytest.raises(NotImplementedError):
        case_builder(ds.box, ds.metadata, ds.input_seq_length, cfg_neighbors={"backend": "no_such_backend"})


def test_padded_synthetic_cases_and_make_case_unchanged():
    """The padded entry point: given counts, trailing pads, num_particles_max in the metadata, a walled non-periodic 2D
    case with bounds inside the box and a periodic one; make_case itself is untouched (a padded case built from it holds
    exactly its rows)."""
    from lagrangebench_amd.data import make_case, make_padded_case
    wd = _padded()
    assert wd.metadata["periodic_boundary_conditions"] == [False, False] and wd.metadata["bounds"] == [[0.1, 0.9], [0.1, 0.9]]
    assert wd.n_real == [300, 190] and wd.metadata["num_particles_max"] == 300
    for i, n in enumerate(wd.n_real):
        pos, pt = wd[i]
        assert pos.shape == (300, 10, 2) and pos.dtype == np.float32 and pt.dtype == np.int32
        assert (pt[:n] == 0).all() and (pt[n:] == -1).all() and (pos[n:] == 0).all()
        assert pos[:n].min() > 0.1 and pos[:n].max() < 0.9
        assert np.abs(np.diff(pos[:n], axis=1)).max() > 0          # it moves
    base = make_case("small2d", n_trajs=2, extra_seq_length=4)
    ref = [(base[i][0].copy(), base[i][1].copy()) for i in range(2)]
    per = make_padded_case("small2d", (256, 100), n_max=300, extra_seq_length=4)
    assert per.metadata["periodic_boundary_conditions"] == [True, True] and per.metadata["num_particles_max"] == 300
    assert base.metadata["num_particles_max"] == 256                # the base case's metadata is not shared
    pos, pt = per[0]
    assert np.array_equal(pos[:256], ref[0][0]) and np.array_equal(pt[:256], ref[0][1]) and (pt[256:] == -1).all()
    pos1, pt1 = per[1]
    rows = {r.tobytes() for r in ref[1][0]}
    assert all(r.tobytes() in rows for r in pos1[:100]) and (pt1[100:] == -1).all() and (pos1[100:] == 0).all()
    again = make_case("small2d", n_trajs=2, extra_seq_length=4)
    assert all(np.array_equal(again[i][0], ref[i][0]) and np.array_equal(again[i][1], ref[i][1]) for i in range(2))


def test_models_other_than_gns_refuse_padded_input():
    """SEGNN, EGNN and PaiNN have not been taken through padded input: they must say so, by name, before any of their
    kernels runs (the check is on the host: no device needed)."""
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.models.base import BaseModel

    class Eng:
        has_pads = True

    class Other(BaseModel):
        def init(self, key, sample):
            return {}, {}
    with pytest.raises(NotImplementedError, match="padded trajectories"):
        Other()._check_padded(Eng())
    GNS(2, 128, 2, 2, 16)._check_padded(Eng())
    Eng.has_pads = False
    Other()._check_padded(Eng())
    from lagrangebench_amd import models
    for cls in (models.SEGNN, models.EGNN, models.PaiNN):
        assert cls._PADDED_OK is False
