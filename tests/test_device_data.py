"""Device-resident training input, the parts that need no device: the random numbers lb_train_batch draws (Philox4x32-10
and Box-Muller, restated here in numpy and checked against the Random123 known answers and against the normal
distribution), DeviceDataset's window numbering and layout against H5Dataset.get_window, the new default, the C ABI and
the Trainer's refusal."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ = os.path.join(ROOT, "tests", "golden", "3D_LJ_3_1214every1")

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  ctr (..., 4),
    key (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(key)[..., i].astype(np.uint64) for i in range(2))
    mask = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r > 0:
            k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def box_muller4(x):
    """(..., 4) uint32 -> (..., 4) N(0, 1): u = (x + 0.5) * 2^-32; (r01 cos t01, r01 sin t01, r23 cos t23, r23 sin t23) with
    r_ab = sqrt(-2 log u_a), t_ab = 2 pi u_b, in fp64."""
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    out = np.empty(u.shape, np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        t = 6.283185307179586 * u[..., a + 1]
        out[..., a], out[..., a + 1] = r * np.cos(t), r * np.sin(t)
    return out


def normals_for(seed, step, slot, n_particles, n_vel, dim):
    """The draws of lb_train_batch for one sample: (n_particles, n_vel, dim); draw q = k * dim + d of a particle is value
    q % 4 of the counter (step, slot, particle, q // 4) under the key (seed lo, seed hi)."""
    n_ctr = (n_vel * dim + 3) // 4
    ctr = np.zeros((n_particles, n_ctr, 4), np.uint32)
    ctr[..., 0], ctr[..., 1] = np.uint32(step), np.uint32(slot)
    ctr[..., 2] = np.arange(n_particles, dtype=np.uint32)[:, None]
    ctr[..., 3] = np.arange(n_ctr, dtype=np.uint32)[None, :]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    z = box_muller4(philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,))))
    return z.reshape(n_particles, n_ctr * 4)[:, :n_vel * dim].reshape(n_particles, n_vel, dim)


def _words(s):
    return np.array([int(w, 16) for w in s.split()], np.uint32)


@pytest.mark.parametrize("ctr, key, want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(_words(ctr), _words(key))
    assert [f"{int(v):08x}" for v in got] == want.split()


def test_draw_statistics():
    """10^6 draws: the mean's sigma is 1e-3, the std's 7e-4, the 3-sigma tail count's 1.9 % of itself - the bounds are about
    five of each."""
    z = normals_for(seed=0x1234567887654321, step=7, slot=3, n_particles=50_000, n_vel=5, dim=4).ravel()
    assert z.size == 10**6 and np.isfinite(z).all()
    mean, std, tail = z.mean(), z.std(), (np.abs(z) > 3.0).mean()
    print(f"[device data] 1e6 draws: mean {mean:.3e}, std - 1 {std - 1:.3e}, beyond 3 sigma {tail:.4e}")
    assert abs(mean) < 5e-3 and abs(std - 1.0) < 5e-3
    assert abs(tail - 2.70e-3) < 0.2 * 2.70e-3
    # counters differ by particle, slot, step and seed
    base = normals_for(5, 1, 0, 4, 5, 3)
    assert not np.array_equal(base[0], base[1])
    for other in (normals_for(5, 1, 1, 4, 5, 3), normals_for(5, 2, 0, 4, 5, 3), normals_for(6, 1, 0, 4, 5, 3),
                  normals_for(5 + (1 << 32), 1, 0, 4, 5, 3)):
        assert not np.array_equal(base, other)


def test_index_mapping_lj():
    """DeviceDataset (buffers kept on the host) numbers and gathers the windows of the LJ fixture as get_window does."""
    from lagrangebench_amd.data import DeviceDataset, H5Dataset
    ds = H5Dataset("train", LJ, name="lj3d", input_seq_length=6, extra_seq_length=2)
    dd = DeviceDataset(ds, device="cpu")
    assert len(dd) == len(ds) and dd.subseq_length == ds.subseq_length == 9
    assert dd.n_traj == len(ds.traj_keys) and dd.sequence_length == ds.sequence_length
    assert tuple(dd.pos.shape) == (dd.n_traj, ds.sequence_length, dd.N, 3) and str(dd.pos.dtype) == "torch.float32"
    assert not dd.has_pads(range(dd.n_traj))
    per = ds.sequence_length - ds.subseq_length + 1
    picks = sorted(i for i in {0, 1, per - 1, per, len(ds) - 1, len(ds) // 2} if i < len(ds))
    for idx in picks:
        assert dd.locate(idx) == (idx // per, idx % per)
        pos, pt = ds.get_window(idx)
        dpos, dpt = dd.window(idx)
        assert dpos.dtype == pos.dtype and np.array_equal(dpos, pos) and np.array_equal(dpt, pt)
    assert np.array_equal(dd.particle_types(picks[:3]), np.stack([ds[i][1] for i in picks[:3]]))
    with pytest.raises(IndexError):
        dd.locate(len(ds))
    with pytest.raises(ValueError, match=rf"{dd.nbytes} bytes.*1000"):
        DeviceDataset(ds, device="cpu", max_bytes=1000)
    with pytest.raises(TypeError):
        DeviceDataset(H5Dataset("valid", LJ, name="lj3d", input_seq_length=6, extra_seq_length=10), device="cpu")


def test_index_mapping_padded(tmp_path):
    """make_padded_case: in memory (sample i = trajectory i) and written as a variable-N H5 directory read with
    nl_backend="matscipy" (several windows per trajectory): pads at position 0 with type -1, as H5Dataset yields them."""
    from lagrangebench_amd.data import DeviceDataset, H5Dataset, make_padded_case, write_padded_h5
    ds = make_padded_case("small2d", [200, 256, 131], extra_seq_length=4)
    dd = DeviceDataset(ds, device="cpu")
    assert len(dd) == 3 and dd.subseq_length == 10 and dd.N == 256
    assert list(dd.traj_has_pads) == [True, False, True] and dd.has_pads([0, 1]) and not dd.has_pads([1])
    for i in range(3):
        assert dd.locate(i) == (i, 0)
        pos, pt = ds[i]
        dpos, dpt = dd.window(i)
        assert np.array_equal(dpos, pos) and np.array_equal(dpt, pt)
        assert (dpt[ds.n_real[i]:] == -1).all() and (dpos[ds.n_real[i]:] == 0).all()
    path = write_padded_h5(ds, str(tmp_path / "2D_PAD_256_10"))
    h5 = H5Dataset("train", path, name="pad2d", input_seq_length=6, extra_seq_length=1, nl_backend="matscipy")
    dh = DeviceDataset(h5, device="cpu")
    per = 10 - 8 + 1
    assert len(dh) == len(h5) == 3 * per and dh.subseq_length == 8
    for idx in range(len(h5)):
        assert dh.locate(idx) == (idx // per, idx % per)
        pos, pt = h5.get_window(idx)
        dpos, dpt = dh.window(idx)
        assert np.array_equal(dpos, pos) and np.array_equal(dpt, pt)
    assert list(dh.traj_has_pads) == [True, False, True]
    # without the padding backend a short trajectory is an error, as it is on the host route's engine
    with pytest.raises(ValueError, match="matscipy"):
        DeviceDataset(H5Dataset("train", path, name="pad2d", input_seq_length=6, extra_seq_length=1), device="cpu")


def test_default_is_off():
    from lagrangebench_amd.defaults import defaults
    assert defaults.train.device_data is False


def test_abi_lists_the_entry_point():
    from lagrangebench_amd import _lib
    assert "lb_train_batch" in _lib._SIGS
    src = open(os.path.join(ROOT, "include", "lbhip.h")).read()
    assert re.search(r"\bint lb_train_batch\s*\(", src)
    assert "strats.py:12-83" in src and "case.py:142-178" in src
    m = re.search(r"#define LB_TRAIN_BATCH_MAX (\d+)", src)
    assert m and int(m.group(1)) == _lib.LB_TRAIN_BATCH_MAX
    from lagrangebench_amd import build
    assert "lb_train_input.hip" in build.SOURCES


def test_trainer_refuses_a_dataset_without_trajectories():
    from lagrangebench_amd.case_setup import case_builder
    from lagrangebench_amd.data import H5Dataset
    from lagrangebench_amd.models import GNS
    from lagrangebench_amd.train import Trainer
    md = json.load(open(os.path.join(LJ, "metadata.json")))
    bounds = np.array(md["bounds"])
    case = case_builder(bounds[:, 1] - bounds[:, 0], md, 6)
    train = H5Dataset("train", LJ, name="lj3d", input_seq_length=6, extra_seq_length=1)
    valid = H5Dataset("valid", LJ, name="lj3d", input_seq_length=6, extra_seq_length=10)
    samples = [train[0], train[1]]                       # a plain list of samples: no trajectories to upload
    kw = dict(cfg_eval={"n_rollout_steps": 10, "train": {"n_trajs": 1}}, input_seq_length=6)
    with pytest.raises(TypeError, match="trajectories"):
        Trainer(GNS(3, 64, 2, 1, 16), case, samples, valid, cfg_train={"device_data": True}, **kw)
    with pytest.raises(TypeError):
        Trainer(GNS(3, 64, 2, 1, 16), case, valid, valid, cfg_train={"device_data": True}, **kw)
    t = Trainer(GNS(3, 64, 2, 1, 16), case, train, valid, cfg_train={"device_data": True}, **kw)
    assert t.device_data and t.loader_train.indices_only
    idx, slots = next(iter(t.loader_train))
    assert len(idx) == 1 and slots == [0] and 0 <= idx[0] < len(train)
    assert not Trainer(GNS(3, 64, 2, 1, 16), case, train, valid, **kw).device_data
