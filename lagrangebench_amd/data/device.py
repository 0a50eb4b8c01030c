"""DeviceDataset: the train split held in device memory, every trajectory uploaded once.

The host route reads each sample's window from the H5 file per step (``H5Dataset.get_window``, data/data.py:227-257);
overlapping windows of a trajectory share all but one frame, so the windows of a split are ``subseq_length`` times its
trajectories.  Here the trajectories themselves live in HBM - ``pos (n_traj, sequence_length, N, dim)`` in the file's dtype
(the order of the H5 ``position`` arrays) and ``ptype (n_traj, N)`` int32 - and a sample is a pair ``(trajectory, t0)`` that
``lb_train_batch`` (csrc/lb_train_input.hip) gathers, noises and turns into targets in one launch.  The index mapping is
``get_window``'s.  Padded data (``nl_backend="matscipy"``) is stored padded to ``num_particles_max`` with trailing rows
at position 0 and type -1, as ``H5Dataset`` yields it; which trajectories hold pads is known on the host.

Sources: an ``H5Dataset`` of the train split, or an in-memory dataset whose items are whole trajectories
``(pos (N, T, dim), particle_type (N,))`` with ``subseq_length == T`` (``SyntheticDataset``: sample i is trajectory i from
frame 0).  Validation and test data keep their loaders.
"""
from __future__ import annotations

import bisect
from typing import List, Sequence, Tuple

import numpy as np
import torch

PAD_VALUE = -1  # utils.NodeType.PAD_VALUE


def trajectory_source(dataset) -> str:
    """"h5" for an H5Dataset of the train split, "items" for an in-memory dataset of whole trajectories; TypeError for
    anything else (a list of samples, a validation split, ...)."""
    if all(hasattr(dataset, a) for a in ("traj_keys", "_open", "sequence_length", "subseq_length", "_keylen_cumulative")):
        return "h5"
    if hasattr(dataset, "traj_keys"):
        raise TypeError("DeviceDataset holds the TRAIN split (an H5Dataset with split='train'); validation and test data "
                        "keep their loader")
    if all(hasattr(dataset, a) for a in ("metadata", "subseq_length", "num_samples", "__getitem__")) and not isinstance(
            dataset, (list, tuple, dict)):
        return "items"
    raise TypeError(f"device_data needs an H5Dataset-like object that exposes its trajectories, got {type(dataset).__name__}")


class WindowIndex:
    """idx -> (trajectory, t0) of H5Dataset.get_window (data.py:227-257): every trajectory has
    ``sequence_length - subseq_length + 1`` windows, numbered trajectory by trajectory."""

    def __init__(self, n_traj: int, sequence_length: int, subseq_length: int):
        if sequence_length < subseq_length:
            raise ValueError(f"trajectories of {sequence_length} frames are shorter than a sample ({subseq_length})")
        self.n_traj, self.sequence_length, self.subseq_length = int(n_traj), int(sequence_length), int(subseq_length)
        per_traj = self.sequence_length - self.subseq_length + 1
        self._cumulative = np.cumsum([per_traj] * self.n_traj).tolist()
        self.num_samples = int(per_traj * self.n_traj)

    def __len__(self) -> int:
        return self.num_samples

    def locate(self, idx: int) -> Tuple[int, int]:
        idx = int(idx)
        if not 0 <= idx < self.num_samples:
            raise IndexError(idx)
        traj = bisect.bisect(self._cumulative, idx)
        return traj, idx if traj == 0 else idx - self._cumulative[traj - 1]


class DeviceDataset:
    def __init__(self, dataset, device=None, max_bytes=None):
        kind = trajectory_source(dataset)
        self.dataset = dataset
        self.metadata = dataset.metadata
        self.N = int(self.metadata["num_particles_max"])
        self.subseq_length = int(dataset.subseq_length)
        padded = getattr(dataset, "nl_backend", None) == "matscipy"
        if kind == "h5":
            db = dataset._open()
            keys = list(dataset.traj_keys)
            seq_len = int(dataset.sequence_length)
            read = lambda k: (np.asarray(db[f"{keys[k]}/position"][:]), np.asarray(db[f"{keys[k]}/particle_type"][:]))
            shape0 = db[f"{keys[0]}/position"].shape
            n_traj, dim, dtype = len(keys), int(shape0[2]), np.dtype(db[f"{keys[0]}/position"].dtype)
        else:
            n_traj = int(dataset.num_samples)
            pos0 = np.asarray(dataset[0][0])
            seq_len, dim, dtype = int(pos0.shape[1]), int(pos0.shape[2]), pos0.dtype
            padded = True  # items come padded already (make_padded_case) or full: both are N rows
            read = lambda k: (np.asarray(dataset[k][0]).transpose(1, 0, 2), np.asarray(dataset[k][1]))
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"positions of dtype {dtype} (float32 and float64 are built)")
        self.index = WindowIndex(n_traj, seq_len, self.subseq_length)
        if kind == "h5" and self.index._cumulative != list(dataset._keylen_cumulative):
            raise ValueError("the dataset's window numbering is not sequence_length - subseq_length + 1 per trajectory")
        self.n_traj, self.sequence_length, self.dim, self.num_samples = n_traj, seq_len, dim, self.index.num_samples
        self.pos_f64 = dtype == np.dtype(np.float64)

        # device = "cpu" keeps the buffers on the host: the layout and the mapping without a device (tests)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.nbytes = n_traj * seq_len * self.N * dim * dtype.itemsize + n_traj * self.N * 4
        if max_bytes is None and self.device.type == "cuda":
            max_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        if max_bytes is not None and self.nbytes > int(max_bytes):
            raise ValueError(f"DeviceDataset: the split needs {self.nbytes} bytes on the device, max_bytes is {int(max_bytes)}")
        tdtype = torch.float64 if self.pos_f64 else torch.float32
        self.pos = torch.empty((n_traj, seq_len, self.N, dim), dtype=tdtype, device=self.device)
        self.ptype_host = np.full((n_traj, self.N), PAD_VALUE, dtype=np.int32)
        for k in range(n_traj):   # one trajectory at a time: the host never holds the split
            pos, pt = read(k)
            n = pos.shape[1]
            if pos.shape[0] != seq_len or pos.shape[2] != dim or pt.shape[0] != n:
                raise ValueError(f"trajectory {k}: positions {pos.shape}, particle types {pt.shape}; expected ({seq_len}, n, {dim})")
            if n > self.N or (n < self.N and not padded):
                raise ValueError(f"trajectory {k} has {n} particles, metadata['num_particles_max'] is {self.N}"
                                 + ("" if n > self.N else " (variable particle counts need nl_backend='matscipy')"))
            buf = np.zeros((seq_len, self.N, dim), dtype=dtype)   # H5Dataset._matscipy_pad: trailing rows at 0, type -1
            buf[:, :n] = pos
            self.ptype_host[k, :n] = pt
            self.pos[k].copy_(torch.from_numpy(buf))
        self.ptype = torch.from_numpy(self.ptype_host).to(self.device)
        self.traj_has_pads = (self.ptype_host == PAD_VALUE).any(axis=1)

    def __len__(self) -> int:
        return self.num_samples

    def locate(self, idx: int) -> Tuple[int, int]:
        return self.index.locate(idx)

    def locate_batch(self, indices: Sequence[int]) -> Tuple[List[int], List[int]]:
        pairs = [self.index.locate(i) for i in indices]
        return [p[0] for p in pairs], [p[1] for p in pairs]

    def has_pads(self, trajs: Sequence[int]) -> bool:
        """Do these trajectories hold pad particles?  From the host copy of the types: no device read-back."""
        return bool(self.traj_has_pads[list(trajs)].any())

    def particle_types(self, indices: Sequence[int]) -> np.ndarray:
        """(len(indices), N) int32 particle types of the samples (host)."""
        return self.ptype_host[self.locate_batch(indices)[0]]

    def window(self, idx: int):
        """Sample idx as the host route yields it: (pos (N, subseq_length, dim), particle_type (N,)) numpy arrays."""
        traj, t0 = self.locate(idx)
        pos = self.pos[traj, t0:t0 + self.subseq_length].cpu().numpy().transpose(1, 0, 2)
        return pos, self.ptype_host[traj].copy()
