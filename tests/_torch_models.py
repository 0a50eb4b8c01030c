"""A small message-passing network in plain torch for the TorchModel tests, and the graph ops restated on the CPU.

`TinyMP` is what a user would write against ``models.TorchModel``: ``forward(features, particle_type, graph)``.  The same
class runs on the device with ``lagrangebench_amd.graph.Graph`` (HIP gather / ordered segment sum) and on the CPU with
`CpuGraph` (``index_select`` / ``index_add_``, any dtype) on the features the engine exported - the float64 and float32
restatements the device results are compared with.
"""
import numpy as np
import torch
from torch import nn

NODE_KEYS = ("vel_hist", "vel_mag", "bound", "force")


class TinyMP(nn.Module):
    """Linear encoder -> one edge MLP on [x_s, x_r, rel_disp, rel_dist] -> a receiver sum AND a sender sum of the messages
    (both roles are in the gradient) -> node MLP -> Linear decoder; SiLU throughout (no ReLU kinks).  node_in counts the
    engine's node feature columns plus one: the particle type as a value.  `gain` is a parameter of the module itself (tree
    module "~"), `in_scale` a persistent buffer (the state tree)."""

    def __init__(self, node_in: int, dim: int, hidden: int = 32):
        super().__init__()
        self.enc = nn.Linear(node_in, hidden)
        self.edge = nn.Sequential(nn.Linear(2 * hidden + dim + 1, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.node = nn.Sequential(nn.Linear(3 * hidden, hidden), nn.SiLU(), nn.Linear(hidden, hidden))
        self.dec = nn.Linear(hidden, dim)
        self.gain = nn.Parameter(torch.ones(hidden))
        self.register_buffer("in_scale", torch.ones(node_in))

    def reset_parameters(self):
        with torch.no_grad():
            self.gain.fill_(1.0)

    def forward(self, features, particle_type, graph):
        dt = self.gain.dtype
        x = torch.cat([features[k].to(dt) for k in NODE_KEYS if k in features] + [particle_type[..., None].to(dt)], -1)
        h = nn.functional.silu(self.enc(x * self.in_scale))
        hs, hr = graph.gather(h, "senders"), graph.gather(h, "receivers")
        m = nn.functional.silu(self.edge(torch.cat([hs, hr, features["rel_disp"].to(dt), features["rel_dist"].to(dt)], -1)))
        agg = torch.cat([h, graph.segment_sum(m, "receivers"), graph.segment_sum(m, "senders")], -1)
        return self.dec(h + self.gain * self.node(agg))


class CpuGraph:
    """``graph.Graph``'s gather / segment_sum with CPU ``index_select`` / ``index_add_`` on an exported list: `senders`,
    `receivers` (B, E_cap) with pad slots holding N, `n_edges` (B,).  Any float dtype; always batched."""

    def __init__(self, senders, receivers, n_edges, n_nodes: int):
        self.idx = {"senders": torch.as_tensor(np.asarray(senders)).long(), "receivers": torch.as_tensor(np.asarray(receivers)).long()}
        self.n_edges = torch.as_tensor(np.asarray(n_edges)).long().reshape(-1)
        self.N = int(n_nodes)
        self.B, self.E = self.idx["senders"].shape
        self.real = torch.arange(self.E)[None, :] < self.n_edges[:, None]          # (B, E_cap)
        off = (torch.arange(self.B) * self.N)[:, None]
        # flat node number of every slot; the pad slots point at one spare row behind the batch
        self.flat = {k: torch.where(self.real, v.clamp(max=self.N - 1) + off, torch.full_like(v, self.B * self.N)).reshape(-1)
                     for k, v in self.idx.items()}

    def gather(self, x, role):
        C = x.shape[-1]
        rows = torch.cat([x.reshape(self.B * self.N, C), x.new_zeros((1, C))])
        return rows.index_select(0, self.flat[role]).reshape(self.B, self.E, C)

    def segment_sum(self, msg, role):
        C = msg.shape[-1]
        m = torch.where(self.real[..., None], msg, torch.zeros((), dtype=msg.dtype)).reshape(self.B * self.E, C)
        out = msg.new_zeros((self.B * self.N + 1, C)).index_add(0, self.flat[role], m)
        return out[:-1].reshape(self.B, self.N, C)


def cpu_features(features, dtype):
    """A FeatureDict's tensors on the CPU as `dtype` (indices as int64), batched."""
    out = {}
    for k in features.keys():
        v = features[k].detach().cpu()
        v = v if features.batched else v[None]
        out[k] = v.long() if k in ("senders", "receivers") else v.to(dtype)
    return out


def node_in_of(engine) -> int:
    return engine.node_in + 1


def mse_loss(pred, target, particle_type, weight=1.0):
    """The reference's _mse per trajectory (trainer.py:35-60): (sum over the batch - what is differentiated -, mean)."""
    pt = torch.as_tensor(np.asarray(particle_type))
    mask = ~((pt == 1) | (pt == 2) | (pt == -1))
    per = torch.where(mask, ((pred - target) ** 2).sum(-1), torch.zeros((), dtype=pred.dtype))
    per_traj = weight * per.sum(1) / mask.sum(1)
    return per_traj.sum(), per_traj.mean()


def adamw_replay_step(w, g, m, v, count, lr, b1=0.9, b2=0.999, eps=1e-8, wd=1e-8):
    """One optax.adamw step in the dtype of its arguments (scale_by_adam, add_decayed_weights, scale by -lr; trainer.py:183-193):
    returns (w, m, v) after step `count` (1-based, the exponent of the bias correction)."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mh, vh = m / (1 - b1 ** count), v / (1 - b2 ** count)
    return w - lr * (mh / (np.sqrt(vh) + eps) + wd * w), m, v
