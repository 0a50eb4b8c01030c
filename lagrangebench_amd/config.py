"""Configs and command-line overrides - mirror of the reference's main.py:6-41 and lagrangebench/defaults.py.

A reference user starts a run with ``python main.py config=configs/rpf_2d/gns.yaml train.step_max=...`` or
``load_ckp=...``; ``python -m lagrangebench_amd`` (``__main__.py``) takes the same arguments and the same YAML files.

* ``reference_defaults()``: the full tree of defaults.py:7-176 (``config``, ``load_ckp``, ``mode: all``, ``gpu``,
  ``xla_mem_fraction``, ``dataset``, ``eval.test`` ... included), plus this package's two keys ``train.device_data`` and
  ``train.device_unroll``.  (``defaults.py`` of this package keeps the subset the rollout path reads.)
* ``load_config(path, cli)``: main.py:17-41 - follows ``extends:`` up to ``LAGRANGEBENCH_DEFAULTS``; paths are used as
  given (relative to the working directory); later files override earlier ones, the command line overrides all.
* ``parse_cli(argv)``: ``OmegaConf.from_cli`` dot-lists, ``a.b.c=value``.
* ``check_cfg(cfg)``: the rules of defaults.py:182-204, with its assertion texts.
* ``to_yaml(cfg)`` / ``load(path)``: the merged config as text and back.

OmegaConf is not a dependency: configs are the plain attribute dicts of ``defaults.py``.  Values are YAML 1.2 scalars:
PyYAML (YAML 1.1) reads ``1.e-4`` as a float but ``1e-4`` as a string, so the loader here carries a float resolver that
takes both, as OmegaConf's does.
"""
from __future__ import annotations

import copy
import re
from typing import Any, List, Mapping, Optional, Sequence

from .defaults import _wrap, merge

DEFAULTS_NAME = "LAGRANGEBENCH_DEFAULTS"

_REFERENCE_DEFAULTS = {
    # global and hardware-related configs (defaults.py:10-27)
    "config": None, "load_ckp": None, "mode": "all", "seed": 0, "dtype": "float64", "gpu": None, "xla_mem_fraction": None,
    "dataset": {"src": None, "name": None},                                                     # defaults.py:30-35
    "model": {                                                                                  # defaults.py:38-63
        "name": None, "input_seq_length": 6, "num_mp_steps": 10, "num_mlp_layers": 2, "latent_dim": 128,
        "magnitude_features": False, "isotropic_norm": False,
        "lmax_attributes": 1, "lmax_hidden": 1, "segnn_norm": "none", "velocity_aggregate": "avg",
    },
    "train": {                                                                                  # defaults.py:66-107
        "batch_size": 1, "step_max": 500_000, "num_workers": 4, "noise_std": 3.0e-4,
        "optimizer": {"lr_start": 1.0e-4, "lr_final": 1.0e-6, "lr_decay_rate": 0.1, "lr_decay_steps": 1.0e5},
        "pushforward": {"steps": [-1, 20000, 300000, 400000], "unrolls": [0, 1, 2, 3], "probs": [18, 2, 1, 1]},
        "loss_weight": {"acc": 1.0, "vel": 0.0, "pos": 0.0},
        "device_data": False,     # not in the reference (lagrangebench_amd/defaults.py)
        "device_unroll": False,   # not in the reference
    },
    "eval": {                                                                                   # defaults.py:110-148
        "n_rollout_steps": 20, "test": False, "rollout_dir": None,
        "train": {"n_trajs": 50, "metrics_stride": 10, "batch_size": 1, "metrics": ["mse"], "out_type": "none"},
        "infer": {"n_trajs": -1, "metrics_stride": 1, "batch_size": 2, "metrics": ["mse", "e_kin", "sinkhorn"],
                  "out_type": "pkl", "n_extrap_steps": 0},
    },
    "logging": {"log_steps": 1000, "eval_steps": 10000, "wandb": False, "wandb_project": None,  # defaults.py:151-166
                "wandb_entity": "lagrangebench", "ckp_dir": "ckp", "run_name": None},
    "neighbors": {"backend": "jaxmd_vmap", "multiplier": 1.25},                                 # defaults.py:169-174
}
ADDED_KEYS = ("train.device_data", "train.device_unroll")   # what reference_defaults() holds beyond defaults.py


def reference_defaults():
    """A fresh copy of the reference's full default tree (defaults.py:7-176) plus ADDED_KEYS."""
    return _wrap(copy.deepcopy(_REFERENCE_DEFAULTS))


# ------------------------------------------------------------------------------------------------ YAML
# YAML 1.2 core-schema floats (what OmegaConf's loader resolves): a mantissa with or without a dot, an optional exponent
# with or without a sign; .inf / .nan
_FLOAT = re.compile(r"""^(?:[-+]?(?:[0-9][0-9_]*)\.[0-9_]*(?:[eE][-+]?[0-9]+)?
                         |[-+]?(?:[0-9][0-9_]*)(?:[eE][-+]?[0-9]+)
                         |\.[0-9_]+(?:[eE][-+]?[0-9]+)?
                         |[-+]?\.(?:inf|Inf|INF)
                         |\.(?:nan|NaN|NAN))$""", re.X)
_loader_cls = None


def _yaml():
    try:
        import yaml
    except ImportError as e:  # pragma: no cover
        raise ImportError("lagrangebench_amd.config reads and writes YAML: PyYAML is required") from e
    return yaml


def _resolvers(base):
    """PyYAML's implicit resolvers of `base` without its YAML 1.1 float rule, as a table of its own (the class attribute
    is shared and stays as it is)."""
    return {ch: [(tag, rx) for tag, rx in lst if tag != "tag:yaml.org,2002:float"]
            for ch, lst in base.yaml_implicit_resolvers.items()}


def _loader():
    global _loader_cls
    if _loader_cls is None:
        yaml = _yaml()

        class Loader(yaml.SafeLoader):
            pass

        Loader.yaml_implicit_resolvers = _resolvers(yaml.SafeLoader)
        Loader.add_implicit_resolver("tag:yaml.org,2002:float", _FLOAT, list("-+0123456789."))
        _loader_cls = Loader
    return _loader_cls


def _parse_yaml(text: str):
    return _yaml().load(text, Loader=_loader())


def parse_value(text: str):
    """One command-line value as a YAML scalar / flow collection: ``1e-4`` -> float, ``null`` -> None, ``true`` -> True,
    ``[0,1,2]`` -> list, anything else a string; an empty value is None (OmegaConf.from_cli)."""
    if text.strip() == "":
        return None
    try:
        return _parse_yaml(text)
    except Exception:   # not YAML (an unbalanced bracket, a path with a colon ...): the text itself
        return text


def load(path: str):
    """One YAML file as an attribute dict (an empty file: {})."""
    with open(path) as f:
        data = _parse_yaml(f.read())
    if data is None:
        data = {}
    if not isinstance(data, Mapping):
        raise ValueError(f"{path}: a config file must hold a mapping, found {type(data).__name__}")
    return _wrap(data)


def to_yaml(cfg) -> str:
    """The config as YAML text (OmegaConf.to_yaml: block style, keys in their order); ``load`` of it gives `cfg` back."""
    yaml = _yaml()

    class Dumper(yaml.SafeDumper):
        pass

    # the Loader's scalar rules decide which strings need quotes: "1e5" as a run name must come back a string
    Dumper.yaml_implicit_resolvers = _resolvers(yaml.SafeDumper)
    Dumper.add_implicit_resolver("tag:yaml.org,2002:float", _FLOAT, list("-+0123456789."))

    def _float(d, v):   # (PyYAML writes 1e-06 without a dot, which YAML 1.1 readers take for a string)
        node = d.represent_float(v)
        if "." not in node.value and ("e" in node.value or "E" in node.value):
            m, e = re.split("[eE]", node.value)
            node.value = f"{m}.0e{e}"
        return node

    Dumper.add_representer(float, _float)
    return yaml.dump(_plain(cfg), Dumper=Dumper, default_flow_style=False, sort_keys=False)


def _plain(x):
    if isinstance(x, Mapping):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if hasattr(x, "tolist") and not isinstance(x, (str, bytes)):   # a numpy scalar or array
        return _plain(x.tolist())
    if x is None or isinstance(x, (str, bool, int, float)):
        return x
    return str(x)   # (a path object, an enum ...: what a hand-written config dict may carry)


# ------------------------------------------------------------------------------------------------ command line
def parse_cli(argv: Sequence[str]):
    """``OmegaConf.from_cli``: every argument is ``a.b.c=value``; later arguments override earlier ones."""
    out: dict = {}
    for arg in argv:
        key, sep, val = arg.partition("=")
        if not key:
            raise ValueError(f"command-line argument {arg!r}: expected key=value")
        node = out
        parts = key.split(".")
        for p in parts[:-1]:
            if not isinstance(node.get(p), dict):
                node[p] = {}
            node = node[p]
        node[parts[-1]] = parse_value(val) if sep else None
    return _wrap(out)


def _leaf_keys(tree, prefix=""):
    """("a.b.c", parent mapping path exists) for every leaf of a nested mapping, depth first in its order."""
    for k, v in tree.items():
        if isinstance(v, Mapping):
            yield from _leaf_keys(v, f"{prefix}{k}.")
        else:
            yield f"{prefix}{k}"


def check_subset(superset, subset) -> None:
    """The rule of main.py:6-14: every key the command line sets must be a key of the defaults.  AssertionError with the
    reference's text, naming the first dotted key that is not."""
    for dotted in _leaf_keys(subset):
        node = superset
        for part in dotted.split("."):
            if not isinstance(node, Mapping) or part not in node:
                raise AssertionError(f"cli_args must be a subset of the defaults. Wrong cli key: '{dotted}'")
            node = node[part]


def load_config(path: str, cli: Optional[Mapping] = None):
    """main.py:17-41 (load_embedded_configs): the file at `path`, under it every config it ``extends`` - up to the
    defaults when the chain ends in ``LAGRANGEBENCH_DEFAULTS`` - and `cli` on top."""
    cli = _wrap(cli or {})
    cfgs: List[Any] = [load(path)]
    while "extends" in cfgs[0]:
        extends_path = cfgs[0].pop("extends")
        if extends_path != DEFAULTS_NAME:
            cfgs.insert(0, load(extends_path))
        else:
            cfgs.insert(0, reference_defaults())
            check_subset(cfgs[0], cli)
            break
    cfg = cfgs[0]
    for c in cfgs[1:] + [cli]:
        cfg = merge(cfg, c)
    return cfg


def cli_config(argv: Sequence[str]):
    """main.py:44-69: the command line of a run -> its merged config.  Exactly one of ``config`` / ``load_ckp``."""
    import os
    cli = parse_cli(argv)
    assert ("config" in cli) != ("load_ckp" in cli), "You must specify one of 'config' or 'load_ckp'."
    path = cli.config if "config" in cli else os.path.join(str(cli.load_ckp), "config.yaml")
    return load_config(path, cli)


_METRICS = ("mse", "e_kin", "sinkhorn")
_OUT_TYPES = ("none", "vtk", "pkl")
# (what must hold of a merged config, the reference's message when it does not): the rules of defaults.py:182-204
_CFG_RULES = (
    (lambda c: c.mode in ("train", "infer", "all"), ""),
    (lambda c: c.dtype in ("float32", "float64"), ""),
    (lambda c: c.dataset.src is not None, "dataset.src must be specified."),
    (lambda c: c.model.input_seq_length >= 2, "At least two positions for one past vel."),
    (lambda c: len({len(c.train.pushforward[k]) for k in ("steps", "unrolls", "probs")}) == 1, ""),
    (lambda c: min(c.train.pushforward.unrolls, default=0) >= 0, "All unrolls must be non-negative."),
    (lambda c: min(c.train.pushforward.probs, default=0) >= 0, "All probabilities must be non-negative."),
    (lambda c: min(c.train.loss_weight.values(), default=0) >= 0, "All loss weights must be non-negative."),
    (lambda c: sum(c.train.loss_weight.values()) > 0, "At least one loss weight must be non-zero."),
    (lambda c: c.eval.train.n_trajs >= -1 and c.eval.infer.n_trajs >= -1, ""),
    (lambda c: set(c.eval.train.metrics) <= set(_METRICS) and set(c.eval.infer.metrics) <= set(_METRICS), ""),
    (lambda c: c.eval.train.out_type in _OUT_TYPES and c.eval.infer.out_type in _OUT_TYPES, ""),
)


def check_cfg(cfg) -> None:
    """AssertionError (the reference's text, where it has one) for the first rule of _CFG_RULES a config breaks."""
    for holds, message in _CFG_RULES:
        if not holds(cfg):
            raise AssertionError(message)
