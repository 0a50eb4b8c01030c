"""``python -m lagrangebench_amd config=configs/rpf_2d/gns.yaml [key=value ...]`` or ``load_ckp=<dir> [key=value ...]`` - the
reference's entry point (main.py:44-77) on its own config files.

``gpu`` and ``xla_mem_fraction`` are accepted and ignored: the device is chosen with ``HIP_VISIBLE_DEVICES`` (one process)
or by ``torchrun`` (one process per GPU), and there is no XLA allocator here."""
from __future__ import annotations

import sys

from . import config as lbconfig


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    cfg = lbconfig.cli_config(argv)
    if cfg.get("gpu") is not None or cfg.get("xla_mem_fraction") is not None:
        print("gpu / xla_mem_fraction are ignored: choose the device with HIP_VISIBLE_DEVICES (or torchrun)")
    print("#" * 79, "\nStarting a LagrangeBench run with the following configs:")
    print(lbconfig.to_yaml(cfg))
    print("#" * 79)
    lbconfig.check_cfg(cfg)
    from .runner import train_or_infer
    return int(train_or_infer(cfg) or 0)


if __name__ == "__main__":
    sys.exit(main())
