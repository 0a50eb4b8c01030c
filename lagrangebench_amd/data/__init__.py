from .data import H5Dataset, force_spec_from_callable, get_dataset_name_from_path
from .device import DeviceDataset
from .synthetic import SyntheticDataset, make_case, make_padded_case, write_padded_h5
from .utils import get_dataset_stats, numpy_collate

__all__ = ["H5Dataset", "DeviceDataset", "SyntheticDataset", "make_case", "make_padded_case", "write_padded_h5", "get_dataset_stats", "numpy_collate",
           "get_dataset_name_from_path", "force_spec_from_callable"]
