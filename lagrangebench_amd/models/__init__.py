from .base import BaseModel
from .egnn import EGNN
from .gns import GNS
from .linear import Linear
from .painn import PaiNN
from .segnn import SEGNN, node_irreps
from .torch_model import TorchModel

__all__ = ["BaseModel", "EGNN", "GNS", "Linear", "PaiNN", "SEGNN", "TorchModel", "node_irreps"]
