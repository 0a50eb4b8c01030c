from .base import BaseModel
from .egnn import EGNN
from .gns import GNS
from .painn import PaiNN
from .segnn import SEGNN, node_irreps

__all__ = ["BaseModel", "EGNN", "GNS", "PaiNN", "SEGNN", "node_irreps"]
