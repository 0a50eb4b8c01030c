from .base import BaseModel
from .egnn import EGNN
from .gns import GNS
from .segnn import SEGNN, node_irreps

__all__ = ["BaseModel", "EGNN", "GNS", "SEGNN", "node_irreps"]
