from .buffers import Buffer, PrioritizedBuffer
from .segments import Segment, flatten_batch

__all__ = ['Buffer', 'PrioritizedBuffer', 'Segment', 'flatten_batch']
