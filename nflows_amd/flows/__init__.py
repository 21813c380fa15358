from .base import Flow
from .autoregressive import MaskedAutoregressiveFlow
from .realnvp import SimpleRealNVP
