"""Family alias module: everything of the WQR family under one name (reference: QuantTorch/WqrNet.py:1-2)."""
from .functions.WQR_connect import *  # noqa: F401,F403
from .layers.WQR_layers import *  # noqa: F401,F403
from .device import device  # noqa: F401  (the reference's family modules re-export it)
