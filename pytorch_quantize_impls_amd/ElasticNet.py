"""Family alias module: everything of the Elastic family under one name (reference: QuantTorch/ElasticNet.py:1-2).  Its
``QuantConv2d`` is the deprecated Elastic conv op (functions.QuantConv2d stays DoReFa's)."""
from .functions.elastic_quant_connect import *  # noqa: F401,F403
from .layers.elastic_layers import *  # noqa: F401,F403
from .device import device  # noqa: F401  (the reference's family modules re-export it)
