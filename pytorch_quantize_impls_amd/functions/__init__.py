"""Public function surface — the names of QuantTorch/functions/__init__.py for the four
hot-path families (BinaryNet, TernaryNet, DoReFa-Net, XNOR-Net)."""
from .binary_connect import (BinaryConnectDeterministic, BinaryConnectStochastic, BinaryConnect,
                             BinaryDense, BinaryConv2d, AP2, ShiftBatch)
from .dorefa_connect import nnDorefaQuant, DorefaQuant, nnQuantWeight, QuantDense, QuantConv2d
from .terner_connect import (TernaryConnectDeterministic, TernaryConnectStochastic, TernaryConnect,
                             TernaryDense, TernaryConv2d)
from .xnor_connect import nnQuantXnor, QuantXnor, XNORDense, XNORConv2d
from .log_lin_connect import LogQuant, LinQuant, nnQuant, Quant
from .elastic_quant_connect import (lin_proj, exp_proj, lin_deriv_l2, exp_deriv_l2, lin_deriv_l1, exp_deriv_l1, QuantWeightLin,
                                    QuantWeightExp, QuantLinDense, QuantLogDense)
from .WQR_connect import lin_deriv_WQR, exp_deriv_WQR, QuantWeightWLin, QuantWeightWExp, QuantWLinDense, QuantWLogDense
from .common import safeSign
# functions.QuantConv2d stays DoReFa's: upstream the deprecated Elastic conv op shadows it here; it is
# elastic_quant_connect.QuantConv2d (and ElasticNet.QuantConv2d).
