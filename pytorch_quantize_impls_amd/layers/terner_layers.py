"""TernaryNet layers (reference: QuantTorch/layers/terner_layers.py)."""
import torch

from ..functions import terner_connect
from .common import QLayer  # noqa: F401  (exported by the family alias module, as upstream)
from .sign_layers import _SignLinear, _SignConv2d


class _Ternary:
    """The ternary family's part of the shared sign-layer bodies (sign_layers.py)."""
    kind = "ternary"

    def _set_op(self, deterministic):
        self.ter_op = terner_connect.TernaryConnectDeterministic if deterministic \
            else terner_connect.TernaryConnectStochastic

    @property
    def _op(self):
        return self.ter_op

    def _weight_on_grid(self, w):
        return ((w == 0) | (w.abs() == 1)).all()


class LinearTer(_Ternary, _SignLinear):
    """nn.Linear with a ternarised weight (terner_layers.py:10-51)."""

    @staticmethod
    def convert(other, dtype="lin", deterministic=True):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        return LinearTer(other.in_features, other.out_features, other.bias is not None,
                         deterministic=deterministic)


class TerConv2d(_Ternary, _SignConv2d):
    """nn.Conv2d with a ternarised weight (terner_layers.py:54-92)."""

    @staticmethod
    def convert(other, deterministic=True):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return TerConv2d(other.in_channels, other.out_channels, other.kernel_size,
                         stride=other.stride, padding=other.padding, dilation=other.dilation,
                         groups=other.groups, bias=other.bias is not None,
                         deterministic=deterministic)
