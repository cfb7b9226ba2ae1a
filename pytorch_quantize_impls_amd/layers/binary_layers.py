"""BinaryNet layers (reference: QuantTorch/layers/binary_layers.py)."""
import torch

from ..functions import binary_connect
from .common import QLayer  # noqa: F401  (exported by the family alias module, as upstream)
from .sign_layers import _SignLinear, _SignConv2d


class _Binary:
    """The binary family's part of the shared sign-layer bodies (sign_layers.py)."""
    kind = "binary"

    def _set_op(self, deterministic):
        self.bin_op = binary_connect.BinaryConnectDeterministic if deterministic \
            else binary_connect.BinaryConnectStochastic

    @property
    def _op(self):
        return self.bin_op

    def _weight_on_grid(self, w):
        return (w.abs() == 1).all()


class LinearBin(_Binary, _SignLinear):
    """nn.Linear whose weight is binarised on the fly (binary_layers.py:7-46).

    ``binary_input``: None (default) = detect +-1 activations (tag from BinaryConnect, else a
    device-side check); True = caller guarantees +-1 activations; False = never take the packed
    path.  Only consulted for device tensors.
    """

    @staticmethod
    def convert(other, deterministic=True):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        # like upstream, a FRESH layer: weights are not copied (binary_layers.py:8-12)
        return LinearBin(other.in_features, other.out_features, other.bias is not None, deterministic)


class BinConv2d(_Binary, _SignConv2d):
    """nn.Conv2d with binarised weight (binary_layers.py:48-106)."""

    @staticmethod
    def convert(other, deterministic=True):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return BinConv2d(other.in_channels, other.out_channels, other.kernel_size,
                         stride=other.stride, padding=other.padding, dilation=other.dilation,
                         groups=other.groups, bias=other.bias is not None,
                         deterministic=deterministic)


class ShiftNormBatch1d(torch.nn.Module):
    """Shift-based batch norm, 1-D (binary_layers.py:110-132); torch ops, off the hot path.
    weight/bias are created uninitialised like upstream."""
    __constants__ = ['momentum', 'eps']

    def __init__(self, in_dim, eps=1e-5, momentum=0.1):
        super().__init__()
        self.in_features = in_dim
        self.weight = torch.nn.Parameter(torch.empty(in_dim))
        self.bias = torch.nn.Parameter(torch.empty(in_dim))
        self.register_buffer('running_mean', torch.zeros(in_dim))
        self.register_buffer('running_var', torch.ones(in_dim))
        self.eps = eps
        self.momentum = momentum

    def forward(self, x):
        m = self.momentum
        self.running_mean = (1 - m) * self.running_mean + m * torch.mean(x, 0).detach()
        c = x - self.running_mean
        self.running_var = (1 - m) * self.running_var + m * torch.mean(c * binary_connect.AP2(c), 0).detach()
        return binary_connect.ShiftBatch.apply(x, self.running_mean, self.running_var, self.weight,
                                               self.bias, self.eps)


class ShiftNormBatch2d(torch.nn.Module):
    """Shift-based batch norm, 2-D (binary_layers.py:137-160)."""
    __constants__ = ['momentum', 'eps']

    def __init__(self, in_channels, eps=1e-5, momentum=0.1):
        super().__init__()
        self.in_features = in_channels
        self.weight = torch.nn.Parameter(torch.empty(in_channels))
        self.bias = torch.nn.Parameter(torch.empty(in_channels))
        self.register_buffer('running_mean', torch.zeros(in_channels))
        self.register_buffer('running_var', torch.ones(in_channels))
        self.eps = eps
        self.momentum = momentum

    @staticmethod
    def _tile(tensor, dim):
        return tensor.repeat(dim[0], dim[1], 1).transpose(2, 0)

    def forward(self, x):
        dim = x.size()[-2:]
        m = self.momentum
        self.running_mean = (1 - m) * self.running_mean + m * torch.mean(x, [0, 2, 3]).detach()
        curr_mean = self._tile(self.running_mean, dim)
        c = x - curr_mean
        self.running_var = (1 - m) * self.running_var + m * torch.mean(c * binary_connect.AP2(c), [0, 2, 3]).detach()
        return binary_connect.ShiftBatch.apply(x, curr_mean, self._tile(self.running_var, dim),
                                               self._tile(self.weight, dim),
                                               self._tile(self.bias, dim), self.eps)
