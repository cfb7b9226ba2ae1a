"""Linear / Conv2d layers of the WQR loss-aware quantisation family (reference: QuantTorch/layers/WQR_layers.py).

All four layers fail in their constructor upstream (they call names ``WQR_connect`` does not define — ``QuantLinDense``,
``QuantLogDense``, ``QuantWeightLin``, ``QuantWeightExp`` — or read the missing ``self.bottom``); here they are built on
``QuantWLinDense`` / ``QuantWLogDense`` / ``QuantWeightWLin`` / ``QuantWeightWExp``, and the Log conv uses ``exp_proj`` and
+-init*gamma^(size-1) where upstream reads ``bottom`` / ``top``.  ``QuantConv2dWLog`` also takes ``bias`` (upstream's signature
lacks it, so its own ``convert`` cannot call it).

Unlike the Elastic layers, ``eval()`` swaps the weight for its projection (kept in ``weight.org``) and ``train()`` restores it, as
upstream; the forward is the training op in both modes (six-term real route, fused regulariser in backward).  Kept: Linear layers
regularise the bias gradient, conv layers do not; ``QuantConv2dWLog.set_beta`` writes ``alpha``.  Fixed: ``set_model_kapa`` /
``set_model_beta`` select the WQR layers (upstream names classes it does not import: NameError); ``train(mode)`` returns ``self``.
"""
import torch

from .. import lazy
from ..functions import WQR_connect
from ..utils.tools import flat_net
from .common import QLayer
from .elastic_layers import _LossQuantLinear, LossQuantMixin, _copy_params


class _WqrTrain:
    def train(self, mode=True):
        """Weight swap as upstream: eval() keeps the real weight in ``weight.org`` and writes its projection into ``weight``."""
        if self.training == mode:
            return self
        self.training = mode
        if mode:
            self.weight.data.copy_(self.weight.org.data)
        else:
            if not hasattr(self.weight, "org"):
                self.weight.org = self.weight.data.clone()
            self.weight.org.data.copy_(self.weight.data)
            with torch.no_grad():
                self.weight.data.copy_(self._project(self.weight.detach()))
        return self

    def set_kapa(self, kapa):
        self._set_coef("kapa", kapa)

    def set_beta(self, beta):
        self._set_coef("beta", beta)


class _WqrLinear(_WqrTrain, _LossQuantLinear):
    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        return self.linear_op.apply(input, self.weight, self.bias, self.kapa, self.beta)


class LinearQuantWLin(_WqrLinear):
    @staticmethod
    def convert(other, bottom=-1, top=1, size=5, kapa=0, beta=0):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        return _copy_params(other, LinearQuantWLin(other.in_features, other.out_features, other.bias is not None, bottom=bottom,
                                                  top=top, size=size, kapa=kapa, beta=beta))

    def __init__(self, in_features, out_features, bias=True, bottom=-1, top=1, size=5, kapa=0, beta=0):
        torch.nn.Module.__init__(self)
        self.bottom, self.top, self.size = bottom, top, size
        self._init_linear(in_features, out_features, bias, kapa=kapa, beta=beta)
        self.linear_op = WQR_connect.QuantWLinDense(size=size, bottom=bottom, top=top)


class LinearQuantWLog(_WqrLinear):
    @staticmethod
    def convert(other, gamma=2, init=0.25, size=5, kapa=0, beta=0):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        return _copy_params(other, LinearQuantWLog(other.in_features, other.out_features, other.bias is not None, gamma=gamma,
                                                  init=init, size=size, kapa=kapa, beta=beta))

    def __init__(self, in_features, out_features, bias=True, gamma=2, init=0.25, size=5, kapa=0, beta=0):
        torch.nn.Module.__init__(self)
        self.gamma, self.init, self.size = gamma, init, size
        self._init_linear(in_features, out_features, bias, kapa=kapa, beta=beta)
        self.linear_op = WQR_connect.QuantWLogDense(gamma=gamma, init=init, size=size)


class _WqrConv(_WqrTrain, LossQuantMixin, torch.nn.Conv2d, QLayer):
    def reset_parameters(self):
        """Uniform over the level range, bias 0 (upstream's QuantConv2dWLin; the Log conv's is fixed to +-init*gamma^(size-1))."""
        _LossQuantLinear.reset_parameters(self)

    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        return self._conv(input, self.weight_op.apply(self.weight, self.kapa, self.beta))


class QuantConv2dWLin(_WqrConv):
    @staticmethod
    def convert(other, bottom=-1, top=1, size=5, kapa=0, beta=0):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return _copy_params(other, QuantConv2dWLin(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride,
                                                  padding=other.padding, dilation=other.dilation, groups=other.groups,
                                                  bias=other.bias is not None, bottom=bottom, top=top, size=size, kapa=kapa,
                                                  beta=beta))

    def __init__(self, in_channels, out_channels, kernel_size, bottom=-1, top=1, size=5, kapa=0, beta=0, stride=1, padding=1,
                 dilation=1, groups=1, bias=True):
        self.top, self.bottom, self.size = top, bottom, size
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)
        self._init_coefs(kapa=kapa, beta=beta)
        self.weight_op = WQR_connect.QuantWeightWLin(self.top, self.bottom, self.size)


class QuantConv2dWLog(_WqrConv):
    @staticmethod
    def convert(other, gamma=2, init=0.25, size=5, kapa=0, beta=0):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return _copy_params(other, QuantConv2dWLog(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride,
                                                  padding=other.padding, dilation=other.dilation, groups=other.groups,
                                                  bias=other.bias is not None, gamma=gamma, init=init, size=size, kapa=kapa,
                                                  beta=beta))

    def __init__(self, in_channels, out_channels, kernel_size, gamma=2, init=0.25, size=5, kapa=0, beta=0, stride=1, padding=1,
                 dilation=1, groups=1, bias=True):
        self.gamma, self.init, self.size = gamma, init, size
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)
        self._init_coefs(kapa=kapa, beta=beta)
        self.weight_op = WQR_connect.QuantWeightWExp(gamma=self.gamma, init=self.init, size=self.size)

    def set_beta(self, beta):
        """Writes ``alpha``, as upstream (WQR_layers.py QuantConv2dWLog.set_beta)."""
        self._set_coef("alpha", beta)


_WQR = (LinearQuantWLin, LinearQuantWLog, QuantConv2dWLin, QuantConv2dWLog)


def set_model_kapa(model, kapa):
    for layer in flat_net(model, _WQR):
        layer.set_kapa(kapa)


def set_model_beta(model, beta):
    for layer in flat_net(model, _WQR):
        layer.set_beta(beta)
