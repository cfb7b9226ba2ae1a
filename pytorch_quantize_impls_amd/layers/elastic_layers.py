"""Linear / Conv2d layers of the Elastic loss-aware quantisation family (reference: QuantTorch/layers/elastic_layers.py).

Training: the weight stays real; the forward runs on the six-term real route (fp32-GEMM accuracy on the bf16 matrix cores) and the
weight gradient (Linear: also the bias gradient, as upstream) gets the fused regulariser, one launch with the coefficient buffers
read on the device.  Eval: like upstream the weight is NOT swapped; the forward uses the projection of the weight onto the level
set, computed once per weight version (version counter + storage) and cached with its GEMM operand.  When every level is exact in
bf16 (the default configurations are) the GEMM is the exact three-term route, otherwise the six-term one.

Upstream behaviour kept: conv layers keep nn.Conv2d's default init and do not regularise the bias; ``QuantConv2dLog.set_beta``
writes ``alpha``.  Fixed: ``QuantConv2dLog.clamp`` (upstream reads the missing ``bottom`` / ``top``) clamps to
+-init*gamma^(size-1); ``train(mode)`` returns ``self``.
"""
import numpy as np
import torch

from .. import lazy
from ..functions import _fused, elastic_quant_connect as EQ
from ..utils.tools import flat_net
from .common import QLayer


def _exact_in_bf16(levels) -> bool:
    lv = np.asarray(levels, dtype=np.float32)
    return bool(np.array_equal(lv.view(np.uint32) & np.uint32(0xFFFF), np.zeros_like(lv, dtype=np.uint32)))


def _real_dev(input, weight) -> bool:
    return input.is_cuda and input.dtype == torch.float32 and weight.dtype == torch.float32 and input.numel() > 0


def _copy_params(other, layer):
    """``layer`` with ``other``'s weight and bias copied in: the loss-aware ``convert``s keep the trained values."""
    layer.weight.data.copy_(other.weight.data)
    if other.bias is not None:
        layer.bias.data.copy_(other.bias.data)
    return layer


class LossQuantMixin:
    """Shared plumbing of the Elastic and WQR layers: level table and range, coefficient buffers, clamp, cached eval projection,
    the device routes."""

    def _levels(self):
        if hasattr(self, "gamma"):
            return EQ.exp_levels(self.gamma, self.init, self.size)
        return EQ.lin_levels(self.top, self.bottom, self.size)

    def _range(self):
        """(low, high) of the level set.  The Log set spans +-init*gamma^(size-1) (upstream's Log convs read the missing
        ``bottom`` / ``top``: fixed)."""
        if hasattr(self, "gamma"):
            b = self.init * self.gamma ** (self.size - 1)
            return -b, b
        return self.bottom, self.top

    def clamp(self):
        lo, hi = self._range()
        self.weight.data.clamp_(lo, hi)
        if self.bias is not None:
            self.bias.data.clamp_(lo, hi)

    def _init_coefs(self, **coefs):
        for name, value in coefs.items():
            self.register_buffer(name, torch.Tensor([value]))

    def _set_coef(self, name, value):
        setattr(self, name, torch.Tensor([value]).to(self.weight.device))

    def _project(self, w):
        return EQ.project(w, self._levels())

    def _proj_cache(self) -> dict:
        """The projected weight and its GEMM operands, valid for one (version counter, storage, level table) of the weight.  Writes
        through ``weight.data`` do not bump the version counter: call ``reset_quant_cache()`` after one."""
        w = self.weight
        key = (w._version, w.data_ptr(), self._levels())
        cache = getattr(self, "_qt_proj", None)
        if not isinstance(cache, dict) or cache.get("key") != key:
            with torch.no_grad():
                cache = {"key": key, "wq": self._project(w.detach())}
            self._qt_proj = cache
        return cache

    def reset_quant_cache(self):
        self._qt_proj = None

    def _eval_linear(self, input):
        if not _real_dev(input, self.weight):
            _fused.note_library_path(input, "loss-aware linear (eval): a non-fp32 dtype")
            return torch.nn.functional.linear(input, self._project(self.weight), self.bias)
        cache = self._proj_cache()
        wq = cache["wq"]
        if not _fused.autograd_records(input, self.weight, self.bias) and _exact_in_bf16(self._levels()):
            if "bf16x3" not in cache:
                cache["bf16x3"] = _fused.ops.weight_bf16x3(wq, "raw", terms=3)
            return _fused.ops.float_linear(input, wq, "raw", self.bias, weight_triples=cache["bf16x3"], terms=3)
        return _fused.RealLinearFn.apply(input, wq, self.bias)

    def _conv_args(self):
        return (self.stride, self.padding, self.dilation, self.groups)

    def _conv_dev(self, input) -> bool:
        return (_real_dev(input, self.weight) and input.dim() == 4 and self.groups == 1 and self.padding_mode == "zeros"
                and not isinstance(self.padding, str))

    def _conv(self, input, w):
        if self._conv_dev(input):
            return _fused.RealConv2dFn.apply(input, w, self.bias, self._conv_args())
        _fused.note_library_path(input, "loss-aware conv: groups, a padding mode or a non-fp32 dtype")
        return torch.nn.functional.conv2d(input, w, self.bias, *self._conv_args())

    def _eval_conv(self, input):
        if not self._conv_dev(input):
            return self._conv(input, self._project(self.weight))
        cache = self._proj_cache()
        wq = cache["wq"]
        if not _fused.autograd_records(input, self.weight, self.bias) and _exact_in_bf16(self._levels()):
            if "conv_bf16x3" not in cache:
                cache["conv_bf16x3"] = _fused.ops.pack_conv_weight_bf16x3(wq, "raw", terms=3)
            N, C, H, W = input.shape
            kh, kw = int(wq.shape[2]), int(wq.shape[3])
            y2 = _fused.ops.float_conv2d(input, wq, "raw", self.bias, self.stride, self.padding, self.dilation,
                                         weight_triples=cache["conv_bf16x3"], terms=3)
            Ho, Wo = _fused.ops.conv_out_hw(H, W, kh, kw, self.stride, self.padding, self.dilation)
            return _fused.nchw_result(y2, input, N, Ho, Wo, wq.shape[0])
        return self._conv(input, wq)


class _LossQuantLinear(LossQuantMixin, torch.nn.Module, QLayer):
    """Parameter setup of the loss-aware Linear layers (Elastic and WQR)."""

    def _init_linear(self, in_features, out_features, bias, **coefs):
        self.in_features, self.out_features = in_features, out_features
        self._init_coefs(**coefs)
        self.weight = torch.nn.Parameter(torch.empty(out_features, in_features))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        """Weight uniform over the level range, bias 0."""
        lo, hi = self._range()
        self.weight.data.uniform_(lo, hi)
        if self.bias is not None:
            self.bias.data.zero_()


class _ElasticTrain:
    def train(self, mode=True):
        """Upstream only flips the flag (no weight swap); returns ``self`` (upstream: None)."""
        self.training = mode
        return self

    def set_alpha(self, alpha):
        self._set_coef("alpha", alpha)

    def set_beta(self, beta):
        self._set_coef("beta", beta)


class _ElasticLinear(_ElasticTrain, _LossQuantLinear):
    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        if self.training:
            return self.linear_op.apply(input, self.weight, self.bias, self.alpha, self.beta)
        return self._eval_linear(input)


class _ElasticConv(_ElasticTrain, LossQuantMixin, torch.nn.Conv2d, QLayer):
    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        if self.training:
            return self._conv(input, self.weight_op.apply(self.weight, self.alpha, self.beta))
        return self._eval_conv(input)


class LinearQuantLin(_ElasticLinear):
    @staticmethod
    def convert(other, bottom=-1, top=1, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        return _copy_params(other, LinearQuantLin(other.in_features, other.out_features, other.bias is not None, bottom=bottom,
                                                 top=top, size=size, alpha=alpha, beta=beta))

    def __init__(self, in_features, out_features, bias=True, bottom=-1, top=1, size=5, alpha=0, beta=0):
        torch.nn.Module.__init__(self)
        self.bottom, self.top, self.size = bottom, top, size
        self._init_linear(in_features, out_features, bias, alpha=alpha, beta=beta)
        self.linear_op = EQ.QuantLinDense(size=size, bottom=bottom, top=top)


class LinearQuantLog(_ElasticLinear):
    @staticmethod
    def convert(other, gamma=2, init=0.25, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        return _copy_params(other, LinearQuantLog(other.in_features, other.out_features, other.bias is not None, gamma=gamma,
                                                 init=init, size=size, alpha=alpha, beta=beta))

    def __init__(self, in_features, out_features, bias=True, gamma=2, init=0.25, size=5, alpha=0, beta=0):
        torch.nn.Module.__init__(self)
        self.gamma, self.init, self.size = gamma, init, size
        self._init_linear(in_features, out_features, bias, alpha=alpha, beta=beta)
        self.linear_op = EQ.QuantLogDense(gamma=gamma, init=init, size=size)


class QuantConv2dLin(_ElasticConv):
    @staticmethod
    def convert(other, bottom=-1, top=1, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return _copy_params(other, QuantConv2dLin(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride,
                                                 padding=other.padding, dilation=other.dilation, groups=other.groups,
                                                 bias=other.bias is not None, bottom=bottom, top=top, size=size, alpha=alpha,
                                                 beta=beta))

    def __init__(self, in_channels, out_channels, kernel_size, bottom=-1, top=1, size=5, alpha=0, beta=0, stride=1, padding=1,
                 dilation=1, groups=1, bias=True):
        self.top, self.bottom, self.size = top, bottom, size
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)
        self._init_coefs(alpha=alpha, beta=beta)
        self.weight_op = EQ.QuantWeightLin(self.top, self.bottom, self.size)


class QuantConv2dLog(_ElasticConv):
    @staticmethod
    def convert(other, gamma=2, init=0.25, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return _copy_params(other, QuantConv2dLog(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride,
                                                 padding=other.padding, dilation=other.dilation, groups=other.groups,
                                                 bias=other.bias is not None, gamma=gamma, init=init, size=size, alpha=alpha,
                                                 beta=beta))

    def __init__(self, in_channels, out_channels, kernel_size, gamma=2, init=0.25, size=5, alpha=0, beta=0, stride=1, padding=1,
                 dilation=1, groups=1, bias=True):
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)
        self.gamma, self.init, self.size = gamma, init, size
        self._init_coefs(alpha=alpha, beta=beta)
        self.weight_op = EQ.QuantWeightExp(gamma=self.gamma, init=self.init, size=self.size)

    def set_beta(self, beta):
        """Writes ``alpha``, as upstream (elastic_layers.py QuantConv2dLog.set_beta)."""
        self._set_coef("alpha", beta)


_ELASTIC = (LinearQuantLin, LinearQuantLog, QuantConv2dLin, QuantConv2dLog)


def set_model_alpha(model, alpha):
    for layer in flat_net(model, _ELASTIC):
        layer.set_alpha(alpha)


def set_model_beta(model, beta):
    for layer in flat_net(model, _ELASTIC):
        layer.set_beta(beta)
