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


class LossQuantMixin:
    """Shared plumbing: level table, cached eval projection, the device routes."""

    def _levels(self):
        if hasattr(self, "gamma"):
            return EQ.exp_levels(self.gamma, self.init, self.size)
        return EQ.lin_levels(self.top, self.bottom, self.size)

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

    def _no_grad_for(self, input) -> bool:
        return not (torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad
                                                 or (self.bias is not None and self.bias.requires_grad)))

    def _eval_linear(self, input):
        if not _real_dev(input, self.weight):
            _fused.note_library_path(input, "loss-aware linear (eval): a non-fp32 dtype")
            return torch.nn.functional.linear(input, self._project(self.weight), self.bias)
        cache = self._proj_cache()
        wq = cache["wq"]
        if self._no_grad_for(input):
            if _exact_in_bf16(self._levels()):
                if "bf16x3" not in cache:
                    cache["bf16x3"] = _fused.ops.weight_bf16x3(wq, "raw", terms=3)
                return _fused.ops.float_linear(input, wq, "raw", self.bias, weight_triples=cache["bf16x3"], terms=3)
            return _fused.RealLinearFn.apply(input, wq, self.bias)
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
        if self._no_grad_for(input) and _exact_in_bf16(self._levels()):
            if "conv_bf16x3" not in cache:
                cache["conv_bf16x3"] = _fused.ops.pack_conv_weight_bf16x3(wq, "raw", terms=3)
            N, C, H, W = input.shape
            kh, kw = int(wq.shape[2]), int(wq.shape[3])
            y2 = _fused.ops.float_conv2d(input, wq, "raw", self.bias, self.stride, self.padding, self.dilation,
                                         weight_triples=cache["conv_bf16x3"], terms=3)
            Ho, Wo = _fused.ops.conv_out_hw(H, W, kh, kw, self.stride, self.padding, self.dilation)
            y = y2.view(N, Ho, Wo, wq.shape[0]).permute(0, 3, 1, 2)
            if input.is_contiguous() and not input.is_contiguous(memory_format=torch.channels_last):
                y = y.contiguous()
            return y
        return self._conv(input, wq)

    def _set_coef(self, name, value):
        setattr(self, name, torch.Tensor([value]).to(self.weight.device))


class _ElasticTrain:
    def train(self, mode=True):
        """Upstream only flips the flag (no weight swap); returns ``self`` (upstream: None)."""
        self.training = mode
        return self


class LinearQuantLin(_ElasticTrain, LossQuantMixin, torch.nn.Module, QLayer):
    @staticmethod
    def convert(other, bottom=-1, top=1, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        result = LinearQuantLin(other.in_features, other.out_features, other.bias is not None, bottom=bottom, top=top, size=size,
                                alpha=alpha, beta=beta)
        result.weight.data.copy_(other.weight.data)
        if other.bias is not None:
            result.bias.data.copy_(other.bias.data)
        return result

    def __init__(self, in_features, out_features, bias=True, bottom=-1, top=1, size=5, alpha=0, beta=0):
        torch.nn.Module.__init__(self)
        self.in_features, self.out_features = in_features, out_features
        self.bottom, self.top, self.size = bottom, top, size
        self.register_buffer("alpha", torch.Tensor([alpha]))
        self.register_buffer("beta", torch.Tensor([beta]))
        self.weight = torch.nn.Parameter(torch.empty(out_features, in_features))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self.linear_op = EQ.QuantLinDense(size=size, bottom=bottom, top=top)

    def reset_parameters(self):
        self.weight.data.uniform_(self.bottom, self.top)
        if self.bias is not None:
            self.bias.data.zero_()

    def clamp(self):
        self.weight.data.clamp_(self.bottom, self.top)
        if self.bias is not None:
            self.bias.data.clamp_(self.bottom, self.top)

    def set_alpha(self, alpha):
        self._set_coef("alpha", alpha)

    def set_beta(self, beta):
        self._set_coef("beta", beta)

    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        if self.training:
            return self.linear_op.apply(input, self.weight, self.bias, self.alpha, self.beta)
        return self._eval_linear(input)


class LinearQuantLog(_ElasticTrain, LossQuantMixin, torch.nn.Module, QLayer):
    @staticmethod
    def convert(other, gamma=2, init=0.25, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        result = LinearQuantLog(other.in_features, other.out_features, other.bias is not None, gamma=gamma, init=init, size=size,
                                alpha=alpha, beta=beta)
        result.weight.data.copy_(other.weight.data)
        if other.bias is not None:
            result.bias.data.copy_(other.bias.data)
        return result

    def __init__(self, in_features, out_features, bias=True, gamma=2, init=0.25, size=5, alpha=0, beta=0):
        torch.nn.Module.__init__(self)
        self.in_features, self.out_features = in_features, out_features
        self.gamma, self.init, self.size = gamma, init, size
        self.register_buffer("alpha", torch.Tensor([alpha]))
        self.register_buffer("beta", torch.Tensor([beta]))
        self.weight = torch.nn.Parameter(torch.empty(out_features, in_features))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self.linear_op = EQ.QuantLogDense(gamma=gamma, init=init, size=size)

    def _bound(self):
        return self.init * self.gamma ** (self.size - 1)

    def reset_parameters(self):
        self.weight.data.uniform_(-self._bound(), self._bound())
        if self.bias is not None:
            self.bias.data.zero_()

    def clamp(self):
        self.weight.data.clamp_(-self._bound(), self._bound())
        if self.bias is not None:
            self.bias.data.clamp_(-self._bound(), self._bound())

    def set_alpha(self, alpha):
        self._set_coef("alpha", alpha)

    def set_beta(self, beta):
        self._set_coef("beta", beta)

    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        if self.training:
            return self.linear_op.apply(input, self.weight, self.bias, self.alpha, self.beta)
        return self._eval_linear(input)


class QuantConv2dLin(_ElasticTrain, LossQuantMixin, torch.nn.Conv2d, QLayer):
    @staticmethod
    def convert(other, bottom=-1, top=1, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        result = QuantConv2dLin(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride, padding=other.padding,
                                dilation=other.dilation, groups=other.groups, bias=other.bias is not None, bottom=bottom, top=top,
                                size=size, alpha=alpha, beta=beta)
        result.weight.data.copy_(other.weight.data)
        if other.bias is not None:
            result.bias.data.copy_(other.bias.data)
        return result

    def __init__(self, in_channels, out_channels, kernel_size, bottom=-1, top=1, size=5, alpha=0, beta=0, stride=1, padding=1,
                 dilation=1, groups=1, bias=True):
        self.top, self.bottom, self.size = top, bottom, size
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)
        self.register_buffer("alpha", torch.Tensor([alpha]))
        self.register_buffer("beta", torch.Tensor([beta]))
        self.weight_op = EQ.QuantWeightLin(self.top, self.bottom, self.size)

    def clamp(self):
        self.weight.data.clamp_(self.bottom, self.top)
        if self.bias is not None:
            self.bias.data.clamp_(self.bottom, self.top)

    def set_alpha(self, alpha):
        self._set_coef("alpha", alpha)

    def set_beta(self, beta):
        self._set_coef("beta", beta)

    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        if self.training:
            return self._conv(input, self.weight_op.apply(self.weight, self.alpha, self.beta))
        return self._eval_conv(input)


class QuantConv2dLog(_ElasticTrain, LossQuantMixin, torch.nn.Conv2d, QLayer):
    @staticmethod
    def convert(other, gamma=2, init=0.25, size=5, alpha=0, beta=0):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        result = QuantConv2dLog(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride, padding=other.padding,
                                dilation=other.dilation, groups=other.groups, bias=other.bias is not None, gamma=gamma, init=init,
                                size=size, alpha=alpha, beta=beta)
        result.weight.data.copy_(other.weight.data)
        if other.bias is not None:
            result.bias.data.copy_(other.bias.data)
        return result

    def __init__(self, in_channels, out_channels, kernel_size, gamma=2, init=0.25, size=5, alpha=0, beta=0, stride=1, padding=1,
                 dilation=1, groups=1, bias=True):
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                                 groups=groups, bias=bias)
        self.gamma, self.init, self.size = gamma, init, size
        self.register_buffer("alpha", torch.Tensor([alpha]))
        self.register_buffer("beta", torch.Tensor([beta]))
        self.weight_op = EQ.QuantWeightExp(gamma=self.gamma, init=self.init, size=self.size)

    def clamp(self):
        """Fixed: upstream reads the missing ``bottom`` / ``top``; the Log set spans +-init*gamma^(size-1)."""
        bound = self.init * self.gamma ** (self.size - 1)
        self.weight.data.clamp_(-bound, bound)
        if self.bias is not None:
            self.bias.data.clamp_(-bound, bound)

    def set_alpha(self, alpha):
        self._set_coef("alpha", alpha)

    def set_beta(self, beta):
        """Writes ``alpha``, as upstream (elastic_layers.py QuantConv2dLog.set_beta)."""
        self._set_coef("alpha", beta)

    def forward(self, input):
        lazy.note_inference_call(self, input)
        input = lazy.resolve(input)
        if self.training:
            return self._conv(input, self.weight_op.apply(self.weight, self.alpha, self.beta))
        return self._eval_conv(input)


_ELASTIC = (LinearQuantLin, LinearQuantLog, QuantConv2dLin, QuantConv2dLog)


def set_model_alpha(model, alpha):
    for layer in flat_net(model, _ELASTIC):
        layer.set_alpha(alpha)


def set_model_beta(model, beta):
    for layer in flat_net(model, _ELASTIC):
        layer.set_beta(beta)
