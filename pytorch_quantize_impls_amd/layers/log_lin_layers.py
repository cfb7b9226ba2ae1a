"""Linear / Conv2d with Lin or Log fixed-point weights (reference: QuantTorch/layers/log_lin_layers.py).

The quantised weight levels — multiples of 2^(fsr - bit_width) up to 2^fsr (Lin, bit_width <= 8) or signed powers
of two (Log) — are exactly representable in bf16, so on a HIP device the contraction of a real-valued activation
with them runs on the bf16 matrix cores through the exact bf16-triple split (same route as the first layer of a
binary net): fp32-GEMM accuracy, and for Log weights this IS the shift-add GEMM the paper motivates.

Under autograd a device fp32 input trains on functions._fused.LogLinLinearFn / LogLinConv2dFn (one quantise-and-pack launch of the
weight per step, exact three-term forward and grad_x, six-term grad_W); configurations whose levels are not exact in bf16
(ops.levels_exact_in_bf16: Lin bit_width > 8, Log levels below 2^-126) on RealLinearFn / RealConv2dFn.  Only grouped convs,
non-"zeros" padding modes, string padding and non-fp32 dtypes take the (counted) dense library.

An activation that is itself exact in bf16 — the output of nnQuant, which carries its one-term plane as a tag, or a pooled /
reshaped one that the detection recognises (_fused.loglin_act_planes) — is contracted as ONE bf16 term against a one-term
weight plane, in training, no-grad and eval mode alike (_fused.LOGLIN_ONE_TERM).
"""
import torch

from .. import lazy, packed
from ..functions import _fused, log_lin_connect
from .common import EvalSwapMixin, QLayer


def _exact_in_bf16(dtype, bit_width):
    return dtype == "log" or (dtype == "lin" and bit_width <= 8)


def _autograd_on_device(layer, input) -> bool:
    """A device fp32 input of a device fp32 layer with autograd recording: the training routes of functions._fused."""
    return (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0 and layer.weight.is_cuda
            and layer.weight.dtype == torch.float32 and _fused.autograd_records(input, layer.weight))


class _WeightInit:
    def reset_parameters(self):
        """uniform magnitude in [2^(fsr - bit_width), 2^fsr] with a random sign, bias 0 (log_lin_layers.py:34-38)."""
        if getattr(self, "bit_width", None) is None:     # nn.Linear/Conv2d.__init__ calls this before our fields exist
            return super().reset_parameters()
        torch.nn.init.uniform_(self.weight, 2 ** (self.fsr - self.bit_width), 2 ** self.fsr)
        self.weight.data.mul_((torch.rand_like(self.weight) < 0.5).type(self.weight.dtype) * 2 - 1)
        if self.bias is not None:
            self.bias.data.zero_()

    def clamp(self):
        self.weight.data.clamp_(-1 * 2 ** self.fsr, 2 ** self.fsr)

    def _quantized_weight_for_eval(self):
        return self.weight_op.forward(self.weight)


class LinearQuant(_WeightInit, EvalSwapMixin, torch.nn.Linear, QLayer):
    """log_lin_layers.py:6-43.  Like upstream, forward re-applies the (idempotent) weight quantiser in eval mode too."""

    @staticmethod
    def convert(other, dtype="lin", fsr=7, bit_width=3):
        if not isinstance(other, torch.nn.Linear):
            raise TypeError("Expected a torch.nn.Linear ! Receive:  {}".format(other.__class__))
        return LinearQuant(other.in_features, other.out_features, other.bias is not None, dtype=dtype, fsr=fsr,
                           bit_width=bit_width)

    def __init__(self, in_features, out_features, bias=True, dtype="lin", fsr=7, bit_width=3):
        self.bit_width, self.fsr, self.qdtype = bit_width, fsr, dtype
        torch.nn.Linear.__init__(self, in_features, out_features, bias=bias)
        self.weight_op = log_lin_connect.nnQuant(dtype=dtype, fsr=fsr, bit_width=bit_width, with_sign=True, lin_back=True)

    def forward(self, input):
        if lazy.DEFER_LEVELS:          # opt-in: the deferred level chain (lazy.py, kind "levels")
            return lazy.levels_linear_forward(self, input)
        lazy.note_inference_call(self, input)
        return self._forward_impl(input)

    def _forward_impl(self, input):
        input = lazy.resolve(input)
        if _autograd_on_device(self, input):
            if _fused.ops.levels_exact_in_bf16(self.qdtype, self.fsr, self.bit_width):
                return _fused.LogLinLinearFn.apply(input, self.weight, self.bias, (self.qdtype, self.fsr, self.bit_width, True))
            return _fused.RealLinearFn.apply(input, self.weight_op.forward(self.weight), self.bias)
        if (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0 and self.weight.is_cuda
                and self.weight.dtype == torch.float32 and not _fused.autograd_records(input, self.weight)
                and _fused.ops.levels_exact_in_bf16(self.qdtype, self.fsr, self.bit_width)):
            planes, flag = _fused.loglin_act_planes(input, self.weight, packed.ROWS_LAST)
            if planes is not None:      # one term x one term; the weight plane comes from the quantise-and-pack launch
                quant = (self.qdtype, self.fsr, self.bit_width, True)
                wt = _fused.ops.pack_levels_bf16x3(self.weight, *quant, grad_x=False, fwd_terms=1)[0] if self.training else \
                    self._eval_planes(lambda _w2: _fused.ops.pack_levels_bf16x3(self.weight, *quant, grad_x=False, fwd_terms=1)[0],
                                      key="bf16x1_levels")
                bias = self.bias.detach() if self.bias is not None else None
                y = _fused.ops.float_linear(None, self.weight.detach(), "raw",
                                            _fused.poison_bias(bias, flag, self.weight.shape[0], input.device),
                                            weight_triples=wt, planes=planes)
                return y.view(*input.shape[:-1], self.weight.shape[0])
        wq = self.weight_op.forward(self.weight)
        if (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0 and _exact_in_bf16(self.qdtype, self.bit_width)
                and not _fused.autograd_records(input, self.weight)):
            # Lin / Log levels are exact in bf16 (fp32's exponent range), not necessarily in fp16: the exact three-term route
            wt = None if self.training else self._eval_planes(
                lambda w2: _fused.ops.weight_bf16x3(w2, "raw", terms=3), key="bf16x3_raw")
            return _fused.ops.float_linear(input, wq.detach(), "raw", self.bias, weight_triples=wt, terms=3)
        _fused.note_library_path(input, "Lin/Log linear: a non-fp32 dtype, or levels beyond bf16 without autograd")
        return torch.nn.functional.linear(input, wq, self.bias)


class QuantConv2d(_WeightInit, EvalSwapMixin, torch.nn.Conv2d, QLayer):
    """log_lin_layers.py:46-101."""

    @staticmethod
    def convert(other, fsr=7, bit_width=3, dtype="lin"):
        if not isinstance(other, torch.nn.Conv2d):
            raise TypeError("Expected a torch.nn.Conv2d ! Receive:  {}".format(other.__class__))
        return QuantConv2d(other.in_channels, other.out_channels, other.kernel_size, stride=other.stride,
                           padding=other.padding, dilation=other.dilation, groups=other.groups,
                           bias=other.bias is not None, fsr=fsr, bit_width=bit_width, dtype=dtype)

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 fsr=7, bit_width=3, dtype="lin"):
        self.fsr, self.bit_width, self.qdtype = fsr, bit_width, dtype
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                                 dilation=dilation, groups=groups, bias=bias)
        self.weight_op = log_lin_connect.nnQuant(dtype=dtype, fsr=fsr, bit_width=bit_width, with_sign=True, lin_back=True)

    def forward(self, input):
        if lazy.DEFER_LEVELS:          # opt-in: the deferred level chain (lazy.py, kind "levels")
            return lazy.levels_conv_forward(self, input)
        lazy.note_inference_call(self, input)
        return self._forward_impl(input)

    def _forward_impl(self, input):
        if isinstance(input, packed.LevelActivation):
            return self._forward_levels(input)
        input = lazy.resolve(input)
        if (_autograd_on_device(self, input) and input.dim() == 4 and self.groups == 1 and self.padding_mode == "zeros"
                and not isinstance(self.padding, str)):
            args = (self.stride, self.padding, self.dilation, 1)
            if _fused.ops.levels_exact_in_bf16(self.qdtype, self.fsr, self.bit_width):
                # eval: the swapped weight already holds the levels -> packed as it is (LinQuant(bit_width = 32) = identity)
                quant = (self.qdtype, self.fsr, self.bit_width, True) if self.training else ("lin", 0, 32, True)
                return _fused.LogLinConv2dFn.apply(input, self.weight, self.bias, quant, args)
            wq = self.weight_op.forward(self.weight) if self.training else self.weight
            return _fused.RealConv2dFn.apply(input, wq, self.bias, args)
        if (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0 and input.dim() == 4
                and self.groups == 1 and self.padding_mode == "zeros" and not isinstance(self.padding, str)
                and self.weight.is_cuda and self.weight.dtype == torch.float32
                and not _fused.autograd_records(input, self.weight)
                and _fused.ops.levels_exact_in_bf16(self.qdtype, self.fsr, self.bit_width)):
            planes, flag = _fused.loglin_act_planes(input, self.weight, packed.NHWC)
            if planes is not None:      # one term x one term on the implicit GEMM
                # eval: the swapped weight already holds the levels -> packed as it is (LinQuant(bit_width = 32) = identity)
                quant = (self.qdtype, self.fsr, self.bit_width, True) if self.training else ("lin", 0, 32, True)
                wt = _fused.ops.pack_levels_bf16x3(self.weight, *quant, grad_x=False, fwd_terms=1)[0] if self.training else \
                    self._eval_planes(lambda _w2: _fused.ops.pack_levels_bf16x3(self.weight, *quant, grad_x=False, fwd_terms=1)[0],
                                      key="conv_bf16x1_levels")
                N, C, H, W = input.shape
                Cout, kh, kw = int(self.weight.shape[0]), int(self.weight.shape[2]), int(self.weight.shape[3])
                bias = self.bias.detach() if self.bias is not None else None
                y2 = _fused.ops.float_conv2d(None, self.weight.detach(), "raw", _fused.poison_bias(bias, flag, Cout, input.device),
                                             self.stride, self.padding, self.dilation, weight_triples=wt, pixels=planes,
                                             in_shape=tuple(input.shape))
                Ho, Wo = _fused.ops.conv_out_hw(H, W, kh, kw, self.stride, self.padding, self.dilation)
                return _fused.nchw_result(y2, input, N, Ho, Wo, Cout)
        wq = self.weight_op.forward(self.weight) if self.training else self.weight
        if (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0 and input.dim() == 4
                and self.groups == 1 and self.padding_mode == "zeros" and not isinstance(self.padding, str)
                and _exact_in_bf16(self.qdtype, self.bit_width) and not _fused.autograd_records(input, self.weight)):
            wt = None if self.training else self._eval_planes(
                lambda _w2: _fused.ops.pack_conv_weight_bf16x3(self.weight.detach(), "raw", terms=3), key="conv_bf16x3_raw")
            N, C, H, W = input.shape
            kh, kw = int(self.weight.shape[2]), int(self.weight.shape[3])
            # levels exact in bf16, not necessarily in fp16: the exact three-term route, named explicitly
            y2 = _fused.ops.float_conv2d(input, wq.detach(), "raw", self.bias, self.stride, self.padding, self.dilation,
                                         weight_triples=wt, terms=3)
            Ho, Wo = _fused.ops.conv_out_hw(H, W, kh, kw, self.stride, self.padding, self.dilation)
            return _fused.nchw_result(y2, input, N, Ho, Wo, self.weight.shape[0])
        _fused.note_library_path(input, "Lin/Log conv: groups, padding mode, a non-fp32 dtype, or levels beyond bf16 without autograd")
        return torch.nn.functional.conv2d(input, wq, self.bias, self.stride, self.padding, self.dilation, self.groups)

    def _forward_levels(self, act):
        """The fp32 result for an activation that exists as a level plane only (a deferred chain that has to hand out this conv's
        value): the one-term contraction of the ordinary eval path on that plane — the same bits."""
        act = act.without_halo()
        N, C, H, W = act.shape
        Cout, kh, kw = int(self.weight.shape[0]), int(self.weight.shape[2]), int(self.weight.shape[3])
        y2 = _fused.ops.float_conv2d(None, self.weight.detach(), "raw", self.bias.detach() if self.bias is not None else None,
                                     self.stride, self.padding, self.dilation, weight_triples=_fused.loglin_conv_weight_plane(self, 1),
                                     pixels=act.planes, in_shape=act.shape)
        Ho, Wo = _fused.ops.conv_out_hw(H, W, kh, kw, self.stride, self.padding, self.dilation)
        y = y2.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2)
        return y if act.channels_last else y.contiguous()
