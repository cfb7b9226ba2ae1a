"""The dispatch body shared by the two sign families, Binary (binary_layers.py) and Ternary (terner_layers.py).

A family's Linear / Conv2d class derives from ``_SignLinear`` / ``_SignConv2d`` and sets only what differs: ``kind`` ("binary" /
"ternary"), ``_set_op`` / ``_op`` (its quantiser Function pair, kept in the instance attribute ``bin_op`` / ``ter_op``) and
``_weight_on_grid``.
"""
from math import sqrt as _sqrt

import torch

from ..functions import _fused
from .. import lazy
from .common import QLayer, EvalSwapMixin
from ..packed import PackedActivation as _PackedActivation


class _SignLinear(EvalSwapMixin, torch.nn.Linear, QLayer):
    kind = None

    def __init__(self, in_features, out_features, bias=True, deterministic=True):
        torch.nn.Linear.__init__(self, in_features, out_features, bias=bias)
        self.deterministic = deterministic
        self._set_op(deterministic)
        self.binary_input = None

    def reset_parameters(self):
        self.weight.data.normal_(0, _sqrt(1. / self.in_features))
        if self.bias is not None:
            self.bias.data.zero_()

    def clamp(self):
        self.weight.data.clamp_(-1, 1)
        if self.bias is not None:  # upstream clamps the bias as well (binary_layers.py:27-28)
            self.bias.data.clamp_(-1, 1)

    def _quantized_weight_for_eval(self):
        return self._op.apply(self.weight)

    def forward(self, input):
        return lazy.linear_forward(self, input, self.kind)

    def _forward_impl(self, input):
        if isinstance(input, _PackedActivation):
            return _fused.packed_linear(self, input, self.kind)
        if _fused.half_route(input, self.weight):
            y = self._half_forward(input)         # bf16 / fp16 activation that is (treated as) +-1: the packed routes
            if y is not None:
                return y
        if not input.is_cuda or input.dtype != torch.float32 or self.weight.dtype != torch.float32:
            # host tensors, and device models in half / bfloat16 / double: the reference expression in torch
            _fused.note_library_path(input, "non-fp32 dtype")
            w = self._op.apply(self.weight) if self.training else self.weight
            return torch.nn.functional.linear(input, w, self.bias)
        if self.training:
            wq = None if self.deterministic else self._op.apply(self.weight.detach())
            wp = self._train_planes(input)
            if wp is not None:      # the plane the fused optimiser step wrote next to the weight: the activation is packed alone
                return _fused.QuantLinearFn.apply(input, self.weight, self.bias, self.kind, wq, self.binary_input, wp)
            return _fused.QuantLinearFn.apply(input, self.weight, self.bias, self.kind, wq, self.binary_input)
        # eval: weight already holds the quantised image; planes are cached
        return self._eval_forward(input)

    def _train_planes(self, input):
        """The nibble plane of Q(weight) recorded by a fused optimiser step (utils/optim.py: ``weight._qt_train_planes``), when it
        still describes the weight — same version counter and storage — and this call would pack the weight for the matrix-core
        GEMM; else None.  Writes through ``weight.data`` do not bump the version counter (the hazard documented for the eval
        cache: ``reset_quant_cache()`` after one); the layer's own ``clamp()`` through ``.data`` cannot change a sign or ternary
        code and the fused step has already applied it.  A forward that is being CAPTURED bakes the buffer's address into the graph:
        it takes the plane only inside the capture that also captures the update rewriting that buffer
        (``_fused.plane_capture_scope``, utils/optim.py:capturing), never otherwise."""
        w = self.weight
        rec = getattr(w, "_qt_train_planes", None)
        if rec is None or not self.deterministic:
            return None
        if rec["version"] != w._version or rec["ptr"] != w.data_ptr():
            return None
        K, N = input.shape[-1], w.shape[0]
        if _fused.ops.select_gemm_impl(_fused._cfg("GEMM_IMPL"), input.numel() // max(K, 1), N, K) != "mfma":
            return None
        if torch.cuda.is_current_stream_capturing() and not _fused.plane_capture_allows(rec["mfma"].words):
            return None
        return rec["mfma"]

    def _half_forward(self, input):
        """bf16 / fp16 device activation (``_fused.half_route``): the packed routes when it is tagged, hinted or detected as +-1 —
        result in the activation's dtype, the exact sum + bias rounded once — else None (real-valued half activations and
        off-grid eval weights keep the counted torch expression below)."""
        from ..packed import ROWS_LAST
        kind = self.kind
        pm1 = _fused.half_gate(input, self.weight, self.binary_input, ROWS_LAST)     # True, or the device flag of a remembered verdict
        if pm1 is False:
            return None
        if self.training:
            wq = None if self.deterministic else self._op.apply(self.weight.detach())
            return _fused.QuantLinearFn.apply(input, self.weight, self.bias, kind, wq, pm1)
        if not self._eval_on_grid():
            return None
        if _fused.autograd_records(input, self.weight):      # the training node on the stored image (see _eval_forward)
            return _fused.QuantLinearFn.apply(input, self.weight, self.bias, kind, self.weight.detach(), pm1)
        K, N = input.shape[-1], self.weight.shape[0]
        impl = _fused.ops.select_gemm_impl(_fused._cfg("GEMM_IMPL"), input.numel() // max(K, 1), N, K)
        hint, flag = _fused.split_hint(pm1)
        xp, _ = _fused.activation_planes(input, hint, impl, self.weight, half_ok=True)
        wp = self._eval_planes(lambda w2: _fused.pack_weight(w2, kind, impl), key=impl)
        bias = _fused.poison_bias(_fused.half_bias(self.bias, input.dtype), flag, N, input.device)
        return _fused.ops.packed_gemm(xp, wp, bias, impl=impl, out_dtype=input.dtype).view(*input.shape[:-1], N)

    def _eval_forward(self, input):
        """Eval-mode forward of a device layer: F.linear(input, weight, bias) (binary_layers.py:46) with the packed path when
        the activation is +-1."""
        kind = self.kind
        if _fused.autograd_records(input, self.weight):
            # eval-mode forward with autograd on (model.eval(); model(x) without no_grad: the parameters require grad).  The
            # reference expression is F.linear on the stored image; on the quantiser's grid that is the training node with the
            # image as the pre-quantised weight — own kernels forward and backward, and its STE mask 1[|W| <= 1.001] is all ones
            # on an image in {0, +-1}, so the gradients are those of F.linear (this route used to be the dense
            # library, uncounted)
            if self._eval_on_grid():
                return _fused.QuantLinearFn.apply(input, self.weight, self.bias, kind, self.weight.detach(), self.binary_input)
            _fused.note_library_path(input, "eval-mode forward under autograd, weight off the quantiser's grid")
            return torch.nn.functional.linear(input, self.weight, self.bias)
        if not self._eval_on_grid():
            # the weight was overwritten with something that is not a quantised image (e.g. a float checkpoint loaded
            # after .eval()): upstream multiplies by whatever `weight` holds, so does this
            _fused.note_library_path(input, "eval-mode weight off the quantiser's grid")
            return torch.nn.functional.linear(input, self.weight, self.bias)
        K, N = input.shape[-1], self.weight.shape[0]
        impl = _fused.ops.select_gemm_impl(_fused._cfg("GEMM_IMPL"), input.numel() // max(K, 1), N, K)
        xp, flag = _fused.activation_planes(input, self.binary_input, impl, self.weight)
        if xp is None:
            if _fused._cfg("FLOAT_PATH") == "bf16x3" and input.dtype == torch.float32 and input.numel() > 0:
                wt = self._eval_planes(lambda w2: _fused.ops.weight_bf16x3(w2, kind), key="bf16x3")
                return _fused.ops.float_linear(input, self.weight, kind, self.bias, weight_triples=wt)
            _fused.note_library_path(input, "eval-mode linear on a real-valued activation with the float route switched off")
            return torch.nn.functional.linear(input, self.weight, self.bias)
        wp = self._eval_planes(lambda w2: _fused.pack_weight(w2, kind, impl), key=impl)
        y = _fused.ops.packed_gemm(xp, wp, _fused.poison_bias(self.bias, flag, N, input.device), impl=impl)
        return y.view(*input.shape[:-1], N)


class _SignConv2d(EvalSwapMixin, torch.nn.Conv2d, QLayer):
    kind = None

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, deterministic=True):
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride,
                                 padding=padding, dilation=dilation, groups=groups, bias=bias)
        self.deterministic = deterministic
        self._set_op(deterministic)
        self.binary_input = None

    def clamp(self):
        """Clamp the real weight to [-1, 1] (bias untouched, binary_layers.py:81-85)."""
        self.weight.data.clamp_(-1, 1)

    def _quantized_weight_for_eval(self):
        return self._op.apply(self.weight)

    def _conv_triples(self, form, terms=None):
        """Cached operand of the eval-mode (already quantised) weight for rung ``form`` of the first-layer ladder on real-valued
        inputs (_fused.first_layer_weight_planes); the split images ('plain', 's2d', 'd2s') under ops.FLOAT_SPLIT or ``terms``."""
        key = form
        if form in ("plain", "s2d", "d2s"):
            terms = _fused.ops.split_terms(terms)
            key = f"conv_split{terms}" + ("" if form == "plain" else "_" + form)
        return self._eval_planes(lambda _w2: _fused.first_layer_weight_planes(form, self.weight.detach(), self.kind, self.stride[0], terms),
                                 key=key)

    def _half_forward(self, input):
        """bf16 / fp16 device activation (``_fused.half_route``) that is tagged, hinted or detected as +-1: the implicit-GEMM conv
        on fp4 planes with the result in the activation's dtype (the exact sum + bias rounded once); None for everything the
        packed conv does not take (real-valued activations, grouped convs, non-zero padding modes, off-grid eval weights): a grouped
        conv goes on to ``_streaming_half_forward``, the rest keeps the counted torch expression below.  Never deferred: the modules between the layers stay torch ops in half."""
        from ..packed import NHWC
        if self.groups != 1 or self.padding_mode != "zeros" or input.dim() != 4 or isinstance(self.padding, str):
            return None
        kind = self.kind
        args = (self.stride, self.padding, self.dilation, self.groups)
        pm1 = _fused.half_gate(input, self.weight, self.binary_input, NHWC)          # True, or the device flag of a remembered verdict
        if pm1 is False:
            return None
        if self.training:
            wq = None if self.deterministic else self._op.apply(self.weight.detach())
            return _fused.QuantConv2dFn.apply(input, self.weight, self.bias, kind, wq, pm1, args)
        if not self._eval_on_grid():
            return None
        if _fused.autograd_records(input, self.weight):
            return _fused.QuantConv2dFn.apply(input, self.weight, self.bias, kind, self.weight.detach(), pm1, args)
        wp = self._eval_planes(lambda _w2: _fused.ops.pack_conv_weight_nib(self.weight.detach(), kind), key="conv_nib")
        return _fused.quant_conv2d_forward(input, self.weight, self.bias, *args, kind, weight_q=self.weight, weight_planes=wp,
                                           binary_input=pm1, padding_mode=self.padding_mode, half_ok=True)

    def _streaming_forward(self, input):
        """``groups == in_channels`` (``_fused.depthwise_route``) or at least ``_fused.GROUPED_MIN_GROUPS`` groups of a few input
        channels (``_fused.grouped_route``) on a device fp32 input: the depthwise / grouped kernels, which quantise the taps
        themselves — training with the layer's quantiser and its STE mask (a stochastic layer draws once for the whole weight and
        hands the draw over), eval on the stored image; None for everything else, an off-grid eval weight included (it keeps the
        counted library expression)."""
        if _fused.depthwise_route(self, input):
            fn = _fused.DepthwiseConv2dFn
        elif _fused.grouped_route(self, input):
            fn = _fused.GroupedConv2dFn
        else:
            return None
        args = (self.stride, self.padding, self.dilation, self.groups)
        if self.training:
            wq = None if self.deterministic else self._op.apply(self.weight.detach())
            return fn.apply(input, self.weight, self.bias, self.kind, wq, _fused.ops.STE_THRESHOLD, args)
        if not self._eval_on_grid():
            return None
        return fn.apply(input, self.weight, self.bias, "raw", self.weight.detach(), _fused.ops.STE_THRESHOLD, args)

    def _streaming_half_forward(self, input):
        """``_streaming_forward`` for a bf16 / fp16 activation (``_fused.depthwise_half_route`` / ``grouped_half_route``): the same
        autograd nodes on the "_h" entries — results rounded once into the activation's dtype, the weight gradient in the weight's
        dtype.  Real-valued activations take it too (nothing asks for +-1); never deferred.  None: the counted library expression."""
        if _fused.depthwise_half_route(self, input):
            fn, fam = _fused.DepthwiseConv2dFn, "depthwise"
        elif _fused.grouped_half_route(self, input):
            fn, fam = _fused.GroupedConv2dFn, "grouped"
        else:
            return None
        args = (self.stride, self.padding, self.dilation, self.groups)
        if self.training:
            wq = None if self.deterministic else self._op.apply(self.weight.detach())
            y = fn.apply(input, self.weight, self.bias, self.kind, wq, _fused.ops.STE_THRESHOLD, args)
        elif not self._eval_on_grid():
            return None
        else:
            y = fn.apply(input, self.weight, self.bias, "raw", self.weight.detach(), _fused.ops.STE_THRESHOLD, args)
        _fused.STREAMING_HALF_STATS[fam] += 1
        return y

    def forward(self, input):
        """Eval mode without autograd on a HIP device: returns a deferred activation (``lazy.LazyActivation``: a Tensor
        that runs this conv fused with the BatchNorm / pooling / Hardtanh / BinaryConnect modules that follow it, or
        computes the plain fp32 result on any other use); every other case computes right here."""
        return lazy.conv_forward(self, input, self.kind)

    def _forward_impl(self, input):
        kind = self.kind
        if isinstance(input, _PackedActivation):
            if 1 < self.groups < self.in_channels:      # a deferred grouped conv on planes that materialises
                return _fused.packed_grouped_conv2d(self, input)
            if self.groups != 1:            # groups == in_channels on planes: a deferred depthwise conv that materialises
                return _fused.packed_depthwise_conv2d(self, input)
            return _fused.packed_conv2d(self, input, kind)
        if _fused.half_route(input, self.weight):
            y = self._half_forward(input)         # bf16 / fp16 activation that is (treated as) +-1: the packed routes
            if y is None and self.groups > 1:
                y = self._streaming_half_forward(input)       # depthwise / few channels per group: the "_h" streaming kernels
            if y is not None:
                return y
        if not input.is_cuda or input.dtype != torch.float32 or self.weight.dtype != torch.float32:
            _fused.note_library_path(input, "non-fp32 dtype")
            w = self._op.apply(self.weight) if self.training else self.weight
            return torch.nn.functional.conv2d(input, w, self.bias, self.stride, self.padding,
                                              self.dilation, self.groups)
        if self.groups > 1 and self.padding_mode == "zeros" and input.dim() == 4 and not isinstance(self.padding, str):
            y = self._streaming_forward(input)                             # depthwise / few channels per group: one streaming launch
            if y is None:
                y = _fused.grouped_quant_conv(self, input, kind, self._op)     # every group on the groups == 1 routes
            if y is not None:
                return y
        args = (self.stride, self.padding, self.dilation, self.groups)
        if self.training:
            wq = None if self.deterministic else self._op.apply(self.weight.detach())
            return _fused.QuantConv2dFn.apply(input, self.weight, self.bias, kind, wq, self.binary_input, args)
        # eval: weight already holds the quantised image; its packed planes are cached
        if _fused.autograd_records(input, self.weight):
            # eval-mode forward under autograd: the training node on the stored image (see _SignLinear._eval_forward)
            if self.padding_mode == "zeros" and not isinstance(self.padding, str) and self._eval_on_grid():
                return _fused.QuantConv2dFn.apply(input, self.weight, self.bias, kind, self.weight.detach(),
                                                  self.binary_input, args)
            _fused.note_library_path(input, "eval-mode conv forward under autograd (off-grid weight / non-zero padding mode)")
            return torch.nn.functional.conv2d(input, self.weight, self.bias, *args)
        if not self._eval_on_grid():
            _fused.note_library_path(input, "eval-mode weight off the quantiser's grid")
            return torch.nn.functional.conv2d(input, self.weight, self.bias, *args)
        wp = None
        if self.groups == 1 and self.padding_mode == "zeros":
            wp = self._eval_planes(lambda _w2: _fused.ops.pack_conv_weight_nib(self.weight.detach(), kind), key="conv_nib")
        return _fused.quant_conv2d_forward(input, self.weight, self.bias, *args, kind,
                                           weight_q=self.weight, weight_planes=wp,
                                           binary_input=self.binary_input, padding_mode=self.padding_mode,
                                           weight_triples_fn=self._conv_triples)
