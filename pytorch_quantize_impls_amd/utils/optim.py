"""``optimizer.step()`` followed by ``model.clamp()`` — how every training loop of the reference ends a step (train/train.py:90-96,
benchmark/BinaryNet/mnist.py:42-44) — as ONE multi-tensor launch sequence per parameter group (csrc/optim_step.hip).

``FusedQuantSGD`` / ``FusedQuantAdam`` are ``torch.optim.Optimizer`` subclasses with the recurrences, the state keys and the
``state_dict()`` layout of ``torch.optim.SGD`` / ``torch.optim.Adam``.  Given the model instead of its parameters they also
fold the layers' ``clamp()`` into the update (``clamp_plan``) and, for deterministic ``LinearBin`` / ``LinearTer``, leave the fp4
nibble plane of the new weight where the next training forward finds it (``weight._qt_train_planes``), so that forward does
not read the fp32 weight again only to take its sign.
"""
import functools
from typing import Dict, Tuple

import torch
from torch.optim.adam import adam as _adam
from torch.optim.optimizer import Optimizer, _get_scalar_dtype
from torch.optim.sgd import sgd as _sgd

from .. import ops
from ..functions import _fused


def _clamp_sign_linear(m):
    return [(m.weight, -1.0, 1.0)] + ([(m.bias, -1.0, 1.0)] if m.bias is not None else [])


def _clamp_sign_conv(m):
    return [(m.weight, -1.0, 1.0)]


def _clamp_log_lin(m):
    return [(m.weight, float(-1 * 2 ** m.fsr), float(2 ** m.fsr))]


def _clamp_loss_quant(m):
    lo, hi = (float(v) for v in m._range())
    return [(m.weight, lo, hi)] + ([(m.bias, lo, hi)] if m.bias is not None else [])


@functools.lru_cache(maxsize=None)
def _known_clamps():
    """The clamp() implementations this module can restate as a (lo, hi) per parameter: keyed on the FUNCTION a class resolves
    ``clamp`` to, so a subclass that overrides clamp() is not mistaken for its base.  (Built on first use: the layer modules
    import this package.)"""
    from ..layers.sign_layers import _SignLinear, _SignConv2d
    from ..layers.log_lin_layers import _WeightInit
    from ..layers.elastic_layers import LossQuantMixin
    from ..layers.xnor_layers import XNORConv2d
    return {
        _SignLinear.clamp: _clamp_sign_linear,
        _SignConv2d.clamp: _clamp_sign_conv,
        _WeightInit.clamp: _clamp_log_lin,
        LossQuantMixin.clamp: _clamp_loss_quant,
        XNORConv2d.clamp: lambda m: [],
    }


def _clamping_layers(module):
    """The layers ``utils.clamp_weights_`` calls ``clamp()`` on, in its order."""
    for m in module.modules():
        if isinstance(getattr(m, "weight", None), torch.nn.Parameter) and callable(getattr(m, "clamp", None)):
            yield m


def clamp_plan(module: torch.nn.Module) -> Dict[torch.nn.Parameter, Tuple[float, float]]:
    """{parameter: (lo, hi)}: what ``utils.clamp_weights_(module)`` does, stated per parameter.  Derived from the layers exactly
    as their ``clamp()`` methods act: LinearBin / LinearTer clamp weight and bias to +-1, the sign convs the weight only, the
    Lin / Log layers the weight to +-2^fsr, the Elastic / WQR layers weight and bias to their ``_range()``, the XNOR layers
    nothing.  A layer class this function does not know gets no entry (``unplanned_clamp_layers``).  Pure: nothing is
    modified."""
    plan: Dict[torch.nn.Parameter, Tuple[float, float]] = {}
    for m in _clamping_layers(module):
        fn = _known_clamps().get(getattr(type(m), "clamp", None))
        if fn is None:
            continue
        for p, lo, hi in fn(m):
            if p in plan:                  # a parameter shared by two layers: both clamps apply
                lo, hi = max(lo, plan[p][0]), min(hi, plan[p][1])
            plan[p] = (lo, hi)
    return plan


def unplanned_clamp_layers(module: torch.nn.Module):
    """Layers that define ``clamp()`` in a way ``clamp_plan`` cannot restate: their ``clamp()`` is called after the launch."""
    return [m for m in _clamping_layers(module) if getattr(type(m), "clamp", None) not in _known_clamps()]


def _on_route(p: torch.Tensor, g: torch.Tensor, *state) -> bool:
    """The kernel's route: contiguous fp32 device tensors, dense gradient."""
    if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
        return False
    if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous():
        return False
    return all(s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.device == p.device for s in state)


class _FusedQuantOptimizer(Optimizer):
    def __init__(self, params, defaults, clamp, emit_planes):
        module = params if isinstance(params, torch.nn.Module) else None
        if module is not None:
            params = list(module.parameters())
        super().__init__(params, defaults)
        self._clamp_plan = clamp_plan(module) if module is not None and (clamp is None or clamp) else {}
        self._post_clamp = unplanned_clamp_layers(module) if module is not None and (clamp is None or clamp) else []
        self._plane_layers = {}
        if module is not None and (emit_planes is None or emit_planes):
            from ..layers.sign_layers import _SignLinear
            self._plane_layers = {m.weight: m for m in module.modules() if isinstance(m, _SignLinear)}
        self._plane_words = {}

    def _plane_of(self, p):
        """(NibPlanes, kind) of the persistent plane buffer of a deterministic LinearBin / LinearTer weight, else None."""
        layer = self._plane_layers.get(p)
        if layer is None or not layer.deterministic or p.dim() != 2:
            return None
        N, K = int(p.shape[0]), int(p.shape[1])
        words = self._plane_words.get(p)
        if words is None or words.device != p.device or tuple(words.shape) != (N, ops.packed_ld_nib(K)):
            words = self._plane_words[p] = torch.empty((N, ops.packed_ld_nib(K)), dtype=torch.int32, device=p.device)
        return ops.NibPlanes(words=words, rows=N, K=K), layer.kind

    def _record(self, fused_params, planes):
        """After a launch: bump the version counters (eval caches, implicit graphs and auto_graphed key on them) and record the
        planes under the new version."""
        torch.autograd.graph.increment_version(fused_params)
        for p, pl in zip(fused_params, planes):
            if pl is not None:
                p._qt_train_planes = {"version": p._version, "ptr": p.data_ptr(), "mfma": pl[0]}

    def _finish(self, library_params):
        """The clamps that were not folded into a launch: parameters off the kernel's route, layers ``clamp_plan`` does not know."""
        for p in library_params:
            rng = self._clamp_plan.get(p)
            if rng is not None:
                p.data.clamp_(*rng)
        for m in self._post_clamp:
            m.clamp()

    def _split(self, group, state_keys):
        """Parameters of ``group`` that have a gradient, as {device: [p, ...]} on the kernel's route and [p, ...] off it."""
        fused, library = {}, []
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            st = self.state.get(p) or {}
            if _on_route(p, g, *(st[k] for k in state_keys if st.get(k) is not None)):
                fused.setdefault(p.device, []).append(p)
            else:
                _fused.note_library_path(p, "optimiser step: parameter off the fused kernel's route")
                library.append(p)
        return fused, library


def _reject(name, **options):
    for k, v in options.items():
        if v:
            raise NotImplementedError(f"{name}: {k}={v!r} is not implemented (use torch.optim for it)")


class FusedQuantSGD(_FusedQuantOptimizer):
    """``torch.optim.SGD`` (momentum, L2 weight decay, nesterov; dampening 0) + ``model.clamp()`` + weight planes in one launch
    sequence per parameter group.

    ``params``: an ``nn.Module`` (clamp and planes available) or an iterable of parameters / param groups (plain update).
    ``clamp`` / ``emit_planes``: default on when a module is given.  Parameters off the kernel's route (host tensors, non-fp32,
    non-contiguous, sparse gradient) take ``torch.optim``'s functional ``sgd`` in the same ``step()``, followed by their
    clamp; they are counted in ``_fused.LIBRARY_PATHS``."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, clamp=None, emit_planes=None):
        _reject("FusedQuantSGD", maximize=maximize, dampening=dampening != 0, differentiable=differentiable, foreach=foreach,
                fused=fused)
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedQuantSGD: negative lr / momentum / weight_decay")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, clamp, emit_planes)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        off_route = []
        for group in self.param_groups:
            _reject("FusedQuantSGD", maximize=group["maximize"], dampening=group["dampening"] != 0)
            lr, mu, wd, nesterov = group["lr"], group["momentum"], group["weight_decay"], group["nesterov"]
            fused, library = self._split(group, ("momentum_buffer",))
            for plist in fused.values():
                bufs, first = None, None
                if mu != 0:
                    bufs, first = [], []
                    for p in plist:
                        st = self.state[p]
                        buf = st.get("momentum_buffer")
                        first.append(buf is None)
                        if buf is None:
                            buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        bufs.append(buf)
                planes = [self._plane_of(p) for p in plist]
                ops.optim_step_sgd(plist, [p.grad for p in plist], bufs, lr=lr, momentum=mu, weight_decay=wd, nesterov=nesterov,
                                   first=first, clamps=[self._clamp_plan.get(p) for p in plist], planes=planes)
                self._record(plist, planes)
            if library:
                bufs = [self.state[p].get("momentum_buffer") for p in library]
                _sgd(library, [p.grad for p in library], bufs, has_sparse_grad=any(p.grad.is_sparse for p in library),
                                    foreach=False, fused=False, weight_decay=wd, momentum=mu, lr=lr, dampening=0.0,
                                    nesterov=nesterov, maximize=False)
                if mu != 0:
                    for p, buf in zip(library, bufs):
                        self.state[p]["momentum_buffer"] = buf
            off_route += library
        self._finish(off_route)
        return loss


class FusedQuantAdam(_FusedQuantOptimizer):
    """``torch.optim.Adam`` (betas, eps, L2 weight decay; no amsgrad) + ``model.clamp()`` + weight planes in one launch sequence
    per parameter group.  Arguments and the handling of parameters off the kernel's route as in ``FusedQuantSGD``; ``step`` is
    kept per parameter as torch keeps it (a host scalar tensor) and the bias corrections are computed from it every step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, clamp=None,
                 emit_planes=None):
        _reject("FusedQuantAdam", amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable,
                foreach=foreach, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedQuantAdam: a tensor lr is not implemented")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedQuantAdam: lr / eps / weight_decay negative or a beta outside [0, 1)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults, clamp, emit_planes)

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        off_route = []
        for group in self.param_groups:
            _reject("FusedQuantAdam", amsgrad=group["amsgrad"], maximize=group["maximize"], capturable=group["capturable"],
                    decoupled_weight_decay=group.get("decoupled_weight_decay", False))
            lr, betas, eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is not None:
                    self._init_state(p)
            fused, library = self._split(group, ("exp_avg", "exp_avg_sq"))
            for plist in fused.values():
                states = [self.state[p] for p in plist]
                steps = []
                for st in states:
                    st["step"] += 1
                    steps.append(int(st["step"]))
                planes = [self._plane_of(p) for p in plist]
                ops.optim_step_adam(plist, [p.grad for p in plist], [st["exp_avg"] for st in states],
                                    [st["exp_avg_sq"] for st in states], steps, lr=lr, betas=betas, eps=eps, weight_decay=wd,
                                    clamps=[self._clamp_plan.get(p) for p in plist], planes=planes)
                self._record(plist, planes)
            if library:
                states = [self.state[p] for p in library]
                _adam(library, [p.grad for p in library], [st["exp_avg"] for st in states],
                                      [st["exp_avg_sq"] for st in states], [], [st["step"] for st in states], foreach=False,
                                      capturable=False, differentiable=False, fused=False,
                                      has_complex=any(torch.is_complex(p) for p in library), amsgrad=False, beta1=betas[0],
                                      beta2=betas[1], lr=lr, weight_decay=wd, eps=eps, maximize=False)
            off_route += library
        self._finish(off_route)
        return loss
