"""``optimizer.step()`` followed by ``model.clamp()`` — how every training loop of the reference ends a step (train/train.py:90-96,
benchmark/BinaryNet/mnist.py:42-44) — as ONE multi-tensor launch sequence per parameter group (csrc/optim_step.hip).

``FusedQuantSGD`` / ``FusedQuantAdam`` are ``torch.optim.Optimizer`` subclasses with the recurrences, the state keys and the
``state_dict()`` layout of ``torch.optim.SGD`` / ``torch.optim.Adam``.  Given the model instead of its parameters they also
fold the layers' ``clamp()`` into the update (``clamp_plan``) and, for deterministic ``LinearBin`` / ``LinearTer``, leave the fp4
nibble plane of the new weight where the next training forward finds it (``weight._qt_train_planes``), so that forward does
not read the fp32 weight again only to take its sign.

Capture mode (``prepare_capture`` / ``captured_step`` / ``before_replay`` / ``after_replay`` / ``cancel_replay``) is what ``utils.GraphedTrainStep``
uses to put the update inside its hipGraph: the launches read the per-step scalars (learning rate, Adam's bias corrections)
from a device block the host rewrites before every replay, everything else is baked into the captured launches.

``max_grad_norm=``: ``torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)`` folded into the step — one sum-of-squares pass
over the gradients, one finalise launch, and the update multiplies each gradient by the coefficient as it reads it.  ``p.grad``
stays UNSCALED on that path; ``opt.grad_norm`` / ``opt.clip_coef`` hold the step's norm and coefficient on the device.
"""
import functools
import math
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


class _CapturedGroup:
    """What one parameter group contributes to a captured step: the parameters that had a gradient at capture time, their state
    tensors, clamp ranges and planes, the slice of the scalar block its launches read and the hyper-parameters baked into them."""

    def __init__(self, index, params, baked):
        self.index, self.params, self.baked = index, params, baked     # index into param_groups (load_state_dict replaces the dicts)
        self.grads = [p.grad for p in params]
        self.pointers = [p.data_ptr() for p in params]
        self.scalars = None                        # view into the scalar block (set by prepare_capture)
        self.states = self.planes = self.clamps = self.steps = None
        self.offset = self.numel = 0


class _Capture:
    """One captured step of an optimiser: what ``prepare_capture()`` returns and ``captured_step`` / ``before_replay`` /
    ``after_replay`` / ``refresh_planes`` take.  It belongs to the graph that was captured with it (``utils.GraphedTrainStep`` keeps
    it), not to the optimiser: one optimiser may serve several graphs (a full and a tail batch shape), each with its own scalar
    block, all on the optimiser's one set of state tensors and plane buffers."""

    def __init__(self, groups, block, state_epoch):
        self.groups, self.block, self.state_epoch = groups, block, state_epoch
        # clipping (max_grad_norm at capture time): the device float the finalise launch reads max_norm from (the last slot of the
        # scalar block), the workspace of the sum-of-squares pass and the two words (norm, coef) it ends in; None = not captured
        self.max_norm = self.norm_work = self.norm_out = None


class _FusedQuantOptimizer(Optimizer):
    #: the group entries a captured launch takes by value: changing one after the capture cannot reach the graph
    _BAKED = ()
    #: the state tensors of a parameter, in the kernel's order
    _STATE_KEYS = ()

    def __init__(self, params, defaults, clamp, emit_planes, max_grad_norm=None):
        module = params if isinstance(params, torch.nn.Module) else None
        self._names = {}
        if module is not None:
            self._names = {p: n for n, p in module.named_parameters()}
            params = list(module.parameters())
        super().__init__(params, defaults)
        self._state_epoch = 0                      # load_state_dict() calls: each replaces every state tensor
        self._clamp_plan = clamp_plan(module) if module is not None and (clamp is None or clamp) else {}
        self._post_clamp = unplanned_clamp_layers(module) if module is not None and (clamp is None or clamp) else []
        self._plane_layers = {}
        if module is not None and (emit_planes is None or emit_planes):
            from ..layers.sign_layers import _SignLinear
            self._plane_layers = {m.weight: m for m in module.modules() if isinstance(m, _SignLinear)}
        self._plane_words = {}
        self.max_grad_norm = max_grad_norm         # an attribute of the optimiser, not a group entry: the norm is global
        self._clip_work = None                     # eager step(): workspace of the sum-of-squares pass, grown on demand
        self._clip_out = None                      # eager step(): (norm, coef)
        self._clip_last = None                     # the (norm, coef) words of the last clipped step, whichever path took it

    @property
    def max_grad_norm(self):
        """``max_norm`` of the ``torch.nn.utils.clip_grad_norm_`` folded into the step (L2 norm over every parameter of every
        group that has a gradient), or None: no clipping.  Assignable between steps, also between replays of a captured step
        (the value travels with the other per-step scalars); switching clipping on or off needs a new capture."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if value is not None:
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
                raise ValueError(f"{type(self).__name__}: max_grad_norm must be a positive finite number or None, got {value!r}")
            value = float(value)
        self._max_grad_norm = value

    @property
    def grad_norm(self):
        """0-dim fp32 tensor on the parameters' device: the global gradient norm of the last clipped step, before clipping (None
        before the first).  Reading its value is the caller's synchronise; the step has none."""
        return None if self._clip_last is None else self._clip_last[0]

    @property
    def clip_coef(self):
        """0-dim fp32 tensor: ``min(1, max_grad_norm / (grad_norm + 1e-6))`` of the last clipped step, what its gradients were
        multiplied by (None before the first)."""
        return None if self._clip_last is None else self._clip_last[1]

    def _clip(self):
        """The clipping part of an eager ``step()``.  Returns the one-element device tensor the update launches multiply the
        gradients by, or None when there is nothing left for them to do: no ``max_grad_norm``, no gradient, or — a parameter off
        the kernel's route, parameters on more than one device — ``torch.nn.utils.clip_grad_norm_`` over all parameters, which
        rewrites the gradients in place as torch does and is counted once in ``_fused.LIBRARY_PATHS``."""
        if self._max_grad_norm is None:
            return None
        params = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not params:
            return None
        off = None
        for p in params:
            st = self.state.get(p) or {}
            if not _on_route(p, p.grad, *(st[k] for k in self._STATE_KEYS if st.get(k) is not None)) or p.device != params[0].device:
                off = p
                break
        if off is not None:
            _fused.note_library_path(off, "optimiser step: clip_grad_norm_ (a parameter off the fused kernel's route)")
            norm = torch.nn.utils.clip_grad_norm_(params, self._max_grad_norm).detach().to(torch.float32)
            self._clip_last = torch.stack([norm, torch.clamp(self._max_grad_norm / (norm + 1e-6), max=1.0)])
            return None
        grads = [p.grad for p in params]
        device, m = params[0].device, sum((g.numel() + 4095) >> 12 for g in grads)      # one word per 4096-element unit
        if self._clip_out is None or self._clip_out.device != device:
            self._clip_out, self._clip_work = torch.zeros(2, dtype=torch.float32, device=device), None
        if self._clip_work is None or self._clip_work.numel() < m:
            self._clip_work = torch.empty(max(m, 1), dtype=torch.float32, device=device)
        ops.optim_grad_norm(grads, self._clip_work, self._clip_out, max_norm=self._max_grad_norm)
        self._clip_last = self._clip_out
        return self._clip_out[1:]

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
                self._stamp(p, pl)

    @staticmethod
    def _stamp(p, pl):
        p._qt_train_planes = {"version": p._version, "ptr": p.data_ptr(), "mfma": pl[0]}

    # ---- capture mode: the update as part of utils.GraphedTrainStep's hipGraph ----

    def _name(self, p):
        if p in self._names:
            return self._names[p]
        for gi, group in enumerate(self.param_groups):
            for i, q in enumerate(group["params"]):
                if q is p:
                    return f"param_groups[{gi}]['params'][{i}] {tuple(p.shape)}"
        return f"parameter {tuple(p.shape)}"

    def _check_group(self, group):                 # pragma: no cover - abstract
        raise NotImplementedError

    def _allocate(self, p, group):                 # pragma: no cover - abstract
        """Create the state of ``p`` if it has none; returns its state tensors in the kernel's order."""
        raise NotImplementedError

    def allocate_state(self):
        """The state of every parameter that has a gradient, created up front as zeros (``step``: the host scalar tensor torch
        keeps): a captured launch needs its pointers before the first step.  A zeroed state is the state before the first step —
        ``torch.optim`` steps from it as from none (Adam starts from zeros anyway; SGD's first ``buf = g`` becomes ``mu * 0 + g``,
        which differs only in turning a -0.0 gradient entry into +0.0 in the buffer).  Existing state is kept."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    self._allocate(p, group)

    def prepare_capture(self) -> _Capture:
        """Fix what a captured step updates — every parameter that has a gradient NOW, with its state allocated
        (``allocate_state``) — and allocate one device block for the per-step scalars of its launch sequences.  Returns the
        ``_Capture`` the other capture-mode methods take; every call makes a new one with a block of its own, and earlier ones stay
        valid.  With ``max_grad_norm`` set the block gains one slot for it, and the capture its own workspace and (norm, coef)
        words for the norm launches: allocated here, outside the stream capture.  A captured step has no library path: a parameter off the kernel's route (host, non-fp32, non-contiguous), a sparse
        gradient or parameters on more than one device raise ``ValueError`` naming the parameter."""
        self.allocate_state()
        groups, device, numel = [], None, 0
        for index, group in enumerate(self.param_groups):
            self._check_group(group)
            params = [p for p in group["params"] if p.grad is not None]
            for p in params:
                if p.grad.is_sparse:
                    raise ValueError(f"captured step: {self._name(p)} has a sparse gradient")
                if not _on_route(p, p.grad, *self._allocate(p, group)):
                    raise ValueError(f"captured step: {self._name(p)} ({p.dtype}, {p.device}, contiguous={p.is_contiguous()}) is off "
                                     "the fused kernel's route (contiguous fp32 device tensors) and a captured step has no library path")
                if device is not None and p.device != device:
                    raise ValueError(f"captured step: {self._name(p)} is on {p.device}, other parameters on {device}: one graph, one device")
                device = p.device
            if params:
                cg = _CapturedGroup(index, params, {k: group[k] for k in self._BAKED})
                cg.offset, cg.numel = numel, self._scalars_per_group(len(params))
                numel += cg.numel
                groups.append(cg)
        # ONE block for the scalars of all groups.  before_replay() rewrites it with a launch that carries the values in its argument
        # block (ops.optim_write_scalars): stream-ordered between the previous replay and the next, no synchronise, and no host
        # staging buffer an earlier, still pending write could be reading — the runtime copies the arguments at enqueue time.
        clip = groups and self._max_grad_norm is not None
        block = torch.zeros(numel + (1 if clip else 0), dtype=torch.float32, device=device) if groups else None
        for cg in groups:
            cg.scalars = block[cg.offset:cg.offset + cg.numel]
            cg.states = [self._allocate(p, self.param_groups[cg.index]) for p in cg.params]
            cg.steps = [self.state[p]["step"] for p in cg.params if "step" in self.state[p]]
            cg.planes = [self._plane_of(p) for p in cg.params]
            cg.clamps = [self._clamp_plan.get(p) for p in cg.params]
        capture = _Capture(groups, block, self._state_epoch)
        if clip:
            m = ops.optim_grad_norm_work_floats([g for cg in groups for g in cg.grads])
            capture.max_norm = block[numel:]
            capture.norm_work = torch.empty(max(m, 1), dtype=torch.float32, device=device)
            capture.norm_out = torch.zeros(2, dtype=torch.float32, device=device)
        return capture

    def load_state_dict(self, state_dict):
        """``Optimizer.load_state_dict``.  It replaces every state tensor, so captured steps of this optimiser would go on updating
        the old ones: their next ``before_replay`` raises (load the state first, then capture)."""
        super().load_state_dict(state_dict)
        self._state_epoch += 1

    def capturing(self, capture: _Capture):
        """Context for the warm-up and the stream capture of ``capture``'s graph: inside it (and nowhere else) the training forward of
        a LinearBin / LinearTer may take ``capture``'s plane buffers while the stream is capturing — the graph's own update rewrites
        them on every replay and ``before_replay`` repacks a stale one.  Any other capture still gets no plane."""
        return _fused.plane_capture_scope([pl[0].words for cg in capture.groups for pl in cg.planes if pl is not None])

    def refresh_planes(self, capture: _Capture):
        """The invariant a captured forward relies on: the persistent plane buffer of every captured deterministic LinearBin /
        LinearTer weight holds the plane of the weight AS IT IS NOW, recorded under its current version counter and storage.  The
        captured step keeps it (it rewrites the buffer with every update, ``after_replay`` re-stamps the record), and so does an
        eager ``step()`` of this optimiser (same buffers); whatever else writes the weight — ``load_state_dict``, an in-place edit,
        ``eval()`` / ``train()``, another optimiser — moves the version counter or drops the record, and the plane is packed again
        here, eagerly, from the weight alone.  Returns the number of planes packed.  (Writes through ``.data`` are invisible, as
        they are to the eval cache.)"""
        packed = 0
        for cg in capture.groups:
            for p, pl in zip(cg.params, cg.planes):
                if pl is None:
                    continue
                rec = getattr(p, "_qt_train_planes", None)
                if rec is not None and rec["mfma"].words is pl[0].words and rec["version"] == p._version and rec["ptr"] == p.data_ptr():
                    continue
                with torch.no_grad():
                    ops.pack_weight_nib_into(p.detach(), pl[1], pl[0])
                self._stamp(p, pl)
                packed += 1
        return packed

    def _launch_captured(self, cg, skip=None, gscale=None):     # pragma: no cover - abstract
        raise NotImplementedError

    @staticmethod
    def _scalars_per_group(n):                     # pragma: no cover - abstract
        """fp32 scalars the launches of a group of ``n`` captured parameters read."""
        raise NotImplementedError

    @torch.no_grad()
    def captured_step(self, capture: _Capture, skip=None):
        """The update of every captured parameter on the current stream, with the clamps and planes of ``step()`` — the launches a
        stream capture records.  Nothing on the host changes: ``before_replay`` / ``after_replay`` do what ``step()`` does there.
        ``skip``: one int32 device element the launches read when they RUN (the guarded entries, ``ops.optim_step_*_dev(skip=)``):
        non-zero and the step leaves parameters, state and planes as they are — ``cancel_replay`` is its host side.  A capture
        with clipping enqueues the norm launches over the gradients of ALL its groups first; they write the capture's own
        workspace and (norm, coef) words and nothing else, so a skipped step still leaves parameters, state and planes alone."""
        if skip is not None and self._post_clamp:
            # their clamp() is arbitrary torch code: nothing here could make it depend on a device word
            raise ValueError(f"{type(self).__name__}: a guarded captured step cannot skip the clamp() of "
                             f"{sorted({type(m).__name__ for m in self._post_clamp})}, which clamp_plan cannot restate")
        gscale = None
        if capture.norm_out is not None:
            ops.optim_grad_norm([g for cg in capture.groups for g in cg.grads], capture.norm_work, capture.norm_out,
                                max_norm_dev=capture.max_norm)
            gscale = capture.norm_out[1:]
        for cg in capture.groups:
            self._launch_captured(cg, skip, gscale)
        for m in self._post_clamp:                 # clamp() of layers clamp_plan cannot restate: torch ops, captured as well
            m.clamp()

    def _scalars_of(self, cg):                     # pragma: no cover - abstract
        """The fp32 scalars of ``cg``'s launches for the step about to run, from the group's CURRENT entries and, for Adam, the
        step counts ``state["step"] + 1``.  Changes nothing."""
        raise NotImplementedError

    def before_replay(self, capture: _Capture):
        """Host side of a replay, before it: checks that nothing baked into the captured launches was changed, restores the plane
        invariant (``refresh_planes``), computes the step's scalars from the current ``param_groups`` (LR schedulers, manual
        ``group['lr']`` edits) and sends them to ``capture``'s device block (``ops.optim_write_scalars``: a launch, no synchronise).
        The step counts advance last, once nothing can fail any more."""
        if capture.state_epoch != self._state_epoch:
            raise RuntimeError(f"{type(self).__name__}: load_state_dict() replaced the state tensors since the step was captured; the "
                               "graph still updates the old ones — load the state first, then capture a new GraphedTrainStep")
        if capture.groups and (self._max_grad_norm is not None) != (capture.norm_out is not None):
            was, now = ("on", "off") if self._max_grad_norm is None else ("off", "on")
            raise RuntimeError(f"{type(self).__name__}: gradient clipping was {was} when the step was captured and is {now} now "
                               f"(max_grad_norm={self._max_grad_norm!r}); its launches are baked into the graph — capture a new "
                               "GraphedTrainStep (a change of the VALUE reaches the replay)")
        for cg in capture.groups:
            group = self.param_groups[cg.index]
            self._check_group(group)
            for k, v in cg.baked.items():
                now = group[k]
                if (tuple(now) if isinstance(now, (list, tuple)) else now) != (tuple(v) if isinstance(v, (list, tuple)) else v):
                    raise RuntimeError(f"{type(self).__name__}: {k} was {v!r} when the step was captured and is {now!r} now; it is "
                                       "baked into the captured launches — capture a new GraphedTrainStep")
            for p, g, ptr in zip(cg.params, cg.grads, cg.pointers):
                if p.grad is not g or p.data_ptr() != ptr:
                    raise RuntimeError(f"{type(self).__name__}: {self._name(p)} or its gradient was replaced since the step was captured "
                                       "(zero_grad(set_to_none=True), .to(), an assignment to .grad / .data); the graph still works on the "
                                       "old storage — keep the gradients (they are zeroed inside the graph) or capture a new "
                                       "GraphedTrainStep")
        self.refresh_planes(capture)
        values = []
        for cg in capture.groups:
            values += self._scalars_of(cg)
        if capture.norm_out is not None:
            values.append(self._max_grad_norm)     # the block's last slot
        if capture.block is not None:
            ops.optim_write_scalars(capture.block, values)
        for cg in capture.groups:
            if cg.steps:
                torch._foreach_add_(cg.steps, 1)   # state["step"] as torch keeps it (host scalar tensors): one call for all

    def cancel_replay(self, capture: _Capture):
        """Host side of a replay whose guarded update the device SKIPPED (``captured_step(skip=)`` with the guard raised): takes
        back what ``before_replay`` / ``after_replay`` did for a step that did not happen.  That is Adam's ``state["step"]``, back
        by one.  The rest stands: the scalar block is rewritten before the next replay; the version counters moved, which only
        costs caches keyed on them a rebuild; and the plane records ``after_replay`` stamped under the new versions name buffers
        the skipped launches did not write, so they still hold the planes of the (unchanged) weights.  No device tensor is
        touched."""
        for cg in capture.groups:
            if cg.steps:
                torch._foreach_sub_(cg.steps, 1)   # host scalar tensors, as in before_replay

    def after_replay(self, capture: _Capture):
        """Host side of a replay, after it: what ``step()`` does after its launches (version counters, plane records)."""
        for cg in capture.groups:
            self._record(cg.params, cg.planes)
        if capture.norm_out is not None:
            self._clip_last = capture.norm_out
        if hasattr(self.step, "_wrapped_by_lr_sched"):
            # torch/optim/lr_scheduler.py (LRScheduler.__init__, patch_track_step_called) wraps step() to set this flag and warns
            # "lr_scheduler.step() before optimizer.step()" while it is unset; a replay IS a step.  Without that wrapper: nothing to do.
            self._opt_called = True

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
    clamp; they are counted in ``_fused.LIBRARY_PATHS``.

    ``max_grad_norm``: positive and finite, or None (default, no clipping).  The step then clips the global L2 gradient norm as
    ``torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)`` in front of it would — over every parameter of every group
    that has a gradient — but inside the update: the gradients are read once more for their sum of squares and the update
    multiplies them by the coefficient as it reads them.  ``p.grad`` is NOT rewritten: after the step it still holds the
    unscaled gradient.  ``opt.grad_norm`` / ``opt.clip_coef`` are 0-dim fp32 device tensors with the step's pre-clip norm and
    coefficient; no host synchronise is involved.  If any parameter with a gradient is off the kernel's route, or they live on
    more than one device, the whole step is ``clip_grad_norm_`` over all of them (which does rewrite the gradients) followed
    by the ordinary step.  L2 only; a non-finite norm is not special (``error_if_nonfinite=False``)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, clamp=None, emit_planes=None, max_grad_norm=None):
        _reject("FusedQuantSGD", maximize=maximize, dampening=dampening != 0, differentiable=differentiable, foreach=foreach,
                fused=fused)
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FusedQuantSGD: negative lr / momentum / weight_decay")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, clamp, emit_planes, max_grad_norm)

    _BAKED = ("momentum", "weight_decay", "nesterov")
    _STATE_KEYS = ("momentum_buffer",)

    def _check_group(self, group):
        _reject("FusedQuantSGD", maximize=group["maximize"], dampening=group["dampening"] != 0)

    def _allocate(self, p, group):
        if group["momentum"] == 0:
            return []
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return [st["momentum_buffer"]]

    @staticmethod
    def _scalars_per_group(n):
        return 1

    def _launch_captured(self, cg, skip=None, gscale=None):
        # no first-step flag: the buffers exist, and from a zeroed buffer mu * 0 + g IS the first step's value (see allocate_state)
        mu = cg.baked["momentum"]
        ops.optim_step_sgd_dev(cg.params, [p.grad for p in cg.params], [st[0] for st in cg.states] if mu != 0 else None, cg.scalars,
                               momentum=mu, weight_decay=cg.baked["weight_decay"], nesterov=cg.baked["nesterov"], clamps=cg.clamps,
                               planes=cg.planes, skip=skip, gscale=gscale)

    def _scalars_of(self, cg):
        return [float(self.param_groups[cg.index]["lr"])]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        off_route = []
        gscale = self._clip()
        for group in self.param_groups:
            self._check_group(group)
            lr, mu, wd, nesterov = group["lr"], group["momentum"], group["weight_decay"], group["nesterov"]
            fused, library = self._split(group, self._STATE_KEYS)
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
                                   first=first, clamps=[self._clamp_plan.get(p) for p in plist], planes=planes, gscale=gscale)
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
    per parameter group.  Arguments (``max_grad_norm`` included: ``p.grad`` stays unscaled on the fused path) and the handling of
    parameters off the kernel's route as in ``FusedQuantSGD``; ``step`` is
    kept per parameter as torch keeps it (a host scalar tensor) and the bias corrections are computed from it every step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, clamp=None,
                 emit_planes=None, max_grad_norm=None):
        _reject("FusedQuantAdam", amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable,
                foreach=foreach, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedQuantAdam: a tensor lr is not implemented")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedQuantAdam: lr / eps / weight_decay negative or a beta outside [0, 1)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults, clamp, emit_planes, max_grad_norm)

    _BAKED = ("betas", "eps", "weight_decay")
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def _check_group(self, group):
        _reject("FusedQuantAdam", amsgrad=group["amsgrad"], maximize=group["maximize"], capturable=group["capturable"],
                decoupled_weight_decay=group.get("decoupled_weight_decay", False))

    def _allocate(self, p, group):
        st = self._init_state(p)
        return [st["exp_avg"], st["exp_avg_sq"]]

    @staticmethod
    def _scalars_per_group(n):
        return 2 * n

    def _launch_captured(self, cg, skip=None, gscale=None):
        ops.optim_step_adam_dev(cg.params, [p.grad for p in cg.params], [st[0] for st in cg.states], [st[1] for st in cg.states],
                                cg.scalars, betas=cg.baked["betas"], eps=cg.baked["eps"], weight_decay=cg.baked["weight_decay"],
                                clamps=cg.clamps, planes=cg.planes, skip=skip, gscale=gscale)

    def _scalars_of(self, cg):
        # the step counts are read from state["step"], so eager step() calls between replays are counted too
        steps = [int(t) + 1 for t in torch.stack(cg.steps).tolist()]
        return [c for pair in ops.adam_coefficients(steps, self.param_groups[cg.index]["lr"], cg.baked["betas"]) for c in pair]

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
        if self._max_grad_norm is not None:        # the state first: the clip's route check looks at it
            for group in self.param_groups:
                self._check_group(group)
                for p in group["params"]:
                    if p.grad is not None:
                        self._init_state(p)
        gscale = self._clip()
        for group in self.param_groups:
            self._check_group(group)
            lr, betas, eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is not None:
                    self._init_state(p)
            fused, library = self._split(group, self._STATE_KEYS)
            for plist in fused.values():
                states = [self.state[p] for p in plist]
                steps = []
                for st in states:
                    st["step"] += 1
                    steps.append(int(st["step"]))
                planes = [self._plane_of(p) for p in plist]
                ops.optim_step_adam(plist, [p.grad for p in plist], [st["exp_avg"] for st in states],
                                    [st["exp_avg_sq"] for st in states], steps, lr=lr, betas=betas, eps=eps, weight_decay=wd,
                                    clamps=[self._clamp_plan.get(p) for p in plist], planes=planes, gscale=gscale)
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
