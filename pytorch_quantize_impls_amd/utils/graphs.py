"""hipGraph replay of a fixed-shape inference forward (launch-bound small batches).

At batch 256 the fused AlexNet-Bin forward is GPU-bound (1.19 ms, ~25 launches); at batch 1-8 the same 25 launches
cost more host + dispatch time than device time: eager 0.37 ms vs 0.27 ms replayed (tools/bench_graph_small_batch.py).
The C-ABI kernels are launched on torch's current stream, so they are captured like any torch op; the only
requirement is a forward without host synchronisation (no un-tagged +-1 detection: give first layers
``binary_input = False``; no DoReFa code-overflow check inside the captured region).
"""
import contextlib
import gc

import torch
from torch.utils._pytree import tree_map_only

from .. import lazy


@contextlib.contextmanager
def _no_collection_inside():
    """Around a stream capture: a full garbage collection first, none inside.  A model that was replayed implicitly is a reference
    cycle (root -> its instance ``forward`` -> engine -> root) that owns hipGraphs, so it dies in whatever allocation happens to
    trigger the cyclic collector; when that fell inside another model's capture, the destruction of its graphs and of their memory
    pool there aborted the process.  ``torch.cuda.graph`` itself no longer collects on entry.  The collector's switch is
    process-wide: a thread that toggles it while another captures is not guarded against."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class GraphedModule(torch.nn.Module):
    """``GraphedModule(module, example_input)(x)``: copies x into the captured input buffer, replays the graph and
    returns the captured output tensor (overwritten by the next call: clone it to keep it).

    ``static_input`` is that buffer: a caller that produces its batches there (the target of its host-to-device copy, or of the
    previous pipeline stage) passes it back — ``g(g.static_input)`` — and the replay starts without the device-to-device copy
    (154 MB / 53 us for a 256 x 3 x 224 x 224 batch)."""

    def __init__(self, module: torch.nn.Module, example_input: torch.Tensor, warmup: int = 3, call=None):
        super().__init__()
        if not example_input.is_cuda:
            raise TypeError("graph capture needs a device input")
        self.module = module
        if call is not None:                        # (implicit graphs, utils/implicit.py: the root's ORIGINAL forward — calling the
            object.__setattr__(self, "_call", call)  #  module itself would re-enter the wrapper installed on it)
            module = call
        self._static_in = example_input.clone()
        self._stream = torch.cuda.Stream(device=example_input.device)
        self._graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.stream(self._stream):
            for _ in range(warmup):                 # allocations, weight packing and caches settle before capture
                module(self._static_in)
            torch.cuda.synchronize(example_input.device)
            with _no_collection_inside(), torch.cuda.graph(self._graph, stream=self._stream):
                out = module(self._static_in)
                # a module that ends in a quantised conv chain returns a deferred activation (lazy.py): its kernels
                # have to be part of the graph, so it is turned into its value inside the captured region
                #: the forward's own result was (or contained) a deferred activation: a root that hands such a result to a consumer
                #: outside itself is not wrapped implicitly (utils/implicit.py) — the consumer would lose the fused hand-over
                self.lazy_output = _contains_lazy(out)
                self._static_out = tree_map_only(lazy.LazyActivation, lambda t: t.value(), out)
        torch.cuda.synchronize(example_input.device)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape != self._static_in.shape or x.dtype != self._static_in.dtype:
            raise ValueError(f"captured for input {tuple(self._static_in.shape)} {self._static_in.dtype}, "
                             f"got {tuple(x.shape)} {x.dtype}")
        if x is not self._static_in:
            self._static_in.copy_(x)
        self._graph.replay()
        return self._static_out

    @property
    def static_input(self) -> torch.Tensor:
        """The captured input buffer (write the next batch here and call ``self(self.static_input)``: no copy)."""
        return self._static_in


def _contains_lazy(out) -> bool:
    if isinstance(out, lazy.LazyActivation):
        return True
    if isinstance(out, (tuple, list)):
        return any(_contains_lazy(o) for o in out)
    if isinstance(out, dict):
        return any(_contains_lazy(o) for o in out.values())
    return False


def graphed(module: torch.nn.Module, example_input: torch.Tensor, warmup: int = 3) -> GraphedModule:
    return GraphedModule(module, example_input, warmup)


class AutoGraphed(torch.nn.Module):
    """``AutoGraphed(model)``: the un-modified model, with its fixed-shape inference forwards replayed as hipGraphs.

    The module graphs of small-map nets are host-bound when run eagerly (DoReFa ResNet-18 at 32 x 32, batch 256: ~2.0 ms of
    Python and launch latency around 0.7 ms of device work; BinaryNet-AlexNet at batch 1: 0.69 ms against 0.13 ms — module
    machinery spread thin over ~150 module calls).  This wrapper keeps the eager path for everything that
    cannot be replayed — training mode, autograd enabled, CPU tensors, the first ``capture_after`` calls with a new input
    signature — and from then on copies the input into a captured buffer and replays the graph captured for that signature
    (shape, dtype, strides, device).  The captured graphs are dropped when a parameter or buffer of the model is written
    (version counters), e.g. after ``load_state_dict`` or a training epoch.  A forward that cannot be captured (it asks the device
    a question) is remembered as such and stays eager.  The returned tensor is a copy of the captured output unless
    ``clone_output=False`` (then it is overwritten by the next call with the same signature)."""

    def __init__(self, module: torch.nn.Module, capture_after: int = 1, max_graphs: int = 8, clone_output: bool = True, call=None,
                 keep_if_faster: float = 0.0):
        super().__init__()
        self.module = module
        # ``call``: what runs the eager forward (default: the module itself); ``keep_if_faster`` = f > 0: at capture time the replay
        # and the eager forward are both timed (the capture synchronises anyway) and the graph is only kept when it needs less than
        # f x the eager time — a device-bound forward gains nothing from a replay and its private memory pool is given back
        object.__setattr__(self, "_call", call if call is not None else module)
        self.keep_if_faster = float(keep_if_faster)
        self.not_faster = 0
        self.refuse_lazy_outputs = False
        self.capture_after, self.max_graphs, self.clone_output = int(capture_after), int(max_graphs), bool(clone_output)
        self._graphs, self._seen, self._state = {}, {}, None
        self.replays = self.eager_calls = 0
        #: stream captures started (kept or not): grows with every signature and every write to a parameter / buffer, not with calls
        self.captures = 0
        #: captures that failed, by reason ("ExceptionType: message" -> count): such a signature stays eager — VISIBLY (a genuine
        #: bug inside a captured forward must not turn into a silent performance regression); ``strict=True`` re-raises instead
        self.capture_failures = {}
        self.strict = False

    def _state_sig(self):
        # version counter + storage of every parameter and buffer (optimizer steps, load_state_dict, copy_, .to()); writes through
        # ``.data`` are invisible to it, as they are to the layers' own plane caches: call reset() after one
        return tuple((t._version, t.data_ptr()) for t in self.module.parameters()) + \
            tuple((t._version, t.data_ptr()) for t in self.module.buffers())

    def reset(self):
        """Drop every captured graph (after a manual ``weight.data`` edit)."""
        self._graphs.clear()
        self._seen.clear()
        self._state = None

    def forward(self, x):
        # (a submodule left in train() — BatchNorm fine-tuning, stochastic quantisers — would be captured once and replayed with
        # frozen behaviour: every module has to be in eval mode, not just the root)
        ok = (isinstance(x, torch.Tensor) and x.is_cuda and not torch.is_grad_enabled()
              and not _any_training(self.module) and not torch.cuda.is_current_stream_capturing())
        if not ok:
            self.eager_calls += 1
            return self._call(x)
        sig = self._state_sig()
        if sig != self._state:                          # weights / running statistics were written: the captured kernels
            self._graphs.clear()                        # baked the old packed planes in
            self._seen.clear()
            self._state = sig
        key = (tuple(x.shape), x.dtype, tuple(x.stride()), x.device)
        g = self._graphs.get(key, False)
        if g is False:
            n = self._seen.get(key, 0) + 1
            self._seen[key] = n
            if n <= self.capture_after or len(self._graphs) >= self.max_graphs:
                self.eager_calls += 1
                return self._call(x)
            self.captures += 1
            try:
                g = GraphedModule(self.module, x, warmup=1, call=None if self._call is self.module else self._call)
                if self.refuse_lazy_outputs and g.lazy_output:
                    g = None
                    self.capture_failures["deferred output"] = self.capture_failures.get("deferred output", 0) + 1
                elif self.keep_if_faster > 0.0 and not self._replay_pays(g, x):
                    g = None
                    self.not_faster += 1
            except Exception as exc:                    # e.g. a host synchronisation inside the forward: stay eager for this signature,
                torch.cuda.synchronize(x.device)        # and say so (capture_failures; bench.py prints it)
                if self.strict:
                    raise
                reason = f"{type(exc).__name__}: {str(exc).splitlines()[0][:160] if str(exc) else ''}"
                self.capture_failures[reason] = self.capture_failures.get(reason, 0) + 1
                g = None
            self._graphs[key] = g
            self._state = self._state_sig()             # the warm-up forwards may have built caches, never written parameters
        if g is None:
            self.eager_calls += 1
            return self._call(x)
        self.replays += 1
        out = g(x)
        return tree_map_only(torch.Tensor, torch.clone, out) if self.clone_output else out


def _replay_pays(self, g, x, n: int = 3) -> bool:
    """Wall time of n replays against n eager forwards, each bracketed by a device synchronise (capture time only)."""
    import time
    dev = x.device

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    with torch.no_grad():
        t_replay = timed(lambda: g(x))
        t_eager = timed(lambda: tree_map_only(lazy.LazyActivation, lambda t: t.value(), self._call(x)))
    return t_replay < self.keep_if_faster * t_eager


AutoGraphed._replay_pays = _replay_pays


def _any_training(module: torch.nn.Module) -> bool:
    """A module of the tree is in training mode.  The quantised layers' own children (``weight_op``: the weight quantiser as a
    module) are not looked at: the reference's train() / eval() of those layers sets the flag of the layer alone
    (layers/binary_layers.py:30-40 — kept, layers/common.py), so they read ``training`` for ever and never act on it."""
    from ..layers.common import EvalSwapMixin
    if module.training:
        return True
    if isinstance(module, EvalSwapMixin):
        return False
    return any(_any_training(c) for c in module.children())


def auto_graphed(module: torch.nn.Module, **kw) -> AutoGraphed:
    return AutoGraphed(module, **kw)


class GraphedTrainStep:
    """One training step — forward, loss, backward and, given a fused optimiser, the update — of a fixed-shape batch captured once
    as a hipGraph and replayed.

    The training steps of small-map nets are launch-bound (DoReFa ResNet-18 at 32 x 32, batch 256: ~900 kernels of 5-40 us per
    step, 12.5 ms eager, 10.3 ms replayed; DESIGN.md section 1 "Training path").  This backend's autograd Functions launch on
    torch's current stream and allocate through torch's caching allocator, so a whole step is capturable — provided nothing in it
    asks the device a question: the +-1 / int8-range verdicts of un-tagged activations must come from memory
    (``functions._fused.DETECT_MODE = "remember"``: a wrong remembered verdict turns the output into NaN, never into a plausible
    number), which this class switches on for the warm-up, the capture and nothing else.

        step = GraphedTrainStep(model, lambda out, target: F.nll_loss(F.log_softmax(out, 1), target), x0, t0)
        for x, t in loader:            # same shapes / dtypes as x0, t0
            loss = step(x, t)          # gradients are in p.grad (overwritten by the next call)
            opt.step()                 # any optimizer: it stays outside the graph

    Gradients are zeroed inside the graph (``zero_grad(set_to_none=False)``), so every replay leaves exactly this batch's
    gradients behind.  BatchNorm running statistics and ``num_batches_tracked`` advance on every replay, like eager steps.

    ``optimizer=``: a ``utils.FusedQuantSGD`` / ``utils.FusedQuantAdam`` whose update — recurrence, the layers' clamp and the
    weight planes of the next forward — becomes part of the graph, so the whole step of the reference's loops is one replay:

        opt = utils.FusedQuantAdam(model, lr=1e-3)
        step = GraphedTrainStep(model, loss_fn, x0, t0, optimizer=opt)
        for x, t in loader:
            loss = step(x, t)          # forward, loss, backward, optimizer.step(), model.clamp()
            scheduler.step()           # group["lr"] is read before every replay

      * The warm-up runs forward, loss and backward only: constructing the step applies no update (parameters and optimiser state
        are what they were; the state tensors exist afterwards, as zeros).
      * Per-step scalars (learning rate, Adam's bias corrections from ``state["step"]``) are written to device memory before each
        replay; momentum, betas, eps, weight decay and nesterov are baked into the graph and changing one raises on the next call.
        ``optimizer.step()`` may still be called eagerly between replays (step counts come from ``state["step"]``).
      * The captured forward of a deterministic LinearBin / LinearTer reads the plane buffer the captured update rewrites.  Before a
        replay, a weight whose version counter or plane record is not what the last replay left (``load_state_dict``, an in-place
        edit under ``no_grad``, ``eval()`` / ``train()``) gets its plane packed again, eagerly.  Writes through ``.data`` are
        invisible to that check, as they are to the eval cache.  ``emit_planes=False``: the captured forward packs from the fp32
        weight.
      * ``p.grad`` holds the batch's gradients after a call, as without an optimiser.  The graph owns those tensors and zeroes them
        itself: a call after ``zero_grad(set_to_none=True)`` (torch's default) raises, it does not train on buffers nobody reads.
      * A captured step has no library path: every parameter with a gradient must be a contiguous fp32 device tensor (a
        channels-last conv weight is not), else the constructor raises ``ValueError`` naming it.  ``optimizer.load_state_dict``
        replaces the state tensors, so the next call raises: load first, then construct the step.
      * One optimiser may serve several steps (a full and a tail batch shape): each has its own scalar block, all share the
        optimiser's state and plane buffers.
      * An optimiser built with ``max_grad_norm=`` clips inside the graph: the norm launches over the gradients of all groups sit
        between the captured backward and the captured update, which multiplies the gradients by the coefficient as it reads
        them — ``p.grad`` stays unscaled.  ``optimizer.max_grad_norm = x`` reaches the next replay like a learning rate;
        switching clipping on or off after the capture raises.  With ``recover=True`` the norm launches run in a skipped
        step too, but they write only their own workspace and the two words behind ``optimizer.grad_norm`` / ``clip_coef``.
    Other optimiser types stay outside the graph (the form above); so do data-parallel steps: a model whose gradients a
    ``GradientSynchronizer`` averages is refused, because the all-reduce runs between backward and the update.

    ``recover=True``: survive a wrong remembered verdict.  Training moves activations: a tensor that was +-1, in the int8 code
    range or exact in bf16 when the step was captured may stop being so, and a replay then poisons that layer's result with NaN —
    and with it every gradient, the update, the optimiser state and BatchNorm's running statistics (behind a BinaryConnect,
    ``safeSign(NaN) = +1``, without the loss ever showing it).  With ``recover=True`` the graph ORs the device flags of every
    trusted verdict of the step (``functions._fused.flag_sink``) into a guard word that its update launches read: raised, the
    update is skipped on the device.  The host learns of it in ``settle()``, restores the module buffers from a snapshot the
    graph took, runs the same batch eagerly in "verify" mode — which remembers the negative answer, so each (weight, question)
    flips at most once — and captures a new graph.  After ``max_recaptures`` re-captures the step warns once and stays eager.

      * ``step(x, t)`` settles the PREVIOUS call first (it needs that call's batch, which is still in the static buffers), then
        replays.  That settle waits for the previous replay to finish before the next batch is even copied in: an armed step
        gives up the run-ahead of the host over the device — the device idles while the host enqueues the next replay —
        and pays for it on launch-bound nets (README, "Fused update", has the figures).  ``step.settle()`` settles the last call
        now; it returns whether a recovery took place (``recoveries`` / ``recaptures`` count them).
      * A recovered call equals the plain eager loop on that batch, and the re-capture puts buffers, gradients and the random
        number generators back.  The REPLAYS of a model that draws random numbers (Dropout, stochastic quantisers) follow
        torch's graph-safe generator, as with ``recover=False``: such a model is not bit-comparable to its eager loop anyway.
      * ``p.grad`` and the returned loss are those of the batch only AFTER ``settle()``: until then they may be the poisoned
        ones of a step that is about to be run again.  The returned tensor is owned by the step and survives a re-capture.
      * Parameters, optimiser state and module buffers must not be touched from outside between a call and its settle.
      * ``optimizer=None``: the caller's own optimiser runs right after the call, so every call settles before it returns —
        one synchronise per call.
      * A step in which no verdict is trusted (every input tagged by its quantiser) arms nothing: no OR launch, the unguarded
        update, nothing to settle.
    ``recover=False`` (default) is the step as it always was, launch for launch."""

    def __init__(self, model: torch.nn.Module, loss_fn, example_input: torch.Tensor, example_target: torch.Tensor,
                 warmup: int = 3, optimizer=None, recover: bool = False, max_recaptures: int = 8):
        if optimizer is not None:
            from .data_parallel import is_synchronized
            from .optim import _FusedQuantOptimizer
            if not isinstance(optimizer, _FusedQuantOptimizer):
                raise TypeError(f"GraphedTrainStep captures the update of utils.FusedQuantSGD / utils.FusedQuantAdam only, not of "
                                f"{type(optimizer).__name__}: keep it outside the graph (loss = step(x, t); opt.step())")
            if is_synchronized(model.parameters()):
                raise RuntimeError("GraphedTrainStep: a GradientSynchronizer averages this model's gradients between backward and the "
                                   "update; data-parallel steps keep the optimiser outside the graph (loss = step(x, t); sync.wait(); "
                                   "opt.step())")
        if not example_input.is_cuda:
            raise TypeError("graph capture needs device tensors")
        if recover and optimizer is not None and optimizer._post_clamp:
            # their clamp() is arbitrary torch code inside the graph: nothing could make it depend on the guard
            raise ValueError(f"GraphedTrainStep(recover=True): the captured update cannot skip the clamp() of "
                             f"{sorted({type(m).__name__ for m in optimizer._post_clamp})}, which utils.clamp_plan cannot restate; "
                             "keep the optimiser outside the graph (optimizer=None) or use recover=False")
        self.model, self.loss_fn, self.optimizer = model, loss_fn, optimizer
        self.recover, self.max_recaptures = bool(recover), int(max_recaptures)
        #: steps whose guard was raised and that were run again eagerly / graphs captured anew after one (``recover=True``)
        self.recoveries = self.recaptures = 0
        self._warmup = max(1, warmup)
        self._x, self._t = example_input.clone(), example_target.clone()
        self._stream = torch.cuda.Stream(device=example_input.device)
        for p in model.parameters():
            if p.requires_grad and p.grad is None:
                p.grad = torch.zeros_like(p)          # static gradient buffers: the captured backward accumulates into them
        self._pending = self._armed = self._eager = False
        if self.recover:
            dev = example_input.device
            self._guard = torch.zeros(1, dtype=torch.int32, device=dev)
            self._guard_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._event = torch.cuda.Event()
            self._buffers = list(model.buffers())
            self._snapshot = [torch.empty_like(b) for b in self._buffers]
            self._flags = self._out = None
        self._capture_graph()

    def _capture_graph(self):
        """Warm-up and stream capture under "remember" (the constructor; with ``recover=True`` every re-capture as well)."""
        from .. import ops
        from ..functions import _fused
        optimizer, dev = self.optimizer, self._x.device
        self._graph = torch.cuda.CUDAGraph()
        self._capture, planes = None, contextlib.nullcontext()
        if optimizer is not None:
            # this graph's handle on the optimiser (its own scalar block; the optimiser may serve other graphs too): state exists,
            # raises for what a captured step cannot update
            self._capture = optimizer.prepare_capture()
            optimizer.refresh_planes(self._capture)   # the planes the captured forward reads: packed once, into the persistent buffers
            self._stream.wait_stream(torch.cuda.current_stream(dev))     # (packed on the caller's stream)
            planes = optimizer.capturing(self._capture)
        with _fused.detect_scope("remember"), planes:  # thread-local; the Functions carry the detect mode into their backward
            with torch.cuda.stream(self._stream):
                for _ in range(self._warmup):         # verdicts asked (and remembered), allocations and weight caches settle
                    loss = self._one()
                if self.recover and self._out is None:
                    self._out = torch.empty_like(loss)     # what __call__ returns: owned by the step, not by one of its graphs
                torch.cuda.synchronize(dev)
                with _no_collection_inside(), torch.cuda.graph(self._graph, stream=self._stream):
                    if not self.recover:
                        self._loss = self._one()
                        if optimizer is not None:
                            optimizer.captured_step(self._capture)
                    else:
                        self._guard.zero_()
                        if self._buffers:
                            torch._foreach_copy_(self._snapshot, self._buffers)
                        with _fused.flag_sink() as flags:
                            loss = self._one()
                        self._flags = flags           # the graph's last launches read them: they live as long as it does
                        self._armed = len(flags) > 0
                        if self._armed:
                            ops.flags_or(flags.flags, self._guard)
                        if optimizer is not None:     # no trusted verdict in the step: nothing to guard against
                            optimizer.captured_step(self._capture, skip=self._guard if self._armed else None)
                        self._out.copy_(loss)
            torch.cuda.synchronize(dev)

    def _one(self):
        self.model.zero_grad(set_to_none=False)
        loss = self.loss_fn(self.model(self._x), self._t)
        loss.backward()
        return loss.detach()

    def __call__(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if x.shape != self._x.shape or x.dtype != self._x.dtype or target.shape != self._t.shape or target.dtype != self._t.dtype:
            raise ValueError(f"captured for input {tuple(self._x.shape)} {self._x.dtype} / target {tuple(self._t.shape)} "
                             f"{self._t.dtype}, got {tuple(x.shape)} {x.dtype} / {tuple(target.shape)} {target.dtype}")
        if self.recover:
            self.settle()                                   # the previous step may still need its batch: it is in _x / _t
        self._x.copy_(x)
        self._t.copy_(target)
        if self._eager:
            return self._eager_step()
        if self.optimizer is not None:
            self.optimizer.before_replay(self._capture)     # this step's scalars to the device, stale planes packed again
        self._graph.replay()
        if self.optimizer is not None:
            self.optimizer.after_replay(self._capture)      # version counters, plane records
        if not self.recover:
            return self._loss
        if self._armed:
            self._guard_host.copy_(self._guard, non_blocking=True)      # outside the graph, behind the replay on its stream
            self._event.record()
            self._pending = True
            if self.optimizer is None:
                self.settle()                               # the caller's optimiser runs next: it must not see poisoned gradients
        return self._out

    def _eager_step(self):
        """The step as the plain loop runs it, in "verify" mode (a recovery; every call once the re-captures are used up)."""
        from ..functions import _fused
        with _fused.detect_scope("verify"):
            loss = self._one()
        if self.optimizer is not None:
            self.optimizer.step()
        self._out.copy_(loss)
        return self._out

    def settle(self) -> bool:
        """``recover=True``: wait for the last call's guard.  Clear (or nothing pending): ``False``.  Raised — a remembered verdict
        was wrong for that batch, the device skipped the update: restore the module buffers from the graph's snapshot, take the
        optimiser's host bookkeeping back (``cancel_replay``), run the same batch eagerly in "verify" mode (which remembers the
        negative answer), capture a new graph, and return ``True``.  ``recoveries`` / ``recaptures`` count."""
        if not self._pending:
            return False
        self._pending = False
        self._event.synchronize()
        if int(self._guard_host[0]) == 0:
            return False
        self.recoveries += 1
        with torch.no_grad():
            if self._buffers:
                torch._foreach_copy_(self._buffers, self._snapshot)
        if self.optimizer is not None:
            self.optimizer.cancel_replay(self._capture)
        self._eager_step()                                  # the batch is still in the static input buffers
        if self.recaptures >= self.max_recaptures:
            import warnings
            warnings.warn(f"GraphedTrainStep: {self.recaptures} re-captures used up (max_recaptures); the step stays eager from now on",
                          RuntimeWarning, stacklevel=2)
            self._eager, self._armed = True, False
            self._graph = self._flags = self._capture = None
        else:
            self.recaptures += 1
            self._recapture()
        return True

    def _recapture(self):
        """A new graph under the verdicts as they are now.  Its warm-up runs forward and backward on the current batch: module
        buffers, ``p.grad`` and the random-number state (host and device generators: Dropout, stochastic quantisers) are put back
        afterwards, so the state is the eager step's.  Parameters and optimiser state are not written by a warm-up (it applies no
        update); a model whose forward writes its own parameters is refused, not mis-trained."""
        dev = self._x.device
        torch.cuda.synchronize(dev)
        rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        params = [p for p in self.model.parameters() if p.grad is not None]
        keep = [b.clone() for b in self._buffers], [p.grad.clone() for p in params]
        versions = [p._version for p in self.model.parameters()]
        self._graph = self._flags = None                    # the old graph and its memory pool go before the new capture
        self._capture_graph()
        if versions != [p._version for p in self.model.parameters()]:
            raise RuntimeError("GraphedTrainStep(recover=True): the model's forward / backward wrote a parameter during the re-capture "
                               "warm-up; the step cannot restore the eager state")
        with torch.no_grad():
            if self._buffers:
                torch._foreach_copy_(self._buffers, keep[0])
            if params:
                torch._foreach_copy_([p.grad for p in params], keep[1])
        torch.set_rng_state(rng[0])
        torch.cuda.set_rng_state(rng[1], dev)
        torch.cuda.synchronize(dev)
