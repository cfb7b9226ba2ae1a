"""The contract of the implicit-hipGraph wrapper itself (utils/implicit.py), on the small sign conv root of
test_gpu_implicit_chains.py: hooks that arrive AFTER the root was wrapped, a forward that writes a buffer of its own tree, and the
work buffer of ``ops.abs_mean`` when its first call on a stream happens inside a stream capture."""
import pytest
import torch
import torch.nn as nn

from test_gpu_implicit_chains import _eighths, _module_by_module, _sign_conv_root
from pytorch_quantize_impls_amd import lazy, ops, utils
from pytorch_quantize_impls_amd.utils import implicit
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _no_timing_verdict(monkeypatch):
    """No test here may depend on the wall clock: the "replay must be faster" verdict is off (KEEP_IF_FASTER = 0)."""
    monkeypatch.setattr(implicit, "KEEP_IF_FASTER", 0.0)


def _stats(root):
    return utils.implicit_graph_stats(root)


def _wrapped_and_replaying(dev):
    root, x = _sign_conv_root(dev), _eighths((3, 3, 10, 10), dev, 101)
    want = _module_by_module(root, x)
    with torch.no_grad():
        for _ in range(5):
            assert torch.equal(root(x), want)
    st = _stats(root)
    assert st["wrapped"] and st["graphs"] == 1 and st["replays"] >= 1 and st["capture_failures"] == {}, st
    return root, x, want


@pytest.mark.parametrize("where", ("inner forward hook", "root pre-hook", "process-wide hook"))
def test_a_hook_registered_after_the_wrap_sees_every_call(dev, where):
    """wrap -> register a hook: while it is there every call runs the original forward (the hook fires, the value is the eager one,
    ``replays`` stands still); after ``remove()`` the SAME graph replays again."""
    with utils.implicit_graphs(True):
        root, x, want = _wrapped_and_replaying(dev)
        seen = []
        if where == "inner forward hook":
            h = root[4].register_forward_hook(lambda mod, inp, out: seen.append(1))            # the second BinConv2d
        elif where == "root pre-hook":
            h = root.register_forward_pre_hook(lambda mod, inp: seen.append(1))
        else:
            h = nn.modules.module.register_module_forward_hook(lambda mod, inp, out: seen.append(1) if mod is root else None)
        try:
            r = _stats(root)["replays"]
            with torch.no_grad():
                for i in range(4):
                    assert torch.equal(root(x), want), i
            st = _stats(root)
            assert len(seen) == 4, (where, len(seen), "the hook was skipped by a replay")
            assert st["replays"] == r and st["hooked_calls"] == 4, st
        finally:
            h.remove()
        with torch.no_grad():
            for i in range(3):
                assert torch.equal(root(x), want), i
        st = _stats(root)
        assert len(seen) == 4 and st["replays"] == r + 3 and st["graphs"] == 1 and st["captures"] == 1 and st["value_mismatch"] == 0, st


class _Counting(nn.Module):
    """A root whose eval forward writes one of its own buffers — a call counter — and then runs the sign chain."""

    def __init__(self, body):
        super().__init__()
        self.body = body
        self.register_buffer("calls", torch.zeros((), dtype=torch.int64))

    def forward(self, x):
        self.calls += 1
        return self.body(x)


def test_a_forward_that_writes_its_own_buffer_is_left_eager_for_good(dev):
    """Every call changes the tree's state signature, so a graph of such a root is stale the moment it exists (and a replay would
    repeat the captured write without its Python side).  The wrapper finds out at the first verification — one capture — and
    leaves the root eager for good.  Forwards the root sees: one per user call, plus in the third call the warm-up in front of the
    capture and the verification behind the first replay (the timing verdict is off; it would add 3 replays + 3 eager forwards) —
    2 extra, pinned through ``calls``.  Before the fix every call from the third on captured again: 3 forwards per call."""
    body, x = _sign_conv_root(dev), _eighths((3, 3, 10, 10), dev, 101)
    root = _Counting(body).to(dev).eval()
    with utils.implicit_graphs(True):
        want = _module_by_module(root, x)
        base = int(root.calls)
        assert base == 1
        steps, last = [], base
        with torch.no_grad():
            for i in range(12):
                y = root(x)
                assert type(y) is torch.Tensor and torch.equal(y, want), i
                now = int(root.calls)
                steps.append(now - last)
                last = now
        assert steps == [1, 1, 3] + [1] * 9, steps
        st = _stats(root)
        print(f"IMPLICIT-STATS counting-root: graphs={st['graphs']} replays={st['replays']} captures={st['captures']} "
              f"left_eager={st['left_eager']!r}")
        assert st["wrapped"] and st["captures"] <= 2 and st["graphs"] == 0 and st["replays"] == 1, st
        assert isinstance(st["left_eager"], str) and "writes" in st["left_eager"], st
        assert st["value_mismatch"] == 0 and st["capture_failures"] == {}, st
        assert int(root.calls) == base + 12 + 2
        # ... and the same root still follows its state and its input
        with torch.no_grad():
            body[4].weight.mul_(-1.0)
            new = _module_by_module(root, x)
            assert not torch.equal(new, want) and torch.equal(root(x), new)
        assert _stats(root)["captures"] == st["captures"]


def test_abs_mean_first_called_inside_a_stream_capture(dev):
    """The work buffer of qt_abs_mean_f32 (a ticket counter that has to start at zero) is cached per stream.  A buffer made during a
    capture is only RECORDED as zeroed and lives in the graph's pool: it must not reach the cache, or an eager call on that stream
    would start from a ticket nobody zeroed and never write its result.  Values: multiples of 1/8 (every partial sum exact), so
    the fp64 mean rounded to fp32 is the only admissible result; a size with a tail and several workgroups."""
    g = torch.Generator().manual_seed(3)
    w = torch.randint(-40, 41, (4 * 4097 + 3,), generator=g).float() / 8
    ref = torch.tensor(float(w.double().abs().mean()), dtype=torch.float32)      # (on the CPU: the exact sum / n, rounded twice)
    w = w.to(dev)
    stream = torch.cuda.Stream(device=dev)
    key = (dev.index, int(stream.cuda_stream))
    ops._ABS_MEAN_WORK.pop(key, None)                 # (stream handles come from a pool: another test may have used this one)
    cached = dict(ops._ABS_MEAN_WORK)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
        out = ops.abs_mean(w)
    assert key not in ops._ABS_MEAN_WORK and ops._ABS_MEAN_WORK.keys() == cached.keys(), "a buffer of the capture was cached"
    graph.replay()
    torch.cuda.synchronize(dev)
    first = out.clone()
    assert torch.equal(first.cpu(), ref), (float(first), float(ref))
    with torch.cuda.stream(stream):
        eager = ops.abs_mean(w)
    torch.cuda.synchronize(dev)
    assert key in ops._ABS_MEAN_WORK and int(ops._ABS_MEAN_WORK[key][0]) == 0
    assert torch.equal(eager.cpu(), ref), (float(eager), float(ref))
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out.cpu(), ref) and torch.equal(out, first)
    assert lazy.ENABLED


def test_folds_of_another_probe_signature_stay_alive_and_are_reused(dev):
    """The device BatchNorm fold of a fused block is made per probe signature (batch extent 1 or more, memory format).  A hipGraph
    captured for signature A has the addresses of A's fold, negative-slope words and integer thresholds baked in, so a forward
    with signature B must neither free nor recompute them (layers/fused.py:_kept_folds): same objects, same addresses when A comes
    back; a written BatchNorm starts over."""
    from pytorch_quantize_impls_amd import packed
    from pytorch_quantize_impls_amd.layers import BinConv2d, FusedConvPoolBnSign, FusedDepthwiseBnSign
    g = torch.Generator().manual_seed(5)

    def bn_of(c):
        bn = nn.BatchNorm2d(c).to(dev).eval()
        bn.running_mean.copy_(torch.randn(c, generator=g).to(dev) * 3)
        bn.weight.data.copy_((torch.randn(c, generator=g) + 0.2).to(dev))
        return bn

    def pm1(n, c):
        return (torch.randint(0, 2, (n, c, 8, 8), generator=g).float() * 2 - 1).to(dev)

    def tensors(blk):
        entry = blk._pool._folded
        held = list(entry[1]) + [blk._neg_alpha] + ([blk._thr[1]] if getattr(blk, "_thr", None) is not None else [])
        return entry, held, [t.data_ptr() for t in held]

    conv = BinConv2d(32, 40, 3, padding=1).to(dev).eval()
    dw = BinConv2d(32, 32, 3, padding=1, groups=32).to(dev).eval()
    blocks = ((FusedConvPoolBnSign(conv, bn_of(40), nn.MaxPool2d(2), fold="device"),
               lambda x: packed.PackedActivation(ops.sign_pack(x.permute(0, 2, 3, 1).contiguous())[0], tuple(x.shape)),
               (pm1(3, 32), pm1(1, 32))),
              (FusedDepthwiseBnSign(dw, bn_of(32), nn.MaxPool2d(2), fold="device"), lambda x: x,
               (pm1(3, 32), pm1(3, 32).contiguous(memory_format=torch.channels_last), pm1(1, 32))))
    with torch.no_grad():
        for blk, feed, (xa, *others) in blocks:
            bits_a = blk(feed(xa)).planes.sign.clone()
            entry_a, held_a, ptrs_a = tensors(blk)
            assert len(held_a) >= 3
            for xb in others:
                blk(feed(xb))
                entry_b, held_b, ptrs_b = tensors(blk)
                assert entry_b is not entry_a and not set(ptrs_a) & set(ptrs_b), "another signature, another fold"
                assert entry_a in blk._pool.__dict__["_folded_kept"][1].values(), "signature A's fold was dropped"
                again = blk(feed(xa)).planes.sign
                entry, held, ptrs = tensors(blk)
                assert entry is entry_a and all(p is q for p, q in zip(held, held_a)) and ptrs == ptrs_a, "recomputed, not reused"
                assert torch.equal(again, bits_a)
            blk.bn.running_mean.add_(1.0)             # a written BatchNorm (it drops the graphs too): everything is folded anew
            blk(feed(xa))
            assert blk._pool._folded is not entry_a and list(blk._pool.__dict__["_folded_kept"][1].values()) == [blk._pool._folded]
