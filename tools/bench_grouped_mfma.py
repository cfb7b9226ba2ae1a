#!/usr/bin/env python
"""The grouped layers with 16 ... 32 channels per group (ResNeXt-50 stages 3 and 4, a wide 24-channel layer, the strided layer that
opens stage 3, a grouped 1 x 1) at batch 256 as BinConv2d(C, Cout, k, stride, padding, groups=G) on +-1 activations, NCHW, one GPU:
one JSON line.  The protocol, the counts and the constants are those of tools/bench_grouped.py (imported): a child process per
shape under a time limit, nothing started after a failing child, the routes taking turns inside each of ``--rounds`` rounds, us per
call as the median and the range of the rounds, forward and forward + backward.  The byte and MAC counts are those of
``bench_grouped.counts`` for a layer whose output channels may differ from its input channels.

Routes:
  mfma   : ``_fused.GroupedMfmaConv2dFn`` called directly (csrc/gconv_mfma.hip; so the measurement does not depend on the switch
           ``_fused.GROUPED_MFMA``, which is set FROM it), with ``_fused.GROUPED_MFMA_WGRAD`` off: the streaming weight gradient;
  mfma_wgrad : the same node with ``_fused.GROUPED_MFMA_WGRAD`` on (a step only: the forward is the same launch);
  loop   : ``_fused.grouped_quant_conv`` with ``binary_input = True``: what these layers run with the switch off;
  torch  : F.conv2d(x, sign(W), b, groups=G) through torch (MIOpen);
  stream : ``_fused.GroupedConv2dFn`` called directly (the streaming kernels of csrc/gconv.hip, not routed at this size).
``hbm_share`` = (4 (|x| + |y|) (x 3 for a step) / 8 TB/s) / the mfma median; ``mfma_share`` = (2 macs x 3 bf16 terms / 2.5 PFLOP/s)
/ the same.  ``grouped_mfma_by_rule`` is the value ``_fused.GROUPED_MFMA`` has to ship with: True iff on every row the route takes the mfma round
range lies wholly below the loop's, forward and forward + backward.  The library and the streaming kernels are reported, not gated.
``grouped_mfma_wgrad_by_rule`` is the value of ``_fused.GROUPED_MFMA_WGRAD``: True iff on every row the route takes the step's round
range with the switch on lies wholly below the range with it off; ``step_beats_torch`` says row by row whether the step with the
switch on lies wholly below the library's.  ``wgrad`` times the weight gradient alone (its two launches through ``ops``), streaming
against matrix cores, with ``hbm_share`` = 4 (|x| + |go|) / 8 TB/s and ``mfma_share`` = 2 macs x 6 bf16 products / 2.5 PFLOP/s over
the matrix-core median.

    python tools/bench_grouped_mfma.py [--rounds 9] [--out profiles/grouped_mfma_wgrad_bench_line.json]

``--dtype bf16|fp16|both`` measures the half-precision route instead (``child_half``: the one-term kernels of csrc/gconv_mfma_h.hip
against the library's half conv, the fp32 route on the upcast tensors for information) on the rows the route takes and writes
profiles/grouped_mfma_wgrad_half_bench_line.json.  A step is measured with ``_fused.GROUPED_MFMA_WGRAD_HALF`` off (the streaming
qt_gconv2d_grad_weight_h) and on (qt_gmconv2d_grad_weight_h); ``grouped_mfma_wgrad_half_by_rule`` is the value that switch has to
ship with (both dtypes measured, on every row the step's round range with it on wholly below the range with it off), and
``grouped_mfma_half_by_rule`` (both dtypes measured, every row passing with the weight-gradient switch at that value) the value of
``_fused.GROUPED_MFMA_HALF``.  ``wgrad`` times the weight gradient's two launches alone through ``ops``: one-term matrix cores
against the streaming "_h" entry, the fp32 matrix-core entry on the upcast tensors for information.  ``--dtype ... --trace-steps``
traces half steps with the weight-gradient switch off and then on.

``--family wide`` measures the wide-group route instead (``child_wide``: ``_fused.GroupedWideConv2dFn``, csrc/gconv_wide_mfma.hip,
called directly, against the per-group loop and the library) on ``WIDE_SHAPES`` — 24 ... 64 channels per group, the rows the
kernels above decline — and writes profiles/grouped_wide_bench_line.json.  ``grouped_wide_by_rule`` is the value
``_fused.GROUPED_WIDE`` has to ship with, by the rule of ``grouped_mfma_by_rule``; ``library_wins`` lists the rows and modes where
the library's median is below the route's.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import bench_grouped as B

sys.path.insert(0, B.ROOT)

#: (channels, map, stride, groups, kernel, output channels).  768 -> 768 at 32 groups has 24 OUTPUT channels per group, no multiple
#: of 16: the matrix-core route declines it (the row keeps its other three routes); 768 -> 1536 is the 24-channel row it takes.
SHAPES = [(512, 14, 1, 32, 3, 512), (768, 14, 1, 32, 3, 768), (768, 14, 1, 32, 3, 1536), (1024, 7, 1, 32, 3, 1024),
          (512, 28, 2, 32, 3, 512), (256, 14, 1, 16, 1, 256)]
#: the wide-group rows: 24 / 24 (the row above that the old kernel declines), ResNeXt-101 32x8d's last stage, two RegNet widths
#: (40 per group; 48 per group under stride 2) and a grouped 1 x 1 of 64
WIDE_SHAPES = [(768, 14, 1, 32, 3, 768), (2048, 7, 1, 32, 3, 2048), (1360, 7, 1, 34, 3, 1360), (1008, 14, 2, 21, 3, 1008),
               (1024, 14, 1, 16, 1, 1024)]
BF16_FLOPS = 2.5e15
DEFAULT_OUT = os.path.join(B.ROOT, "profiles", "grouped_mfma_wgrad_bench_line.json")


def child(index, rounds):
    import torch
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd import _lib, ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    C, H, stride, G, k, Cout = SHAPES[index]
    pad = k // 2
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(index)
    layer = BinConv2d(C, Cout, k, stride=stride, padding=pad, groups=G).to(dev)
    layer.weight.data.uniform_(-1.2, 1.2)
    layer.binary_input = True
    args = (layer.stride, layer.padding, layer.dilation, G)
    x = torch.where(torch.rand(B.BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev)
    xg = x.clone().requires_grad_(True)

    def node(fn):
        return lambda inp: fn.apply(inp, layer.weight, layer.bias, "binary", None, ops.STE_THRESHOLD, args)

    def library(inp):                                       # in a step the library computes the weight gradient too
        wq = torch.where(layer.weight.detach() < 0, -1.0, 1.0).requires_grad_(inp.requires_grad)
        return F.conv2d(inp, wq, layer.bias, stride, pad, 1, G)

    forward = {"mfma": node(_fused.GroupedMfmaConv2dFn), "loop": lambda inp: _fused.grouped_quant_conv(layer, inp, "binary", layer._op),
               "torch": library,
               "stream": node(_fused.GroupedConv2dFn)}
    taken = ops.grouped_mfma_applicable(x.shape, layer.weight.shape, *args)
    if not taken:
        del forward["mfma"]
    with torch.no_grad():
        want = forward["loop"](x)
        go = torch.randn(want.shape, generator=g).to(dev)
        for r in set(forward) - {"loop", "torch"}:         # integer sums plus the bias: the same bits on every route of ours
            assert torch.equal(forward[r](x), want), r
    def switched(fn, on):                                   # the backward reads the switch when it runs
        def run(*a):
            _fused.GROUPED_MFMA_WGRAD = on
            return fn(*a)
        return run

    for on, gwt in ((False, "qt_gconv2d_grad_weight_f32"), (True, "qt_gmconv2d_grad_weight_f32")) if taken else ():
        calls = dict(_lib.call_counts)
        switched(lambda: forward["mfma"](xg).backward(go), on)()
        used = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
        assert used == {"qt_gmconv2d_f32": 1, "qt_gmconv2d_grad_input_f32": 1, gwt: 1}, used

    def fwd(r):
        def run():
            with torch.no_grad():
                forward[r](x)
        return run

    def step(r):
        def run():
            forward["mfma" if r == "mfma_wgrad" else r](xg).backward(go)
            xg.grad = None
            layer.zero_grad(set_to_none=True)
        return run

    def run_us(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    x_b, y_b, m = 4 * x.numel(), 4 * want.numel(), want.numel() * (C // G) * k * k
    nbytes, macs = {"fwd": x_b + y_b, "fwd_bwd": 3 * (x_b + y_b)}, {"fwd": m, "fwd_bwd": 3 * m}
    result = {"channels": C, "out_channels": Cout, "map": H, "stride": stride, "groups": G, "cin_g": C // G, "cout_g": Cout // G,
              "kernel": k, "bytes": nbytes, "macs": macs, "mfma_takes_it": taken}
    def wgrad(r):
        op = ops.grouped_mfma_conv2d_grad_weight if r == "mfma" else ops.grouped_conv2d_grad_weight
        return lambda: op(x, go, layer.weight, *args, ops.STE_THRESHOLD, True)

    for mode, make in (("fwd", fwd), ("fwd_bwd", step), ("wgrad", wgrad)):
        routes = [r for r in forward if mode != "wgrad" or r in ("stream", "mfma")]
        fns = {r: switched(make(r), False) for r in routes}
        if taken and mode == "fwd_bwd":
            fns["mfma_wgrad"] = switched(make("mfma_wgrad"), True)
        steps = {r: (2 if r == "loop" else 10) for r in fns}
        for fn in fns.values():
            for _ in range(2):
                fn()
        samples = {r: [] for r in fns}
        for _ in range(rounds):
            for r, fn in fns.items():
                samples[r].append(run_us(fn, steps[r]))
        result[mode] = {r: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                        for r, v in samples.items()}
        if not taken:
            continue
        t = result[mode]["mfma"]["median_us"] * 1e-6
        if mode == "wgrad":                                 # both operands real: six bf16 products per MAC, 2 flops each
            result[mode]["mfma"].update(hbm_share=round((x_b + y_b) / B.HBM_BYTES_PER_S / t, 3),
                                        mfma_share=round(12 * m / BF16_FLOPS / t, 3))
            continue
        result[mode]["mfma"].update(hbm_share=round(nbytes[mode] / B.HBM_BYTES_PER_S / t, 3),
                                    mfma_share=round(6 * macs[mode] / BF16_FLOPS / t, 3))
    print(json.dumps(result))


def child_wide(index, rounds):
    import torch
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd import _lib, ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    C, H, stride, G, k, Cout = WIDE_SHAPES[index]
    pad = k // 2
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(index)
    layer = BinConv2d(C, Cout, k, stride=stride, padding=pad, groups=G).to(dev)
    layer.weight.data.uniform_(-1.2, 1.2)
    layer.binary_input = True
    args = (layer.stride, layer.padding, layer.dilation, G)
    x = torch.where(torch.rand(B.BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev)
    xg = x.clone().requires_grad_(True)
    assert ops.grouped_wide_applicable(x.shape, layer.weight.shape, *args) and not ops.grouped_mfma_applicable(x.shape, layer.weight.shape, *args)

    def library(inp):                                       # in a step the library computes the weight gradient too
        wq = torch.where(layer.weight.detach() < 0, -1.0, 1.0).requires_grad_(inp.requires_grad)
        return F.conv2d(inp, wq, layer.bias, stride, pad, 1, G)

    forward = {"wide": lambda inp: _fused.GroupedWideConv2dFn.apply(inp, layer.weight, layer.bias, "binary", None, ops.STE_THRESHOLD, args),
               "loop": lambda inp: _fused.grouped_quant_conv(layer, inp, "binary", layer._op), "torch": library}
    with torch.no_grad():
        want = forward["loop"](x)
        go = torch.randn(want.shape, generator=g).to(dev)
        assert torch.equal(forward["wide"](x), want)       # integer sums plus the bias: the same bits
    calls = dict(_lib.call_counts)
    forward["wide"](xg).backward(go)
    used = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    assert used == {"qt_gwconv2d_f32": 1, "qt_gwconv2d_grad_input_f32": 1}, used

    def fwd(r):
        def run():
            with torch.no_grad():
                forward[r](x)
        return run

    def step(r):
        def run():
            forward[r](xg).backward(go)
            xg.grad = None
            layer.zero_grad(set_to_none=True)
        return run

    def run_us(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    x_b, y_b, m = 4 * x.numel(), 4 * want.numel(), want.numel() * (C // G) * k * k
    nbytes, macs = {"fwd": x_b + y_b, "fwd_bwd": 3 * (x_b + y_b)}, {"fwd": m, "fwd_bwd": 3 * m}
    result = {"channels": C, "out_channels": Cout, "map": H, "stride": stride, "groups": G, "cin_g": C // G, "cout_g": Cout // G,
              "kernel": k, "bytes": nbytes, "macs": macs,
              "plan": {op: ops.grouped_wide_plan(op, x.shape, layer.weight.shape, *args) for op in ("forward", "grad_input")}}
    for mode, make in (("fwd", fwd), ("fwd_bwd", step)):
        fns = {r: make(r) for r in forward}
        steps = {r: (2 if r == "loop" else 10) for r in fns}
        for fn in fns.values():
            for _ in range(2):
                fn()
        samples = {r: [] for r in fns}
        for _ in range(rounds):
            for r, fn in fns.items():
                samples[r].append(run_us(fn, steps[r]))
        result[mode] = {r: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                        for r, v in samples.items()}
        t = result[mode]["wide"]["median_us"] * 1e-6
        result[mode]["wide"].update(hbm_share=round(nbytes[mode] / B.HBM_BYTES_PER_S / t, 3),
                                    mfma_share=round(6 * macs[mode] / BF16_FLOPS / t, 3))
    print(json.dumps(result))


def main_wide(a):
    shapes = []
    for i in range(len(WIDE_SHAPES)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--family", "wide", "--child", str(i), "--rounds", str(a.rounds)],
                           stdout=subprocess.PIPE, text=True, timeout=B.CHILD_LIMIT_S)
        if p.returncode != 0:
            raise SystemExit(f"shape {WIDE_SHAPES[i]}: the measuring process ended with status {p.returncode}; nothing more was started")
        shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr)
    from pytorch_quantize_impls_amd.functions import _fused
    passes = [all(s[m]["wide"]["max_us"] < s[m]["loop"]["min_us"] for m in ("fwd", "fwd_bwd")) for s in shapes]
    line = {"bench": "grouped_wide", "batch": B.BATCH, "rounds": a.rounds, "dtype": "float32", "layout": "NCHW",
            "hbm_bytes_per_s": B.HBM_BYTES_PER_S, "bf16_flops": BF16_FLOPS, "shapes": shapes, "shape_passes_rule": passes,
            "grouped_wide_by_rule": all(passes), "grouped_wide_shipped": bool(_fused.GROUPED_WIDE),
            "library_wins": [[i, m] for i, s in enumerate(shapes) for m in ("fwd", "fwd_bwd")
                             if s[m]["torch"]["median_us"] < s[m]["wide"]["median_us"]]}
    text = json.dumps(line)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(B.ROOT, "profiles", "grouped_wide_bench_line.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")
    print(text)


def child_half(index, rounds, dtype):
    """``--dtype bf16|fp16``: one row the route takes, the layer as ``.to(dtype)`` on +-1 activations of that dtype.  Sides:
    mfma_h   : ``_fused.GroupedMfmaConv2dFn`` on the half tensors (csrc/gconv_mfma_h.hip; qt_gconv2d_grad_weight_h in a step:
               ``_fused.GROUPED_MFMA_WGRAD_HALF`` off);
    mfma_h_wgrad : the same node with that switch on (a step only: qt_gmconv2d_grad_weight_h);
    torch    : F.conv2d(x, sign(W), b, groups=G) in the same dtype through torch: what these layers run with the switch off;
    mfma_f32 : for information, the fp32 node on the upcast tensors.
    ``floor_share`` = max(2 (|x| + |y|) bytes (x 3 for a step) / 8 TB/s, 2 macs (x 3) / 2.5 PFLOP/s) / the mfma_h median, and
    ``floor`` says which of the two it is.  ``wgrad``: the weight gradient alone through ``ops`` — mfma_h (one-term matrix cores),
    stream_h (qt_gconv2d_grad_weight_h), mfma_f32 (the fp32 matrix-core entry on the upcast tensors)."""
    import torch
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd import _lib, ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    C, H, stride, G, k, Cout = SHAPES[index]
    pad, tdt = k // 2, {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(index)
    layer32 = BinConv2d(C, Cout, k, stride=stride, padding=pad, groups=G).to(dev)
    layer32.weight.data.uniform_(-1.2, 1.2)
    layer32.bias.data.copy_(torch.randint(-3, 4, (Cout,), generator=g))          # integers: every route's sum is exact
    layer = BinConv2d(C, Cout, k, stride=stride, padding=pad, groups=G).to(dev)
    layer.load_state_dict(layer32.state_dict())
    layer = layer.to(tdt)
    args = (layer.stride, layer.padding, layer.dilation, G)
    x32 = torch.where(torch.rand(B.BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev)
    x = x32.to(tdt)
    assert ops.grouped_mfma_applicable(x.shape, layer.weight.shape, *args)
    leaves = {"mfma_h": x.clone().requires_grad_(True), "torch": x.clone().requires_grad_(True), "mfma_f32": x32.clone().requires_grad_(True)}

    def node(lay):
        return lambda inp: _fused.GroupedMfmaConv2dFn.apply(inp, lay.weight, lay.bias, "binary", None, ops.STE_THRESHOLD, args)

    def library(inp):                                       # in a step the library computes the weight gradient too
        wq = torch.where(layer.weight.detach() < 0, -1.0, 1.0).to(tdt).requires_grad_(inp.requires_grad)
        return F.conv2d(inp, wq, layer.bias, stride, pad, 1, G)

    forward = {"mfma_h": node(layer), "torch": library, "mfma_f32": node(layer32)}
    with torch.no_grad():
        want = forward["mfma_f32"](x32).to(tdt)             # exact integer sums, rounded once
        assert torch.equal(forward["mfma_h"](x), want)
        go32 = torch.randn(want.shape, generator=g).to(dev)
    gos = {"mfma_h": go32.to(tdt), "torch": go32.to(tdt), "mfma_f32": go32}

    def switched(fn, on):                                   # the backward reads the switch when it runs
        def run():
            _fused.GROUPED_MFMA_WGRAD_HALF = on
            return fn()
        return run

    for on, gwt in ((False, "qt_gconv2d_grad_weight_h"), (True, "qt_gmconv2d_grad_weight_h")):
        calls = dict(_lib.call_counts)
        switched(lambda: forward["mfma_h"](leaves["mfma_h"]).backward(gos["mfma_h"]), on)()
        used = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
        assert used == {"qt_gmconv2d_h": 1, "qt_gmconv2d_grad_input_h": 1, gwt: 1}, used

    def fwd(r):
        def run():
            with torch.no_grad():
                forward[r](leaves[r].detach())
        return run

    def step(r):
        def run():
            forward[r](leaves[r]).backward(gos[r])
            leaves[r].grad = None
            layer.zero_grad(set_to_none=True)
            layer32.zero_grad(set_to_none=True)
        return run

    def wgrad(r):
        op = ops.grouped_conv2d_grad_weight if r == "stream_h" else ops.grouped_mfma_conv2d_grad_weight
        xa, ga, lay = (x32, go32, layer32) if r == "mfma_f32" else (x, gos["mfma_h"], layer)
        return lambda: op(xa, ga, lay.weight, *args, ops.STE_THRESHOLD, True)

    def run_us(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    nb, m = 2 * (x.numel() + want.numel()), want.numel() * (C // G) * k * k
    result = {"channels": C, "out_channels": Cout, "map": H, "stride": stride, "groups": G, "cin_g": C // G, "cout_g": Cout // G,
              "kernel": k, "dtype": dtype, "bytes": {"fwd": nb, "fwd_bwd": 3 * nb}, "macs": {"fwd": m, "fwd_bwd": 3 * m}}
    leaves["mfma_h_wgrad"], gos["mfma_h_wgrad"], forward["mfma_h_wgrad"] = leaves["mfma_h"], gos["mfma_h"], forward["mfma_h"]
    sides = {"fwd": ("mfma_h", "torch", "mfma_f32"), "fwd_bwd": ("mfma_h", "mfma_h_wgrad", "torch", "mfma_f32"),
             "wgrad": ("mfma_h", "stream_h", "mfma_f32")}
    for mode, make, mult in (("fwd", fwd, 1), ("fwd_bwd", step, 3), ("wgrad", wgrad, 1)):
        fns = {r: switched(make(r), r == "mfma_h_wgrad") for r in sides[mode]}
        for fn in fns.values():
            for _ in range(2):
                fn()
        samples = {r: [] for r in fns}
        for _ in range(rounds):
            for r, fn in fns.items():
                samples[r].append(run_us(fn, 10))
        result[mode] = {r: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                        for r, v in samples.items()}
        floors = {"hbm": mult * nb / B.HBM_BYTES_PER_S, "bf16": 2 * mult * m / BF16_FLOPS}          # wgrad reads |x| + |go| once
        top = max(floors, key=floors.get)
        result[mode]["mfma_h"].update(floor=top, floor_share=round(floors[top] / (result[mode]["mfma_h"]["median_us"] * 1e-6), 3))
    print(json.dumps(result))


def half_passes(s, side="mfma_h"):
    """The rule of ``GROUPED_HALF_MAX_CIN_G``: the step's round range wholly below the library's, the forward median not above it.
    ``side``: the step with the weight-gradient switch at the value it ships with."""
    return (s["fwd_bwd"][side]["max_us"] < s["fwd_bwd"]["torch"]["min_us"]
            and s["fwd"]["mfma_h"]["median_us"] <= s["fwd"]["torch"]["median_us"])


def half_wgrad_passes(s):
    """The rule of ``GROUPED_MFMA_WGRAD``: the step's round range with the switch on wholly below the range with it off."""
    return s["fwd_bwd"]["mfma_h_wgrad"]["max_us"] < s["fwd_bwd"]["mfma_h"]["min_us"]


def main_half(a):
    """Both dtypes on every row of SHAPES the route takes; profiles/grouped_mfma_wgrad_half_bench_line.json."""
    rows = [i for i, (C, _H, _s, G, _k, Cout) in enumerate(SHAPES) if (Cout // G) % 16 == 0]
    shapes = []
    for dtype in (a.dtype if a.dtype != "both" else "bf16,fp16").split(","):
        for i in rows:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), "--rounds", str(a.rounds), "--dtype", dtype],
                               stdout=subprocess.PIPE, text=True, timeout=B.CHILD_LIMIT_S)
            if p.returncode != 0:
                raise SystemExit(f"shape {SHAPES[i]} in {dtype}: the measuring process ended with status {p.returncode}; nothing more was started")
            shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(shapes[-1]), file=sys.stderr)
    from pytorch_quantize_impls_amd.functions import _fused
    line = {"bench": "grouped_mfma_half", "batch": B.BATCH, "rounds": a.rounds, "layout": "NCHW", "hbm_bytes_per_s": B.HBM_BYTES_PER_S,
            "bf16_flops": BF16_FLOPS, "shapes": shapes}
    both = {s["dtype"] for s in shapes} == {"bf16", "fp16"}
    wgrad_on = both and all(half_wgrad_passes(s) for s in shapes)
    side = "mfma_h_wgrad" if wgrad_on else "mfma_h"
    line.update(wgrad_passes_rule=[half_wgrad_passes(s) for s in shapes], grouped_mfma_wgrad_half_by_rule=wgrad_on,
                grouped_mfma_wgrad_half_shipped=bool(_fused.GROUPED_MFMA_WGRAD_HALF), step_side_of_the_half_rule=side,
                shape_passes_rule=[half_passes(s, side) for s in shapes],
                grouped_mfma_half_by_rule=both and all(half_passes(s, side) for s in shapes),
                grouped_mfma_half_shipped=bool(_fused.GROUPED_MFMA_HALF))
    text = json.dumps(line)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(B.ROOT, "profiles", "grouped_mfma_wgrad_half_bench_line.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")
    print(text)


def trace_steps(steps, dtype=None):
    """For ``rocprofv3 --kernel-trace --stats -- python tools/bench_grouped_mfma.py --trace-steps 3``: every row the route takes, in
    one process, ``steps`` training steps with the weight-gradient switch off and then on.  Kernel times instead of wall-time
    differences: the rows differ in their grids, the two sides in the grad_weight kernels' names.  ``dtype`` ("bf16" | "fp16"): the
    layer and the activation in that dtype, the switch ``GROUPED_MFMA_WGRAD_HALF``."""
    import torch
    from pytorch_quantize_impls_amd import ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    dev = torch.device("cuda:0")
    for C, H, stride, G, k, Cout in SHAPES:
        tdt = {None: torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
        layer = BinConv2d(C, Cout, k, stride=stride, padding=k // 2, groups=G).to(dev).to(tdt)
        args = (layer.stride, layer.padding, layer.dilation, G)
        xg = torch.where(torch.rand(B.BATCH, C, H, H) < 0.5, -1.0, 1.0).to(dev).to(tdt).requires_grad_(True)
        if not ops.grouped_mfma_applicable(xg.shape, layer.weight.shape, *args):
            continue
        for on in (False, True):
            _fused.GROUPED_MFMA_WGRAD = _fused.GROUPED_MFMA_WGRAD_HALF = on
            for _ in range(steps):
                y = _fused.GroupedMfmaConv2dFn.apply(xg, layer.weight, layer.bias, "binary", None, ops.STE_THRESHOLD, args)
                y.backward(torch.ones_like(y))
        torch.cuda.synchronize()


def shape_passes(s):
    """None: the route declines the row (it keeps the loop whatever the switch says)."""
    if not s["mfma_takes_it"]:
        return None
    return all(s[m]["mfma"]["max_us"] < s[m]["loop"]["min_us"] for m in ("fwd", "fwd_bwd"))


def wgrad_passes(s, against="mfma"):
    """The step with the matrix-core weight gradient lies wholly below the step of ``against``; None: the route declines the row."""
    if not s["mfma_takes_it"]:
        return None
    return s["fwd_bwd"]["mfma_wgrad"]["max_us"] < s["fwd_bwd"][against]["min_us"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--trace-steps", type=int, default=None)
    ap.add_argument("--dtype", default=None, choices=("bf16", "fp16", "both"),
                    help="the half-precision route against the library's half conv (both: what the switch GROUPED_MFMA_HALF needs)")
    ap.add_argument("--family", default="mfma", choices=("mfma", "wide"),
                    help="wide: the wide-group route (24 ... 64 channels per group) against the per-group loop and the library")
    a = ap.parse_args()
    if a.family == "wide":
        return child_wide(a.child, a.rounds) if a.child is not None else main_wide(a)
    if a.trace_steps is not None:
        return trace_steps(a.trace_steps, a.dtype)
    if a.child is not None:
        return child_half(a.child, a.rounds, a.dtype) if a.dtype else child(a.child, a.rounds)
    if a.dtype:
        return main_half(a)
    shapes = []
    for i in range(len(SHAPES)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), "--rounds", str(a.rounds)],
                           stdout=subprocess.PIPE, text=True, timeout=B.CHILD_LIMIT_S)
        if p.returncode != 0:
            raise SystemExit(f"shape {SHAPES[i]}: the measuring process ended with status {p.returncode}; nothing more was started")
        shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr)
    from pytorch_quantize_impls_amd.functions import _fused
    line = {"bench": "grouped_mfma", "batch": B.BATCH, "rounds": a.rounds, "dtype": "float32", "layout": "NCHW",
            "hbm_bytes_per_s": B.HBM_BYTES_PER_S, "bf16_flops": BF16_FLOPS, "shapes": shapes,
            "shape_passes_rule": [shape_passes(s) for s in shapes], "grouped_mfma_by_rule": all(shape_passes(s) is not False for s in shapes),
            "grouped_mfma_shipped": bool(_fused.GROUPED_MFMA),
            "wgrad_passes_rule": [wgrad_passes(s) for s in shapes], "step_beats_torch": [wgrad_passes(s, "torch") for s in shapes],
            "grouped_mfma_wgrad_by_rule": all(wgrad_passes(s) is not False for s in shapes),
            "grouped_mfma_wgrad_shipped": bool(_fused.GROUPED_MFMA_WGRAD)}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
