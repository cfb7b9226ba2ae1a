#!/usr/bin/env python
"""Depthwise and grouped BinConv2d in bf16 / fp16 at batch 256 on one GPU: the "_h" streaming kernels against what these layers ran
before them, the dense library's half conv.  One JSON line; it decides ``_fused.DEPTHWISE_HALF`` and
``_fused.GROUPED_HALF_MAX_CIN_G`` (DESIGN.md "Half-precision streaming convs").

Shapes: the six depthwise layers of MobileNet-v1 (tools/bench_depthwise.py) and the ResNeXt-style rows of tools/bench_grouped.py
with 4 and 8 channels per group, each as BinConv2d(C, C, k, stride, padding, groups) on +-1 activations, in both half dtypes.

Two ways of running each layer, forward and forward + backward:
  new   : ``_fused.DepthwiseConv2dFn`` / ``GroupedConv2dFn`` called directly on the half tensors (so the measurement does not depend
          on the switches, which are set FROM it): one streaming launch forward, two calls backward;
  torch : what the layer ran before, F.conv2d(x, sign(W), b, groups=G) in the same half dtype through torch (MIOpen).

Method (that of tools/bench_depthwise.py / bench_grouped.py): every shape runs in a child process of its own under a time limit,
one after another, and nothing more is started after a child that fails or overruns.  Inside a child the routes take turns within
each of ``--rounds`` rounds; a round times ``steps`` calls with the host clock around a run that ends in a device synchronise.
Reported per route: the median round and the range of the rounds.

The rules:
  depthwise_half_by_rule          True iff for both dtypes and all six depthwise shapes the new route's forward + backward round
                                  range lies entirely below the library's.
  grouped_half_max_cin_g_by_rule  the largest of 4, 8 such that at it and below, for both dtypes and every measured shape, the
                                  forward + backward round range lies below the library's and the forward median is not above
                                  the library's; 0 when 4 fails.

    python tools/bench_half_streaming.py [--rounds 9] [--out profiles/half_streaming_bench_line.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
os.environ.setdefault("QT_AUTO_GRAPH", "0")

BATCH = 256
#: (family, channels, map, stride, groups, kernel)
SHAPES = ([("depthwise", C, H, s, C, 3) for C, H, s in ((32, 112, 1), (64, 112, 2), (128, 56, 1), (256, 28, 1), (512, 14, 1), (1024, 7, 1))]
          + [("grouped", 128, 56, 1, 32, 3), ("grouped", 256, 28, 1, 32, 3), ("grouped", 256, 56, 2, 32, 3), ("grouped", 128, 28, 1, 16, 1)])
DTYPES = ("bfloat16", "float16")
CIN_G_STEPS = (4, 8)
CHILD_LIMIT_S = 420


def child(index, rounds):
    import torch
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd import _lib, ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    fam, C, H, stride, G, k = SHAPES[index]
    pad = k // 2
    dev = torch.device("cuda:0")
    fn = _fused.DepthwiseConv2dFn if fam == "depthwise" else _fused.GroupedConv2dFn
    stem = "qt_dwconv2d" if fam == "depthwise" else "qt_gconv2d"
    result = {"family": fam, "channels": C, "map": H, "stride": stride, "groups": G, "cin_g": C // G, "kernel": k}
    for name in DTYPES:
        dt = getattr(torch, name)
        torch.manual_seed(index)
        g = torch.Generator().manual_seed(index)
        layer = BinConv2d(C, C, k, stride=stride, padding=pad, groups=G).to(dev)
        layer.weight.data.uniform_(-1.2, 1.2)
        layer = layer.to(dt)
        args = (layer.stride, layer.padding, layer.dilation, G)
        x = torch.where(torch.rand(BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev).to(dt)
        xg = x.clone().requires_grad_(True)

        def new(inp):
            return fn.apply(inp, layer.weight, layer.bias, "binary", None, ops.STE_THRESHOLD, args)

        with torch.no_grad():
            y0 = new(x)
        go = torch.randn(y0.shape, generator=g).to(dev).to(dt)

        def new_fwd():
            with torch.no_grad():
                return new(x)

        def new_fb():
            new(xg).backward(go)

        def sign_w():
            w = layer.weight.detach()
            return torch.where(w < 0, -1.0, 1.0).to(dt)

        def torch_fwd():
            with torch.no_grad():
                return F.conv2d(x, sign_w(), layer.bias, stride, pad, 1, G)

        def torch_fb():
            wq = sign_w().requires_grad_(True)
            F.conv2d(xg, wq, layer.bias, stride, pad, 1, G).backward(go)

        fns = {"fwd": {"new": new_fwd, "torch": torch_fwd}, "fwd_bwd": {"new": new_fb, "torch": torch_fb}}
        # the two routes compute the same conv: an integer sum plus the bias, rounded to the dtype (the library in its own order)
        a, b = new_fwd().float(), torch_fwd().float()
        assert torch.allclose(a, b, rtol=2.0 ** -6, atol=2.0 ** -6), float((a - b).abs().max())
        calls = dict(_lib.call_counts)
        new_fb()
        used = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
        assert used == {stem + "_h": 1, stem + "_grad_input_h": 1, stem + "_grad_weight_h": 1}, used

        def run_us(f, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / steps

        out = {}
        for mode, routes in fns.items():
            for f in routes.values():
                for _ in range(2):
                    f()
                    xg.grad = None
            samples = {r: [] for r in routes}
            for _ in range(rounds):
                for r, f in routes.items():
                    samples[r].append(run_us(f, 10))
                    xg.grad = None
                    layer.zero_grad(set_to_none=True)
            out[mode] = {r: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                         for r, v in samples.items()}
        result[name] = out
        del layer, x, xg, go, y0
        torch.cuda.empty_cache()
    print(json.dumps(result))


def step_below(s, name):
    """The new route's forward + backward round range lies entirely below the library's."""
    fb = s[name]["fwd_bwd"]
    return fb["new"]["max_us"] < fb["torch"]["min_us"]


def forward_not_above(s, name):
    fw = s[name]["fwd"]
    return fw["new"]["median_us"] <= fw["torch"]["median_us"]


def depthwise_by_rule(shapes):
    mine = [s for s in shapes if s["family"] == "depthwise"]
    return bool(mine) and all(step_below(s, n) for s in mine for n in DTYPES)


def grouped_max_cin_g_by_rule(shapes):
    top = 0
    for cin_g in CIN_G_STEPS:
        mine = [s for s in shapes if s["family"] == "grouped" and s["cin_g"] == cin_g]
        if not mine or not all(step_below(s, n) and forward_not_above(s, n) for s in mine for n in DTYPES):
            break
        top = cin_g
    return top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_streaming_bench_line.json"))
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.rounds)
    shapes = []
    for i in range(len(SHAPES)):
        # a child per shape, each under its own limit; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), "--rounds", str(a.rounds)],
                           stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            raise SystemExit(f"shape {SHAPES[i]}: the measuring process ended with status {p.returncode}; nothing more was started")
        shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr)
    line = {"bench": "half_streaming", "batch": BATCH, "rounds": a.rounds, "dtypes": list(DTYPES), "layout": "NCHW", "shapes": shapes,
            "step_below_library": {n: [step_below(s, n) for s in shapes] for n in DTYPES},
            "forward_not_above_library": {n: [forward_not_above(s, n) for s in shapes] for n in DTYPES},
            "depthwise_half_by_rule": depthwise_by_rule(shapes), "grouped_half_max_cin_g_by_rule": grouped_max_cin_g_by_rule(shapes),
            "not_measured": ["hardware counters", "batch sizes other than 256", "a whole model", "channels-last activations"]}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
