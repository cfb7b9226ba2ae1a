#!/usr/bin/env python
"""The grouped layers of ResNeXt-50 (32 groups) at batch 256 as BinConv2d(C, C, 3, stride, padding=1, groups=G), one layer at 24
channels per group and one grouped 1 x 1 layer, on one GPU: one JSON line.

Three ways of running each layer, forward and forward + backward, on +-1 activations:
  new   : ``_fused.GroupedConv2dFn`` called directly (so the measurement does not depend on ``GROUPED_MAX_CIN_G``, which is set
          FROM it) — one streaming launch forward and two calls backward (csrc/gconv.hip);
  loop  : the route before the grouped kernels, ``_fused.grouped_quant_conv`` called directly with ``binary_input = True`` (one fp4
          implicit-GEMM conv per group on copied slices, told that the activation is +-1 so that it does not stop to detect it);
  torch : what DorefaConv2d did before and what a user would write, F.conv2d(x, sign(W), b, groups=G) through torch (MIOpen).

Method (that of tools/bench_depthwise.py): every shape runs in a child process of its own under a time limit, and nothing more is
started after a child that fails or overruns.  Inside a child the routes take turns within each of ``--rounds`` rounds; a round times
``steps`` calls with the host clock around a run that ends in a device synchronise.  Reported per route: the median round and the
range of the rounds.  ``bytes`` is what the algorithm has to move (fp32: x and y once forward; x, y, grad_x and grad_y three times
in all forward + backward; the weights are noise) and ``macs`` the multiply-adds (three convs' worth forward + backward);
``hbm_share`` = (bytes / 8 TB/s) / median time of the new route, ``vector_share`` = (2 macs / 157 TFLOP/s) / the same, and
``bound`` names the larger of the two floors.

``grouped_max_cin_g_by_rule`` is the value ``_fused.GROUPED_MAX_CIN_G`` has to ship with: the largest measured cin_g of 4, 8, 16, 24
such that at it and at every smaller one, on every shape, the new route's round range lies below the loop's AND below the
library's forward + backward, and its forward range does not lie wholly above the range of the better (lower median) of the two;
1 (routing off) when 4 fails.

    python tools/bench_grouped.py [--rounds 9] [--out profiles/grouped_bench_line.json]
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
#: (channels, map, stride, groups, kernel): the 3 x 3 layers of ResNeXt-50 32x4d at 224 x 224 (stages 1-3 and the strided layer
#: that opens stage 3), 24 channels per group, a grouped 1 x 1
SHAPES = [(128, 56, 1, 32, 3), (256, 28, 1, 32, 3), (512, 14, 1, 32, 3), (256, 56, 2, 32, 3), (768, 14, 1, 32, 3), (128, 28, 1, 16, 1)]
CIN_G_STEPS = (4, 8, 16, 24)
HBM_BYTES_PER_S = 8e12
VECTOR_FLOPS = 157e12
CHILD_LIMIT_S = 420


def counts(C, H, stride, G, k):
    pad = k // 2
    Ho = (H + 2 * pad - k) // stride + 1
    x, y = 4 * BATCH * C * H * H, 4 * BATCH * C * Ho * Ho
    macs = BATCH * C * Ho * Ho * (C // G) * k * k
    return {"fwd": x + y, "fwd_bwd": 3 * (x + y)}, {"fwd": macs, "fwd_bwd": 3 * macs}


def child(index, rounds):
    import torch
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd import _lib, ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import BinConv2d

    C, H, stride, G, k = SHAPES[index]
    pad = k // 2
    dev = torch.device("cuda:0")
    torch.manual_seed(index)
    g = torch.Generator().manual_seed(index)
    layer = BinConv2d(C, C, k, stride=stride, padding=pad, groups=G).to(dev)
    layer.weight.data.uniform_(-1.2, 1.2)
    layer.binary_input = True
    args = (layer.stride, layer.padding, layer.dilation, G)
    x = torch.where(torch.rand(BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev)
    xg = x.clone().requires_grad_(True)

    def new(inp):
        return _fused.GroupedConv2dFn.apply(inp, layer.weight, layer.bias, "binary", None, ops.STE_THRESHOLD, args)

    with torch.no_grad():
        y0 = new(x)
    go = torch.randn(y0.shape, generator=g).to(dev)

    def new_fwd():
        with torch.no_grad():
            return new(x)

    def new_fb():
        new(xg).backward(go)

    def loop_fwd():
        with torch.no_grad():
            return _fused.grouped_quant_conv(layer, x, "binary", layer._op)

    def loop_fb():
        _fused.grouped_quant_conv(layer, xg, "binary", layer._op).backward(go)

    def torch_fwd():
        with torch.no_grad():
            return F.conv2d(x, torch.where(layer.weight < 0, -1.0, 1.0), layer.bias, stride, pad, 1, G)

    def torch_fb():
        wq = torch.where(layer.weight.detach() < 0, -1.0, 1.0).requires_grad_(True)
        F.conv2d(xg, wq, layer.bias, stride, pad, 1, G).backward(go)

    fns = {"fwd": {"new": new_fwd, "loop": loop_fwd, "torch": torch_fwd}, "fwd_bwd": {"new": new_fb, "loop": loop_fb, "torch": torch_fb}}
    # the three routes compute the same conv: integer sums plus the bias (the library's algorithm is its own choice)
    assert torch.allclose(new_fwd(), torch_fwd(), rtol=0, atol=1e-4)
    assert torch.equal(new_fwd(), loop_fwd())
    calls = dict(_lib.call_counts)
    new_fb()
    used = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    assert used == {"qt_gconv2d_f32": 1, "qt_gconv2d_grad_input_f32": 1, "qt_gconv2d_grad_weight_f32": 1}, used

    def run_us(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps

    nbytes, macs = counts(C, H, stride, G, k)
    result = {"channels": C, "map": H, "stride": stride, "groups": G, "cin_g": C // G, "kernel": k, "bytes": nbytes, "macs": macs}
    for mode, routes in fns.items():
        steps = {r: (2 if r == "loop" else 10) for r in routes}
        for r, fn in routes.items():
            for _ in range(2):
                fn()
                xg.grad = None
        samples = {r: [] for r in routes}
        for _ in range(rounds):
            for r, fn in routes.items():
                samples[r].append(run_us(fn, steps[r]))
                xg.grad = None
                layer.zero_grad(set_to_none=True)
        result[mode] = {r: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                        for r, v in samples.items()}
        t = result[mode]["new"]["median_us"] * 1e-6
        hbm, vec = nbytes[mode] / HBM_BYTES_PER_S / t, 2 * macs[mode] / VECTOR_FLOPS / t
        result[mode]["new"].update(hbm_share=round(hbm, 3), vector_share=round(vec, 3), bound="compute" if vec > hbm else "memory")
    print(json.dumps(result))


def shape_passes(s):
    """The rule for one shape: a step below both other routes with disjoint ranges; the forward not wholly above the better one."""
    fb, fw = s["fwd_bwd"], s["fwd"]
    step = fb["new"]["max_us"] < fb["loop"]["min_us"] and fb["new"]["max_us"] < fb["torch"]["min_us"]
    better = min(("loop", "torch"), key=lambda r: fw[r]["median_us"])
    return step and not fw["new"]["min_us"] > fw[better]["max_us"]


def max_cin_g_by_rule(shapes):
    top = 1
    for cin_g in CIN_G_STEPS:
        mine = [s for s in shapes if s["cin_g"] == cin_g]
        if not mine or not all(shape_passes(s) for s in mine):
            break
        top = cin_g
    return top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_bench_line.json"))
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
    from pytorch_quantize_impls_amd.functions import _fused
    line = {"bench": "grouped_resnext50", "batch": BATCH, "rounds": a.rounds, "dtype": "float32", "layout": "NCHW",
            "hbm_bytes_per_s": HBM_BYTES_PER_S, "vector_flops": VECTOR_FLOPS, "shapes": shapes,
            "shape_passes_rule": [shape_passes(s) for s in shapes],
            "grouped_max_cin_g_by_rule": max_cin_g_by_rule(shapes), "grouped_max_cin_g_shipped": _fused.GROUPED_MAX_CIN_G}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
