#!/usr/bin/env python
"""Lin / Log fixed-point training step on the GPU: one JSON line.

A VGG-style CIFAR-10 net shaped like the reference's models/samples/VGG16_LinLogQuant.py (six 3 x 3 QuantConv2d 3-64-64-128-128-
256-256 with BatchNorm, ReLU, MaxPool and the nnQuant(fsr=1, bit_width=8, with_sign=False) activation quantiser; LinearQuant
4096-1024-1024-10), batch 256, weight fsr 2 (convs) / 1 (linears), for dtype lin (bit_width 8) and log (bit_width 3).  A step is
forward, NLL loss, backward, SGD step and clamp().  Measured two ways on the same module:
  * this package's route (functions/_fused.py LogLinConv2dFn / LogLinLinearFn: one quantise-and-pack launch per layer, matrix-core
    forward and grad_x, six-term grad_W);
  * the reference's op sequence: F.conv2d / F.linear on the quantised weight (the weight quantiser is still this package's
    kernel, so the difference is the contraction and its backward: the dense library against the routes above).
Also the time of the quantise-and-pack launches of one step on their own.

    python tools/bench_loglin_train.py [--iters 20] [--batch 256] [--out profiles/loglin_train_bench_line.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from pytorch_quantize_impls_amd import ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import log_lin_connect  # noqa: E402
from pytorch_quantize_impls_amd.layers import LinearQuant, QuantConv2d  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


class VGGLinLog(torch.nn.Module):
    def __init__(self, dtype="lin", bits=8):
        super().__init__()
        self.quant_act = log_lin_connect.nnQuant(fsr=1, bit_width=8, with_sign=False)
        chans = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256)]
        self.convs = torch.nn.ModuleList(QuantConv2d(a, b, 3, padding=1, fsr=2, bit_width=bits, dtype=dtype) for a, b in chans)
        self.bns = torch.nn.ModuleList(torch.nn.BatchNorm2d(b) for _, b in chans)
        self.lins = torch.nn.ModuleList([LinearQuant(4096, 1024, fsr=1, bit_width=bits, dtype=dtype),
                                         LinearQuant(1024, 1024, fsr=1, bit_width=bits, dtype=dtype),
                                         LinearQuant(1024, 10, fsr=1, bit_width=bits, dtype=dtype)])
        self.bn1d = torch.nn.ModuleList([torch.nn.BatchNorm1d(1024), torch.nn.BatchNorm1d(1024)])

    def clamp(self):
        for m in list(self.convs) + list(self.lins):
            m.clamp()

    def forward(self, x):
        for i, (conv, bn) in enumerate(zip(self.convs, self.bns)):
            x = self.quant_act(F.relu(bn(conv(x))))
            if i % 2 == 1:
                x = F.max_pool2d(x, 2)
        x = x.flatten(1)
        for lin, bn in zip(self.lins[:2], self.bn1d):
            x = self.quant_act(F.relu(bn(lin(x))))
        return F.log_softmax(self.lins[2](x), 1)


class ReferenceOps:
    """Inside the block the two layer classes run the reference's forward: F.conv2d / F.linear(x, Q(W), b)
    (layers/log_lin_layers.py of the reference), autograd deriving the backward on the dense library."""

    def __enter__(self):
        self.saved = (QuantConv2d.forward, LinearQuant.forward)

        def conv_fwd(m, x):
            return F.conv2d(x, m.weight_op(m.weight), m.bias, m.stride, m.padding, m.dilation, m.groups)

        def lin_fwd(m, x):
            return F.linear(x, m.weight_op(m.weight), m.bias)
        QuantConv2d.forward, LinearQuant.forward = conv_fwd, lin_fwd
        return self

    def __exit__(self, *exc):
        QuantConv2d.forward, LinearQuant.forward = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"what": "Lin/Log VGG16-style CIFAR-10 training step, MI355X", "batch": args.batch}
    for dtype, bits in (("lin", 8), ("log", 3)):
        torch.manual_seed(0)
        net = VGGLinLog(dtype, bits).to(dev)
        opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
        x = torch.randn(args.batch, 3, 32, 32, device=dev)
        t = torch.randint(0, 10, (args.batch,), device=dev)

        def step():
            opt.zero_grad(set_to_none=False)
            F.nll_loss(net(x), t).backward()
            opt.step()
            net.clamp()

        layers = list(net.convs) + list(net.lins)

        def packs():
            for m in layers:
                ops.pack_levels_bf16x3(m.weight, dtype, m.fsr, bits, grad_x=m is not net.convs[0])

        hip = timed(step, args.iters)
        with ReferenceOps():
            ref = timed(step, args.iters)
        pack = timed(packs, args.iters)
        res[dtype] = {"bit_width": bits, "step_us": round(hip, 1), "reference_ops_step_us": round(ref, 1),
                      "speedup": round(ref / hip, 2), "pack_us_per_step": round(pack, 1), "pack_launches_per_step": len(layers)}
        print(f"[{dtype}] step {hip:.1f} us (median of {args.iters}), reference ops {ref:.1f} us, x{ref / hip:.2f}; "
              f"quantise-and-pack {pack:.1f} us per step ({len(layers)} launches)", file=sys.stderr)
        del net, opt
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
