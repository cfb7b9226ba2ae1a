#!/usr/bin/env python
"""Elastic / WQR loss-aware quantisation on the GPU: one JSON line.

  * the fused regulariser (g - lin_l2 - lin_l1 and g - exp_l2 - exp_l1, size 5) and the projections on an 8192 x 8192 weight
    (256 MiB per tensor: 768 MiB per regulariser pass, 512 MiB per projection, well past the L3), as us and TB/s;
  * the same computations as the reference's torch operation sequence (reg_torch / the repeat-abs-argmin-gather projection);
  * one training step and one eval forward of a loss_quant_lin_convert-ed MLP 784-2048-2048-10 at batch 256, with the HIP
    kernels and with the reference's sequences for the regulariser and the projection (the GEMMs are the same in both).

    python tools/bench_elastic.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from pytorch_quantize_impls_amd import utils  # noqa: E402
from pytorch_quantize_impls_amd.functions import elastic_quant_connect as EQ  # noqa: E402


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


def proj_reference(w, levels):
    """The reference's _proj_val sequence: repeat, permute, subtract, abs, argmin, gather."""
    s = torch.tensor(levels, device=w.device)
    x = w.repeat((s.size()[0],) + (1,) * w.dim())
    x = x.permute(*(tuple(range(x.dim()))[1:] + (0,)))
    return s[torch.argmin(torch.abs(x - s), dim=x.dim() - 1)]


class _RefKernels:
    """Swap the two kernels for the reference's torch sequences inside the functions module (for the 'both ways' step)."""

    def __enter__(self):
        self.saved = (EQ.regularised_grad, EQ.project)
        EQ.regularised_grad = lambda g, w, t1, a1, t2, a2: (g - EQ.reg_torch(w, t1, a1)) - EQ.reg_torch(w, t2, a2)
        EQ.project = lambda w, levels: proj_reference(w, levels)
        return self

    def __exit__(self, *exc):
        EQ.regularised_grad, EQ.project = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    n = 8192
    w = torch.randn(n, n, device=dev) * 0.6
    g = torch.randn(n, n, device=dev) * 0.01
    alpha, beta = torch.tensor([0.03], device=dev), torch.tensor([0.01], device=dev)
    mib = n * n * 4 / 2 ** 20
    res = {"what": "elastic/WQR kernels, MI355X", "weight": [n, n]}

    cases = {"reg_lin": (EQ.lin_l2_terms("tensor", 1, -1, 5), EQ.lin_l1_terms(1, -1, 5)),
             "reg_exp": (EQ.exp_l2_terms(2, 0.25, 5), EQ.exp_l1_terms(2, 0.25, 5))}
    for name, (t1, t2) in cases.items():
        us = timed(lambda: EQ.regularised_grad(g, w, t1, alpha, t2, beta), args.iters)
        ref = timed(lambda: (g - EQ.reg_torch(w, t1, alpha)) - EQ.reg_torch(w, t2, beta), max(3, args.iters // 4), warmup=1)
        res[name] = {"terms": int(len(t1) + len(t2)), "us": round(us, 1), "TBps": round(3 * mib * 2 ** 20 / us / 1e6, 2),
                     "reference_us": round(ref, 1), "speedup": round(ref / us, 1)}
    for name, levels in (("proj_lin", EQ.lin_levels(1, -1, 5)), ("proj_exp", EQ.exp_levels(2, 0.25, 5))):
        us = timed(lambda: EQ.project(w, levels), args.iters)
        ref = timed(lambda: proj_reference(w, levels), max(3, args.iters // 4), warmup=1)
        res[name] = {"levels": len(levels), "us": round(us, 1), "TBps": round(2 * mib * 2 ** 20 / us / 1e6, 2),
                     "reference_us": round(ref, 1), "speedup": round(ref / us, 1)}
    del w, g
    torch.cuda.empty_cache()

    mlp = torch.nn.Sequential(torch.nn.Linear(784, 2048), torch.nn.ReLU(), torch.nn.Linear(2048, 2048), torch.nn.ReLU(),
                              torch.nn.Linear(2048, 10))
    net = utils.loss_quant_lin_convert(mlp, alpha=0.03, beta=0.01).to(dev)
    x = torch.randn(256, 784, device=dev)
    t = torch.randint(0, 10, (256,), device=dev)

    def step():
        net.zero_grad(set_to_none=False)
        F.cross_entropy(net(x), t).backward()

    def eval_fwd():
        for m in net:
            if hasattr(m, "reset_quant_cache"):
                m.reset_quant_cache()             # a fresh weight version each call: projection + GEMM
        with torch.no_grad():
            net(x)

    net.train()
    res["mlp_train_step_us"] = round(timed(step, args.iters), 1)
    with _RefKernels():
        res["mlp_train_step_reference_ops_us"] = round(timed(step, args.iters), 1)
    net.eval()
    res["mlp_eval_forward_us"] = round(timed(eval_fwd, args.iters), 1)
    with _RefKernels():
        res["mlp_eval_forward_reference_ops_us"] = round(timed(eval_fwd, args.iters), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
