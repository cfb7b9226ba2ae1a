#!/usr/bin/env python
"""A whole training step as one hipGraph replay, on one GPU: one JSON line.

Two forms of the same step — forward, loss, backward, optimizer.step(), model.clamp() — on the same model, batch and optimiser:

  outside : utils.GraphedTrainStep(model, loss, x, t) replays forward + loss + backward, then utils.FusedQuantSGD / FusedQuantAdam
            .step() runs eagerly (walks the parameter groups, builds the descriptor table, launches).
  captured: utils.GraphedTrainStep(model, loss, x, t, optimizer=opt): the update is part of the graph; before a replay the host
            writes the step's scalars (learning rate / Adam's bias corrections) to device memory.

on bench_models.DorefaResNet18(w_bits=1, a_bits=4) at 32 x 32, batch 256; bench_models.AlexNetBin at batch 256; a 784-256-10 binary
MLP at batch 64 (+-1 inputs); each with SGD (momentum 0.9) and Adam.  A step is timed with the host clock around a run of steps
that ends in a device synchronise, so host and launch overhead count.  Both forms are measured in the same process in alternating
rounds; the figure is the median round.  The implicit hipGraphs are switched off (QT_AUTO_GRAPH=0).  Every step trains on the
same random batch.  A replayed step answers the range questions of un-tagged activations from the verdicts remembered at capture;
with the default ``recover=False`` — the two forms compared here — it turns its output into NaN when training has made one wrong
(GraphedTrainStep's docstring), in either form alike.  The DoReFa ResNet on a random batch gets there within a dozen steps at
ordinary learning rates, so THIS comparison times it at 1e-6; the line says per form whether the loss was still finite after the
last timed step (``loss_finite``) and which learning rate was used (``lr``).  At 1e-6 SGD stays finite and Adam, whose update has
the size of the learning rate whatever the gradient's, does not: its ResNet entry in profiles/graphed_step_bench_line.json compares
rounds on NaN values.  What a training step of that net costs at an ordinary learning rate is measured by the ``--recover`` leg.

``--recover`` measures what surviving a wrong verdict costs and buys (profiles/graph_recover_bench_line.json):

  * per net and optimiser, the captured step as above against the same step with ``recover=True`` (guard, buffer snapshot, flag OR,
    guard copy, one step of run-ahead), alternating, on a batch where nothing flips: medians, round ranges, and by how much the
    ``recover=True`` median lies outside the captured form's round range (0 when inside);
  * the DoReFa ResNet with Adam at lr 1e-3, where the step without recovery goes non-finite: ``loss_finite``, ``recoveries``,
    ``recaptures`` and the median step time of the ``recover=True`` step, next to the ``recover=False`` step at the same rate.

    python tools/bench_graphed_step.py [--rounds 9] [--steps 20] [--nets resnet18,alexnet,mlp] [--out profiles/graphed_step_bench_line.json]
    python tools/bench_graphed_step.py --recover [--out profiles/graph_recover_bench_line.json]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("QT_AUTO_GRAPH", "0")

import torch  # noqa: E402

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
import bench_models  # noqa: E402
from pytorch_quantize_impls_amd import _lib, utils  # noqa: E402


def run_us(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def alternate(fns, rounds, steps):
    """Median over the rounds of the per-call time of each function, the functions taking turns within a round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(run_us(fn, steps))
    return {k: round(sorted(v)[len(v) // 2], 1) for k, v in samples.items()}, {k: [round(x, 1) for x in v] for k, v in samples.items()}


def _mlp():
    net = torch.nn.Sequential(torch.nn.Linear(784, 256), torch.nn.BatchNorm1d(256), torch.nn.Hardtanh(), torch.nn.Linear(256, 10))
    return utils.binary_net_convert(net)


def nets(dev):
    """name -> (model factory, input factory, loss, learning rate)."""
    ce = torch.nn.functional.cross_entropy

    yield "dorefa_resnet18_32x32_b256", (lambda: bench_models.DorefaResNet18(w_bits=1, a_bits=4),
                                         lambda: torch.randn(256, 3, 32, 32, device=dev), ce, 1e-6), "resnet18"
    yield "alexnet_bin_b256", (bench_models.AlexNetBin, lambda: torch.randn(256, 3, 224, 224, device=dev),
                               torch.nn.functional.nll_loss, 1e-3), "alexnet"
    yield "binary_mlp_784_256_10_b64", (_mlp, lambda: (torch.randint(0, 2, (64, 784), device=dev) * 2 - 1).float(), ce, 1e-3), "mlp"


OPTIMISERS = {"sgd": (utils.FusedQuantSGD, dict(momentum=0.9, weight_decay=1e-4)),
              "adam": (utils.FusedQuantAdam, dict())}


def bench_net(dev, make, make_x, loss_fn, lr, rounds, steps):
    res = {"lr": lr}
    for oname, (Fused, hp) in OPTIMISERS.items():
        hp = dict(hp, lr=lr)
        torch.manual_seed(0)
        a = make().to(dev).train()
        torch.manual_seed(0)
        b = make().to(dev).train()
        torch.manual_seed(1)
        x, t = make_x(), torch.randint(0, 10, (make_x().shape[0],), device=dev)
        opt_a, opt_b = Fused(a, **hp), Fused(b, **hp)
        outside_step = utils.GraphedTrainStep(a, loss_fn, x, t)
        captured_step = utils.GraphedTrainStep(b, loss_fn, x, t, optimizer=opt_b)

        def outside():
            outside_step(x, t)
            opt_a.step()

        def captured():
            captured_step(x, t)

        before = dict(_lib.call_counts)
        med, raw = alternate({"outside": outside, "captured": captured}, rounds, steps)
        calls = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if k.startswith("qt_optim_") and v != before.get(k, 0)}
        finite = {"outside": bool(torch.isfinite(outside_step(x, t))), "captured": bool(torch.isfinite(captured_step(x, t)))}
        res[oname] = {"outside_us": med["outside"], "captured_us": med["captured"],
                      "saved_us": round(med["outside"] - med["captured"], 1), "speedup": round(med["outside"] / med["captured"], 3),
                      "outside_rounds_us": raw["outside"], "captured_rounds_us": raw["captured"],
                      # host-side entry calls per step: the outside form's update launch, the captured form's scalar write
                      "entry_calls_per_step": {k: v / (rounds * steps + 3) for k, v in calls.items()}, "loss_finite": finite}
        del a, b, opt_a, opt_b, outside_step, captured_step
        torch.cuda.empty_cache()
    res["parameter_tensors"] = len(list(make().parameters()))
    return res


def _outside(median, rounds_us):
    """How far ``median`` lies outside [min, max] of ``rounds_us`` (us; 0.0 inside, negative below)."""
    lo, hi = min(rounds_us), max(rounds_us)
    return round(median - hi, 1) if median > hi else (round(median - lo, 1) if median < lo else 0.0)


def bench_recover_net(dev, make, make_x, loss_fn, lr, rounds, steps):
    """The captured step (``recover=False``: the step as it was) against ``recover=True`` on a batch where no verdict flips."""
    res = {"lr": lr}
    for oname, (Fused, hp) in OPTIMISERS.items():
        hp = dict(hp, lr=lr)
        torch.manual_seed(0)
        a = make().to(dev).train()
        torch.manual_seed(0)
        b = make().to(dev).train()
        torch.manual_seed(1)
        x, t = make_x(), torch.randint(0, 10, (make_x().shape[0],), device=dev)
        plain = utils.GraphedTrainStep(a, loss_fn, x, t, optimizer=Fused(a, **hp))
        rec = utils.GraphedTrainStep(b, loss_fn, x, t, optimizer=Fused(b, **hp), recover=True)
        med, raw = alternate({"captured": lambda: plain(x, t), "recover": lambda: rec(x, t)}, rounds, steps)
        rec.settle()
        res[oname] = {"captured_us": med["captured"], "recover_us": med["recover"], "cost_us": round(med["recover"] - med["captured"], 1),
                      "captured_rounds_us": raw["captured"], "recover_rounds_us": raw["recover"],
                      "recover_outside_captured_range_us": _outside(med["recover"], raw["captured"]),
                      "trusted_flags": len(rec._flags) if rec._flags is not None else 0, "recoveries": rec.recoveries,
                      "recaptures": rec.recaptures,
                      "loss_finite": {"captured": bool(torch.isfinite(plain(x, t))), "recover": bool(torch.isfinite(rec(x, t)))}}
        del a, b, plain, rec
        torch.cuda.empty_cache()
    return res


def bench_flip(dev, rounds, steps, lr=1e-3):
    """DoReFa ResNet-18 W1A4, 32 x 32, batch 256, Adam at an ordinary learning rate: training moves the activations out of the
    ranges remembered at capture.  One form after the other (each trains its own model from the same start)."""
    res = {"lr": lr, "optimiser": "adam"}
    for form, recover in (("recover", True), ("captured", False)):
        torch.manual_seed(0)
        m = bench_models.DorefaResNet18(w_bits=1, a_bits=4).to(dev).train()
        torch.manual_seed(1)
        x, t = torch.randn(256, 3, 32, 32, device=dev), torch.randint(0, 10, (256,), device=dev)
        step = utils.GraphedTrainStep(m, torch.nn.functional.cross_entropy, x, t, optimizer=utils.FusedQuantAdam(m, lr=lr),
                                      recover=recover)
        samples = [run_us(lambda: step(x, t), steps) for _ in range(rounds)]
        loss = step(x, t)
        if recover:
            step.settle()
        params_finite = all(bool(torch.isfinite(p).all()) for p in m.parameters())
        res[form] = {"step_us": round(sorted(samples)[len(samples) // 2], 1), "rounds_us": [round(v, 1) for v in samples],
                     "loss_finite": bool(torch.isfinite(loss)), "parameters_finite": params_finite, "loss": float(loss),
                     "recoveries": step.recoveries, "recaptures": step.recaptures, "steps": rounds * steps + 1}
        del m, step
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recover", action="store_true", help="measure GraphedTrainStep(recover=True) instead (see the module docstring)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nets", default="resnet18,alexnet,mlp")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "graph_recover_bench_line.json" if args.recover else "graphed_step_bench_line.json")
    wanted = set(args.nets.split(","))
    if not torch.cuda.is_available():
        raise SystemExit("bench_graphed_step.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    name, cus = _lib.device_info()
    line = {"what": "one training step (forward, loss, backward, fused update + clamp): GraphedTrainStep replay + eager FusedQuant*.step() "
                    "vs GraphedTrainStep(optimizer=...) with the update inside the graph; host clock, us per step, median round",
            "device": name, "rounds": args.rounds, "steps_per_round": args.steps, "nets": {}}
    if args.recover:
        line["what"] = ("one training step as one hipGraph replay, GraphedTrainStep(optimizer=...): recover=False (the step as it was) vs "
                        "recover=True on a batch where no verdict flips; then DoReFa ResNet-18 with Adam at lr 1e-3, where verdicts do "
                        "flip; host clock, us per step, median round")
    for key, (make, make_x, loss_fn, lr), short in nets(dev):
        if short in wanted:
            bench = bench_recover_net if args.recover else bench_net
            line["nets"][key] = bench(dev, make, make_x, loss_fn, lr, args.rounds, args.steps)
    if args.recover and "resnet18" in wanted:
        line["dorefa_resnet18_32x32_b256_adam_lr1e-3"] = bench_flip(dev, args.rounds, args.steps)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
