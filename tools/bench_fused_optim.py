#!/usr/bin/env python
"""The fused training update on one GPU: one JSON line.

(a) optimizer.step() + model.clamp().  The parent sequence — torch.optim.SGD / torch.optim.Adam (default implementation) followed
    by utils.clamp_weights_ — against utils.FusedQuantSGD / FusedQuantAdam (one multi-tensor launch sequence per parameter group,
    clamp folded in, nibble planes of the LinearBin weights written in the same pass) on three parameter sets: BinaryNet-AlexNet
    and DoReFa ResNet-18 (bench_models.py) and one LinearBin(4096, 4096).  Gradients are fixed random tensors; a step is timed
    with the host clock around a run of steps that ends in a device synchronise, so launch and host overhead count.
(b) LinearBin(4096, 4096).train()(x) at batch 4096 (+-1 input) with the plane the fused step left behind and without it
    (a twin layer with the same weight and no record: it packs both operands).

Both sides of a comparison are measured in the same process in alternating rounds; the figure is the median round.  The
implicit hipGraphs are switched off (QT_AUTO_GRAPH=0) so that every call launches what it launches.

    python tools/bench_fused_optim.py [--rounds 9] [--steps 20] [--out profiles/fused_optim_bench_line.json]

--clip measures gradient-norm clipping instead, same protocol, same three parameter sets: what a user does without it —
torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True) followed by the unclipped FusedQuant*.step() — against the
clipped fused step (max_grad_norm=), with the unclipped fused step alongside so that the cost of the norm pass itself shows.

    python tools/bench_fused_optim.py --clip [--out profiles/fused_clip_bench_line.json]
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
from pytorch_quantize_impls_amd.layers import LinearBin  # noqa: E402


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


def param_sets(dev):
    yield "alexnet_bin", lambda: bench_models.AlexNetBin().to(dev).train()
    yield "dorefa_resnet18", lambda: bench_models.DorefaResNet18().to(dev).train()
    yield "linear_bin_4096", lambda: LinearBin(4096, 4096).to(dev).train()


def set_grads(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g, device=p.device) * 1e-2


def bench_steps(dev, rounds, steps):
    out = {}
    variants = {"sgd": (torch.optim.SGD, utils.FusedQuantSGD, dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)),
                "adam": (torch.optim.Adam, utils.FusedQuantAdam, dict(lr=1e-3))}
    for name, make in param_sets(dev):
        res = {}
        for vname, (Ref, Fused, hp) in variants.items():
            torch.manual_seed(0)
            a = make()
            torch.manual_seed(0)
            b = make()
            set_grads(a, 1)
            set_grads(b, 1)
            ref, fused = Ref(a.parameters(), **hp), Fused(b, **hp)

            def parent():
                ref.step()
                utils.clamp_weights_(a)

            before = dict(_lib.call_counts)
            med, raw = alternate({"parent": parent, "fused": fused.step}, rounds, steps)
            launches = sum(v - before.get(k, 0) for k, v in _lib.call_counts.items() if k.startswith("qt_optim_"))
            res[vname] = {"parent_us": med["parent"], "fused_us": med["fused"], "speedup": round(med["parent"] / med["fused"], 2),
                          "parent_rounds_us": raw["parent"], "fused_rounds_us": raw["fused"],
                          "fused_entry_calls_per_step": launches / (rounds * steps + 3)}        # (+ 3 warm-up steps)
            del a, b, ref, fused
        n = sum(p.numel() for p in make().parameters())
        res["parameters"] = n
        out[name] = res
    return out


def bench_clip(dev, rounds, steps, max_norm=1.0):
    out = {}
    variants = {"sgd": (utils.FusedQuantSGD, dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)), "adam": (utils.FusedQuantAdam, dict(lr=1e-3))}
    for name, make in param_sets(dev):
        res = {}
        for vname, (Fused, hp) in variants.items():
            models = []
            for _ in range(3):
                torch.manual_seed(0)
                models.append(make())
                set_grads(models[-1], 1)
            a, b, c = models
            base, clipped, plain = Fused(a, **hp), Fused(b, max_grad_norm=max_norm, **hp), Fused(c, **hp)
            params = [p for p in a.parameters() if p.grad is not None]

            def torch_clip_then_fused():
                torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)      # rewrites the gradients in place
                base.step()

            med, raw = alternate({"torch_clip_then_fused": torch_clip_then_fused, "fused_clip": clipped.step, "fused_unclipped": plain.step},
                                 rounds, steps)
            assert float(clipped.clip_coef) < 1.0, "the clip does not act: the comparison would time a no-op"
            res[vname] = {"torch_clip_then_fused_us": med["torch_clip_then_fused"], "fused_clip_us": med["fused_clip"],
                          "fused_unclipped_us": med["fused_unclipped"],
                          "speedup": round(med["torch_clip_then_fused"] / med["fused_clip"], 2),
                          "norm_pass_us": round(med["fused_clip"] - med["fused_unclipped"], 1),
                          "torch_clip_then_fused_rounds_us": raw["torch_clip_then_fused"], "fused_clip_rounds_us": raw["fused_clip"],
                          "fused_unclipped_rounds_us": raw["fused_unclipped"]}
            del models, a, b, c, base, clipped, plain, params
        n = sum(p.numel() for p in make().parameters())
        res["parameters"] = n
        res["norm_pass_bytes"] = 4 * n                                               # every gradient read once
        out[name] = res
    return out


def bench_forward(dev, rounds, steps):
    torch.manual_seed(0)
    layer, twin = LinearBin(4096, 4096).to(dev).train(), LinearBin(4096, 4096).to(dev).train()
    opt = utils.FusedQuantSGD(layer, lr=1e-2)
    set_grads(layer, 2)
    opt.step()
    with torch.no_grad():
        twin.weight.copy_(layer.weight)
        twin.bias.copy_(layer.bias)
    x = (torch.randint(0, 2, (4096, 4096), device=dev) * 2 - 1).float()
    assert layer.weight._qt_train_planes is not None and getattr(twin.weight, "_qt_train_planes", None) is None
    before = _lib.call_counts["qt_pack_pair_nib_f32"]
    ya = layer(x)
    assert _lib.call_counts["qt_pack_pair_nib_f32"] == before, "the plane was not consumed"
    yb = twin(x)
    assert _lib.call_counts["qt_pack_pair_nib_f32"] == before + 1 and torch.equal(ya, yb)
    med, raw = alternate({"with_plane": lambda: layer(x), "without_plane": lambda: twin(x)}, rounds, steps)
    return {"with_plane_us": med["with_plane"], "without_plane_us": med["without_plane"],
            "speedup": round(med["without_plane"] / med["with_plane"], 2), "with_plane_rounds_us": raw["with_plane"],
            "without_plane_rounds_us": raw["without_plane"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--clip", action="store_true", help="measure gradient-norm clipping (see the module docstring)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "fused_clip_bench_line.json" if args.clip else "fused_optim_bench_line.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_fused_optim.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    name, cus = _lib.device_info()
    if args.clip:
        line = {"what": "gradient-norm clipping: clip_grad_norm_(foreach=True) + unclipped fused step vs the clipped fused step "
                        "(max_grad_norm=) vs the unclipped fused step", "device": name, "rounds": args.rounds,
                "steps_per_round": args.steps, "max_norm": 1.0, "step": bench_clip(dev, args.rounds, args.steps)}
    else:
        line = {"what": "optimizer.step() + clamp: torch.optim + clamp_weights_ vs the fused update; LinearBin train forward with / "
                        "without the emitted weight plane", "device": name, "rounds": args.rounds, "steps_per_round": args.steps,
                "step": bench_steps(dev, args.rounds, args.steps),
                "forward_linear_bin_4096_b4096": bench_forward(dev, args.rounds, args.steps)}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
