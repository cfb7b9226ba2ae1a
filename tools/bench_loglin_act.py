#!/usr/bin/env python
"""Lin / Log training step and eval forward on the GPU, for A/B runs of two source trees: one JSON line per run.

The workloads of tools/bench_loglin_train.py (its VGGLinLog: six 3 x 3 QuantConv2d with BatchNorm, ReLU, MaxPool and the
nnQuant(fsr=1, bit_width=8, with_sign=False) activation quantiser, three LinearQuant; CIFAR-10 shapes, batch 256; lin bit_width 8 and
log bit_width 3):
  * the training step — forward, NLL loss, backward, SGD step, clamp();
  * the eval-mode forward under no_grad.
Every timing is device-synchronised (one event pair per call, synchronised before the next call), after a warm-up of the same
call; the figure is the median of --iters calls (default 100).

``--root DIR`` imports the package (and tools/bench_loglin_train.py) from another checkout of this repository — the tree a change
is compared against is a second checkout, built on its own, never a switch inside the new code:

    python tools/bench_loglin_act.py --label new    --out new_1.json
    python tools/bench_loglin_act.py --label parent --root ../parent --out parent_1.json      (alternate, five times each)
    python tools/bench_loglin_act.py --aggregate parent_*.json new_*.json --out profiles/loglin_act_bench_line.json

``--aggregate`` folds such lines: per label the median of the runs' medians, the spread (max - min) of the ``parent`` runs as
the noise, and new / parent.  ``--reference`` also times the reference's op sequence (F.conv2d / F.linear on the quantised
weight, bench_loglin_train.ReferenceOps).  ``--detect remember``: un-tagged activations are trusted after the first verdict (no
host sync per pooled / flattened activation; a broken assumption poisons the output).  ``--profile-steps N``: run N steps and N
eval forwards after a warm-up of five and exit (the program of a ``rocprofv3 --kernel-trace --stats`` pass);
``--kernel-classes FILE``: fold such a pass's kernel_stats.csv into the classes GEMM / conv, weight gradient, packs and splits,
quantisers, other.
"""
import argparse
import csv
import importlib.util
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

CLASSES = [   # first match wins; names are this library's kernels (csrc/*.hip) and the runtime's
    ("weight gradient", ("wgrad", "pm_reduce", "pm_pack", "gemm_taps")),
    ("packs and splits", ("level_pack", "act_plane", "triple", "split", "sext", "pack", "absmax", "check_exact")),
    ("quantisers", ("unary_kernel", "OpLinQuant", "OpLogQuant", "quant")),
    ("GEMM / conv", ("mfma", "gemm", "conv", "implicit", "Cijk", "igemm")),
]


def kernel_classes(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    out = {}
    for r in rows:
        name = r["Name"]
        cls = next((c for c, keys in CLASSES if any(k in name for k in keys)), "other")
        d = out.setdefault(cls, {"us": 0.0, "calls": 0})
        d["us"] += float(r["TotalDurationNs"]) / 1e3
        d["calls"] += int(r["Calls"])
    return {c: {"us": round(d["us"], 1), "calls": d["calls"], "share": round(d["us"] * 1e3 / total, 3)} for c, d in out.items()}


def aggregate(paths):
    runs = {}
    for p in paths:
        for line in open(p):
            line = line.strip()
            if line.startswith("{"):
                rec = json.loads(line)
                runs.setdefault(rec["label"], []).append(rec)
    res = {"what": "Lin/Log VGG16-style CIFAR-10 training step and eval forward, MI355X: medians of alternating runs", "labels": {}}
    for label, recs in runs.items():
        res["batch"], res["iters"] = recs[0]["batch"], recs[0]["iters"]
        lab = res["labels"][label] = {"runs": len(recs)}
        for dtype in ("lin", "log"):
            for key in ("step_us", "eval_us", "reference_ops_step_us", "reference_ops_eval_us"):
                vals = [r[dtype][key] for r in recs if key in r.get(dtype, {})]
                if vals:
                    lab.setdefault(dtype, {})[key] = {"median": round(statistics.median(vals), 1), "min": min(vals), "max": max(vals),
                                                      "runs": vals}
    if "parent" in res["labels"] and "new" in res["labels"]:
        res["new_over_parent"], res["noise_us"] = {}, {}
        for dtype in ("lin", "log"):
            for key in ("step_us", "eval_us"):
                p, q = res["labels"]["parent"][dtype][key], res["labels"]["new"][dtype][key]
                res["noise_us"][f"{dtype}_{key}"] = round(p["max"] - p["min"], 1)
                res["new_over_parent"][f"{dtype}_{key}"] = round(q["median"] / p["median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--label", default="new")
    ap.add_argument("--root", default=os.path.normpath(os.path.join(HERE, "..")), help="checkout whose package is measured")
    ap.add_argument("--reference", action="store_true", help="also time the reference's op sequence")
    ap.add_argument("--detect", default=None, choices=("verify", "remember"),
                    help="detection mode for un-tagged (pooled, flattened) activations; default: the package's (verify: one sync each)")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--aggregate", nargs="+", default=None)
    ap.add_argument("--kernel-classes", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.aggregate or args.kernel_classes:
        res = aggregate(args.aggregate) if args.aggregate else {}
        if args.kernel_classes:
            res["kernel_classes"] = kernel_classes(args.kernel_classes)
    else:
        res = measure(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def measure(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import torch.nn.functional as F
    spec = importlib.util.spec_from_file_location("bench_loglin_train", os.path.join(root, "tools", "bench_loglin_train.py"))
    blt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(blt)
    import pytorch_quantize_impls_amd
    assert os.path.abspath(pytorch_quantize_impls_amd.__file__).startswith(root + os.sep), pytorch_quantize_impls_amd.__file__

    from pytorch_quantize_impls_amd.functions import _fused
    if args.detect:
        _fused.DETECT_MODE = args.detect           # the process default: the backward threads read it too
    dev = torch.device("cuda")
    res = {"label": args.label, "batch": args.batch, "iters": args.iters, "detect": _fused.DETECT_MODE}
    for dtype, bits in (("lin", 8), ("log", 3)):
        torch.manual_seed(0)
        net = blt.VGGLinLog(dtype, bits).to(dev)
        opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
        x = torch.randn(args.batch, 3, 32, 32, device=dev)
        t = torch.randint(0, 10, (args.batch,), device=dev)

        def step():
            opt.zero_grad(set_to_none=False)
            F.nll_loss(net(x), t).backward()
            opt.step()
            net.clamp()

        def fwd():
            with torch.no_grad():
                net(x)

        if args.profile_steps:
            net.train()
            blt.timed(step, args.profile_steps, warmup=5)
            net.eval()
            blt.timed(fwd, args.profile_steps, warmup=5)
            continue
        net.train()
        rec = {"bit_width": bits, "step_us": round(blt.timed(step, args.iters, warmup=10), 1)}
        if args.reference:
            with blt.ReferenceOps():
                rec["reference_ops_step_us"] = round(blt.timed(step, args.iters, warmup=10), 1)
        net.eval()
        rec["eval_us"] = round(blt.timed(fwd, args.iters, warmup=10), 1)
        if args.reference:
            with blt.ReferenceOps():
                rec["reference_ops_eval_us"] = round(blt.timed(fwd, args.iters, warmup=10), 1)
        res[dtype] = rec
        print(f"[{args.label} {dtype}] step {rec['step_us']} us, eval forward {rec['eval_us']} us (medians of {args.iters})", file=sys.stderr)
        del net, opt
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
