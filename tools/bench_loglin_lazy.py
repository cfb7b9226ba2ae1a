#!/usr/bin/env python
"""Eval forward of the Lin / Log VGG16-style CIFAR-10 net with and without the deferred level chain (lazy.DEFER_LEVELS).

The net of tools/bench_loglin_train.py (six 3 x 3 QuantConv2d with BatchNorm, ReLU, MaxPool and the nnQuant(fsr=1, bit_width=8,
with_sign=False) activation quantiser, three LinearQuant), batch 256, lin (bit_width 8) and log (bit_width 3), under no_grad:

  * switch off — the module-by-module forward, call for call what the tree did before the switch existed;
  * switch on  — ``lazy.levels_deferred()``: BatchNorm, ReLU and the quantiser run in the convs' epilogues;
  * the reference's op sequence (F.conv2d / F.linear on the quantised weight: bench_loglin_train.ReferenceOps).

Off and on are timed ALTERNATELY in one session, ``--runs`` times each (default five); a run is the median of ``--iters`` (default
100) device-synchronised calls after a warm-up.  Each mode has a model instance of its own (same seed, same weights): the implicit
hipGraph of a root module is keyed by the input's signature, not by the switch, so one instance would replay one mode's capture for
both.  Every figure is taken twice: with the package's defaults (``eval_us``: implicit hipGraphs as they come — a forward that
synchronises, as the switched-off one does per un-tagged activation in "verify" mode, is never captured) and with implicit graphs
off (``eval_eager_us``: the host-issued launches).  Noise = spread (max - min) of the switched-off runs' medians.

    python tools/bench_loglin_lazy.py --out profiles/loglin_lazy_bench_line.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_loglin_lazy.py --profile-forwards 25 --switch off   (and: on)
    python tools/bench_loglin_lazy.py --kernel-classes off=OFF_kernel_stats.csv on=ON_kernel_stats.csv --forwards 50 \\
        --md profiles/loglin_lazy_rocprof.md
"""
import argparse
import csv
import importlib.util
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))

CLASSES = [   # first match wins; names are this library's kernels (csrc/*.hip) and the runtime's
    ("level pool / BatchNorm1d pass", ("pool_levels", "bn_relu_quant_rows")),
    ("packs and splits", ("level_pack", "act_plane", "triple", "split", "sext", "pack", "absmax", "check_exact")),
    ("quantisers", ("unary_kernel", "OpLinQuant", "OpLogQuant", "quant")),
    ("GEMM / conv (mfma_gemm_kernel)", ("mfma", "gemm", "conv", "implicit", "Cijk", "igemm")),
]


def kernel_classes(path, forwards):
    out = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        cls = next((c for c, keys in CLASSES if any(k in name for k in keys)), "other")
        d = out.setdefault(cls, {"us": 0.0, "calls": 0})
        d["us"] += float(r["TotalDurationNs"]) / 1e3
        d["calls"] += int(r["Calls"])
    return {c: {"us_per_forward": round(d["us"] / forwards, 1), "launches_per_forward": round(d["calls"] / forwards, 1)}
            for c, d in out.items()}


def write_md(path, tables, forwards):
    names = [c for c, _ in CLASSES] + ["other"]
    labels = list(tables)
    lines = ["# Lin / Log VGG eval forward: kernel time by class, switch off and on",
             "",
             f"`rocprofv3 --kernel-trace --stats`, one pass per mode, no counters in the same run; {forwards} eval forwards in all per pass "
             "(lin and log nets, batch 256, after a warm-up of five each, implicit hipGraphs off); microseconds of kernel time and "
             "launches per forward, both nets averaged.  Folded by `tools/bench_loglin_lazy.py --kernel-classes`.",
             "",
             "| kernel class | " + " | ".join(f"{lab}: us | {lab}: launches" for lab in labels) + " |",
             "|---|" + "---|---|" * len(labels)]
    total = {lab: [0.0, 0.0] for lab in labels}
    for c in names:
        cells = []
        for lab in labels:
            d = tables[lab].get(c, {"us_per_forward": 0.0, "launches_per_forward": 0.0})
            total[lab][0] += d["us_per_forward"]
            total[lab][1] += d["launches_per_forward"]
            cells.append(f"{d['us_per_forward']} | {d['launches_per_forward']}")
        lines.append(f"| {c} | " + " | ".join(cells) + " |")
    lines.append("| sum | " + " | ".join(f"{round(total[lab][0], 1)} | {round(total[lab][1], 1)}" for lab in labels) + " |")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _load():
    sys.path.insert(0, ROOT)
    spec = importlib.util.spec_from_file_location("bench_loglin_train", os.path.join(HERE, "bench_loglin_train.py"))
    blt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(blt)
    return blt


def _net(blt, dtype, bits, dev):
    import torch
    torch.manual_seed(0)
    net = blt.VGGLinLog(dtype, bits).to(dev)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                 # statistics and affine parameters away from their initial values
        for bn in list(net.bns) + list(net.bn1d):
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.5)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 4 + 0.5)
            bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.2)
    return net.eval()


def measure(args):
    blt = _load()
    import torch
    from pytorch_quantize_impls_amd import lazy, utils
    from pytorch_quantize_impls_amd.functions import _fused
    dev = torch.device("cuda")
    res = {"what": "Lin/Log VGG16-style CIFAR-10 eval forward, MI355X: lazy.DEFER_LEVELS off / on, alternating runs",
           "batch": args.batch, "iters": args.iters, "runs": args.runs, "detect": _fused.DETECT_MODE}
    for dtype, bits in (("lin", 8), ("log", 3)):
        nets = {"off": _net(blt, dtype, bits, dev), "on": _net(blt, dtype, bits, dev), "ref": _net(blt, dtype, bits, dev)}
        x = torch.randn(args.batch, 3, 32, 32, device=dev)

        def fwd(mode):
            with torch.no_grad(), lazy.levels_deferred(mode == "on"):
                return nets[mode](x)

        with utils.implicit_graphs(False):
            same = bool(torch.equal(fwd("off"), fwd("on")))
        rec = {"bit_width": bits, "on_equals_off": same}
        runs = {"off": [], "on": [], "off_eager": [], "on_eager": []}
        for _ in range(args.runs):
            for mode in ("off", "on"):
                runs[mode].append(round(blt.timed(lambda: fwd(mode), args.iters, warmup=10), 1))
                with utils.implicit_graphs(False):
                    runs[mode + "_eager"].append(round(blt.timed(lambda: fwd(mode), args.iters, warmup=10), 1))
        with blt.ReferenceOps():
            rec["reference_ops_eval_us"] = round(blt.timed(lambda: fwd("ref"), args.iters, warmup=10), 1)
        for key, name in (("off", "eval_us"), ("off_eager", "eval_eager_us")):
            on = runs["on" + key[3:]]
            rec[name] = {"off": {"median": statistics.median(runs[key]), "min": min(runs[key]), "max": max(runs[key]), "runs": runs[key]},
                         "on": {"median": statistics.median(on), "min": min(on), "max": max(on), "runs": on}}
            rec[name]["noise_us"] = round(max(runs[key]) - min(runs[key]), 1)
            rec[name]["on_over_off"] = round(rec[name]["on"]["median"] / rec[name]["off"]["median"], 3)
            rec[name]["on_over_reference_ops"] = round(rec[name]["on"]["median"] / rec["reference_ops_eval_us"], 3)
        rec["implicit_graph"] = {m: {k: v for k, v in utils.implicit_graph_stats(nets[m]).items() if k in ("wrapped", "replays", "graphs",
                                                                                                       "not_faster", "why")}
                                 for m in ("off", "on")}
        res[dtype] = rec
        print(f"[{dtype}] eval forward off {rec['eval_us']['off']['median']} us, on {rec['eval_us']['on']['median']} us "
              f"(eager: {rec['eval_eager_us']['off']['median']} / {rec['eval_eager_us']['on']['median']}), reference ops "
              f"{rec['reference_ops_eval_us']} us", file=sys.stderr)
        del nets
        torch.cuda.empty_cache()
    return res


def profile(args):
    blt = _load()
    import torch
    from pytorch_quantize_impls_amd import lazy, utils
    dev = torch.device("cuda")
    with utils.implicit_graphs(False):
        for dtype, bits in (("lin", 8), ("log", 3)):
            net = _net(blt, dtype, bits, dev)
            x = torch.randn(args.batch, 3, 32, 32, device=dev)

            def fwd():
                with torch.no_grad(), lazy.levels_deferred(args.switch == "on"):
                    net(x)
            blt.timed(fwd, args.profile_forwards, warmup=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--profile-forwards", type=int, default=0, help="run this many eval forwards per net and exit (a rocprofv3 pass)")
    ap.add_argument("--switch", default="off", choices=("off", "on"), help="the mode a --profile-forwards pass runs in")
    ap.add_argument("--kernel-classes", nargs="+", default=None, metavar="LABEL=kernel_stats.csv")
    ap.add_argument("--forwards", type=int, default=60, help="forwards per profiled pass, warm-up included (for --kernel-classes)")
    ap.add_argument("--md", default=None, help="write the --kernel-classes table here")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.profile_forwards:
        return profile(args)
    if args.kernel_classes:
        res = {"kernel_classes": {item.split("=", 1)[0]: kernel_classes(item.split("=", 1)[1], args.forwards) for item in args.kernel_classes}}
        if args.md:
            write_md(args.md, res["kernel_classes"], args.forwards)
    else:
        res = measure(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
