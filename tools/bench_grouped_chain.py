#!/usr/bin/env python
"""The grouped layer of a binarised ResNeXt / ShuffleNet body between its two pointwise convs at batch 256, un-modified modules, with
and without the grouped layer inside the fused inference chain: one JSON line and a markdown table.

    pw 1x1 -> run -> grouped k x k -> run -> pw 1x1 -> run          run = BatchNorm -> Hardtanh -> BinaryConnect

on a +-1 fp32 NCHW input, eval mode, ``torch.no_grad()``, implicit hipGraphs off.  Two sides, the same modules and tensors:
  deferred : ``lazy.grouped_deferred(True)`` — the grouped layer takes the bit planes of the first pointwise chain and its conv,
             BatchNorm / Hardtanh / sign and the operand pack of the second pointwise conv are ONE launch (qt_gconv2d_sign);
  eager    : ``lazy.grouped_deferred(False)`` — how the triple runs without the switch (the path of the commit before it): the first
             pointwise chain materialises fp32 (conv, BatchNorm, Hardtanh, sign as library passes), qt_gconv2d_f32 reads it and writes
             fp32, three more library passes, and the second pointwise conv packs the +-1 image again.
Both sides end by asking the triple's result for the bit planes the next binarised layer would take (the last pointwise chain runs
fused on either side), and both are checked to give the same planes before anything is timed.

Method (tools/bench_depthwise_chain.py): every shape runs in a child process of its own under a time limit, nothing more is started
after a child that fails or overruns; inside a child every side is warmed up, then the two sides take turns within each of
``--rounds`` rounds; a round times ``steps`` forwards with the host clock around a run that ends in a device synchronise.  Reported
per side: the median round and the range of the rounds.  ``bytes`` is what the grouped part of the triple — the grouped layer and
what its presence does to the chain on either side of it — has to move, from the shapes alone (|x| input, |y| output elements of the
grouped layer):
  eager    : the producer's chain un-fused: conv result 4|x|, BatchNorm 8|x|, Hardtanh 8|x|, sign 8|x|; the grouped conv 4|x| + 4|y|;
             BatchNorm 8|y|, Hardtanh 8|y|, sign 8|y|, the consumer's pack 4|y|                                  =  32|x| + 32|y|
  deferred : the bit plane written and read, |x| / 8 each, and the consumer's nibble plane |y| / 2               =  |x| / 4 + |y| / 2
``hbm_share`` = (bytes / 8 TB/s) / median time of the WHOLE triple on that side — the pointwise convs are in the time and not in the
bytes, so it is a lower bound of the grouped part's own share.

    python tools/bench_grouped_chain.py [--rounds 9] [--out profiles/grouped_chain_bench_line.json] [--docs] [--kernel-times]

``--docs`` rewrites the table between the ``grouped-chain-table`` markers of README.md and DESIGN.md.  ``--kernel-times`` adds the
grouped plane kernel's own time per shape (``kernel_us``) from one separate ``rocprofv3 --kernel-trace --stats`` pass of each child,
with no counters in that run.

``--family dorefa`` measures the DoReFa counterpart with the same shapes and the same protocol:

    pw 1x1 (bit_width 1) -> run -> grouped k x k (bit_width 1) -> run -> pw 1x1 (bit_width 1) -> run
                                                                              run = BatchNorm -> ReLU -> nnDorefaQuant(4)

on a quantiser-tagged fp32 input (the channels-last result of nnDorefaQuant(4): an fp32 image that carries its int8 codes).
  deferred : ``lazy.grouped_deferred(True)`` — the grouped layer reads the first pointwise chain's code plane and writes the second
             pointwise conv's code plane in ONE launch (qt_gconv2d_codes);
  eager    : ``lazy.grouped_deferred(False)`` — the path without ``lazy.DEFER_GROUPED_CODES`` (that of the commit before it): the
             producer's codes are expanded to fp32, qt_gconv2d_f32 reads that image and writes fp32, BatchNorm, ReLU and the quantiser
             are three passes over fp32 tensors, then the second pointwise conv runs on the quantiser's codes.
Both sides end by asking for the triple's int8 code plane and must agree on it.  ``bytes`` of the grouped part, from the shapes, by
the count of tools/bench_depthwise_chain.py:
  eager    : conv 4|x| + 4|y|, BatchNorm 8|y|, ReLU 8|y|, quantiser 4|y| in + 4|y| image + |y| codes  =  4|x| + 29|y|
  deferred : |x| + |y| (one code in, one code out)
The line goes to profiles/grouped_codes_chain_bench_line.json, the table between the ``grouped-codes-chain-table`` markers;
``--kernel-times`` then times gc_codes_kernel.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
os.environ.setdefault("QT_AUTO_GRAPH", "0")

BATCH = 256
#: (channels, map, stride, groups, kernel): the grouped layers of tools/bench_grouped.py with at most 8 input channels per group
SHAPES = [(128, 56, 1, 32, 3), (256, 28, 1, 32, 3), (256, 56, 2, 32, 3), (128, 28, 1, 16, 1)]
HBM_BYTES_PER_S = 8e12
CHILD_LIMIT_S = 300
STEPS = 20
MARK = "grouped-chain-table"
KERNEL = "gc_planes_kernel"
FAMILIES = {"sign": {"mark": MARK, "out": "grouped_chain_bench_line.json", "kernel": KERNEL},
            "dorefa": {"mark": "grouped-codes-chain-table", "out": "grouped_codes_chain_bench_line.json", "kernel": "gc_codes_kernel"}}


def algorithmic_bytes(C, H, stride, k):
    Ho = (H + 2 * (k // 2) - k) // stride + 1
    x, y = BATCH * C * H * H, BATCH * C * Ho * Ho
    return {"eager": 32 * x + 32 * y, "deferred": x // 4 + y // 2}


def algorithmic_bytes_dorefa(C, H, stride, k):
    Ho = (H + 2 * (k // 2) - k) // stride + 1
    x, y = BATCH * C * H * H, BATCH * C * Ho * Ho
    return {"eager": 4 * x + 29 * y, "deferred": x + y}


def kernel_time_us(index, workdir, family="sign"):
    """Average duration of the family's grouped chain kernel in one ``rocprofv3 --kernel-trace --stats`` pass of the child of shape ``index``
    (one round; no counters in the run)."""
    import csv
    import glob
    out = os.path.join(workdir, f"kt_{family}_{index}")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "gc", "--output-format", "csv", "--",
                        sys.executable, os.path.abspath(__file__), "--child", str(index), "--rounds", "1", "--family", family],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT_S)
    if p.returncode != 0:
        raise SystemExit(f"shape {SHAPES[index]}: the profiled process ended with status {p.returncode}; nothing more was started")
    path = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))[0]
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if FAMILIES[family]["kernel"] in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    return round(sum(float(r["TotalDurationNs"]) for r in rows) / max(calls, 1) / 1e3, 1), calls


def child(index, rounds):
    import torch
    import torch.nn as nn
    from pytorch_quantize_impls_amd import _lib, lazy
    from pytorch_quantize_impls_amd.functions import BinaryConnect
    from pytorch_quantize_impls_amd.layers import BinConv2d

    C, H, stride, G, k = SHAPES[index]
    dev = torch.device("cuda:0")
    torch.manual_seed(index)
    g = torch.Generator().manual_seed(index)

    def run(c):
        bn = nn.BatchNorm2d(c)
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(torch.rand(c, generator=g) * 8 + 2)
        gamma = torch.rand(c, generator=g) + 0.5
        gamma[::3] *= -1
        bn.weight.data.copy_(gamma)
        bn.bias.data.copy_(torch.randn(c, generator=g) * 0.5)
        return [bn, nn.Hardtanh(inplace=True), BinaryConnect()]

    triple = nn.Sequential(BinConv2d(C, C, 1), *run(C), BinConv2d(C, C, k, stride=stride, padding=k // 2, groups=G), *run(C),
                           BinConv2d(C, C, 1), *run(C)).to(dev).eval()
    for i in (0, 4, 8):
        triple[i].binary_input = True          # +-1 by construction: no side stops to ask the device
    x = torch.where(torch.rand(BATCH, C, H, H, generator=g) < 0.5, -1.0, 1.0).to(dev)

    def forward(on):
        with torch.no_grad(), lazy.grouped_deferred(on):
            out = triple(x)
            act = out._qt.force(None)          # the planes the next binarised layer would ask for
            assert act is not None and act.planes is not None
            return act.planes.sign

    sides = {"deferred": lambda: forward(True), "eager": lambda: forward(False)}
    calls = dict(_lib.call_counts)
    a = sides["deferred"]()
    used_on = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    calls = dict(_lib.call_counts)
    b = sides["eager"]()
    used_off = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    assert torch.equal(a, b), "the two sides disagree"
    assert used_on.get("qt_gconv2d_sign") == 1 and "qt_gconv2d_f32" not in used_on, used_on
    assert used_off.get("qt_gconv2d_f32") == 1 and "qt_gconv2d_sign" not in used_off, used_off

    def run_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / STEPS

    for fn in sides.values():
        for _ in range(3):
            fn()
    samples = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            samples[s].append(run_us(fn))
    nbytes = algorithmic_bytes(C, H, stride, k)
    result = {"channels": C, "map": H, "stride": stride, "groups": G, "kernel": k, "bytes": nbytes,
              "launches": {"deferred": used_on, "eager": used_off}}
    for s, v in samples.items():
        med = sorted(v)[len(v) // 2]
        result[s] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                     "hbm_share": round(nbytes[s] / HBM_BYTES_PER_S / (med * 1e-6), 3)}
    result["deferred_range_below_eager"] = result["deferred"]["max_us"] < result["eager"]["min_us"]
    print(json.dumps(result))


def child_dorefa(index, rounds):
    import torch
    import torch.nn as nn
    from pytorch_quantize_impls_amd import _lib, lazy
    from pytorch_quantize_impls_amd.functions import nnDorefaQuant
    from pytorch_quantize_impls_amd.layers import DorefaConv2d

    C, H, stride, G, k = SHAPES[index]
    dev = torch.device("cuda:0")
    torch.manual_seed(index)
    g = torch.Generator().manual_seed(index)

    def run(c, fan):
        # statistics sized for a sum of ``fan`` products of +-E and a 4-bit image: the codes stay far inside int8
        bn = nn.BatchNorm2d(c)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_((torch.rand(c, generator=g) + 0.5) * fan * 0.05)
        gamma = torch.rand(c, generator=g) * 0.5 + 0.25
        gamma[::3] *= -1
        bn.weight.data.copy_(gamma)
        bn.bias.data.copy_(torch.randn(c, generator=g) * 0.2 + 0.3)
        return [bn, nn.ReLU(), nnDorefaQuant(4)]

    triple = nn.Sequential(DorefaConv2d(C, C, 1, bit_width=1), *run(C, C),
                           DorefaConv2d(C, C, k, stride=stride, padding=k // 2, groups=G, bit_width=1), *run(C, C // G * k * k),
                           DorefaConv2d(C, C, 1, bit_width=1), *run(C, C))
    triple = triple.to(dev).to(memory_format=torch.channels_last).eval()
    with torch.no_grad():
        x = nnDorefaQuant(4)(torch.rand(BATCH, C, H, H, generator=g).to(dev).contiguous(memory_format=torch.channels_last))

    def forward(on):
        with torch.no_grad(), lazy.grouped_deferred(on):
            out = triple(x)
            act = out._qt.force((0, 0))        # the code plane the next DoReFa layer would ask for
            assert act is not None
            return act.codes

    sides = {"deferred": lambda: forward(True), "eager": lambda: forward(False)}
    calls = dict(_lib.call_counts)
    a = sides["deferred"]()
    used_on = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    calls = dict(_lib.call_counts)
    b = sides["eager"]()
    used_off = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    assert torch.equal(a.codes, b.codes), "the two sides disagree"
    assert int(a.overflow.item()) == 0 and int(b.overflow.item()) == 0 and int(a.codes.count_nonzero()) > 0
    assert used_on.get("qt_gconv2d_codes") == 1 and "qt_gconv2d_f32" not in used_on, used_on
    assert used_off.get("qt_gconv2d_f32") == 1 and "qt_gconv2d_codes" not in used_off, used_off

    def run_us(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / STEPS

    for fn in sides.values():
        for _ in range(3):
            fn()
    samples = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            samples[s].append(run_us(fn))
    nbytes = algorithmic_bytes_dorefa(C, H, stride, k)
    result = {"channels": C, "map": H, "stride": stride, "groups": G, "kernel": k, "bytes": nbytes,
              "launches": {"deferred": used_on, "eager": used_off}}
    for s, v in samples.items():
        med = sorted(v)[len(v) // 2]
        result[s] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                     "hbm_share": round(nbytes[s] / HBM_BYTES_PER_S / (med * 1e-6), 3)}
    result["deferred_range_below_eager"] = result["deferred"]["max_us"] < result["eager"]["min_us"]
    print(json.dumps(result))


def table(shapes, kernel_name="grouped plane kernel"):
    own = all("kernel_us" in s for s in shapes)
    rows = ["| grouped channels x map, groups, kernel, stride | eager: median (range) us | deferred: median (range) us | "
            "eager MB, share of 8 TB/s | deferred MB, share of 8 TB/s | deferred range below eager |"
            + (f" {kernel_name} alone, us |" if own else ""),
            "|---|---|---|---|---|---|" + ("---|" if own else "")]
    for s in shapes:
        e, d = s["eager"], s["deferred"]
        ok = "yes" if s["deferred_range_below_eager"] else "**no**"
        name = f"{s['channels']} x {s['map']}², g{s['groups']}, {s['kernel']}x{s['kernel']}, s{s['stride']}"
        rows.append(f"| {name if s['deferred_range_below_eager'] else '**' + name + '**'} | {e['median_us']} ({e['min_us']}–{e['max_us']}) | "
                    f"{d['median_us']} ({d['min_us']}–{d['max_us']}) | {s['bytes']['eager'] / 1e6:.1f}, {e['hbm_share']} | "
                    f"{s['bytes']['deferred'] / 1e6:.1f}, {d['hbm_share']} | {ok} |" + (f" {s['kernel_us']} |" if own else ""))
    return "\n".join(rows)


def write_docs(text, mark=MARK):
    pat = re.compile(rf"(<!-- {mark}:begin -->\n).*?(<!-- {mark}:end -->)", re.S)
    for name in ("README.md", "DESIGN.md"):
        path = os.path.join(ROOT, name)
        with open(path) as fh:
            doc = fh.read()
        if not pat.search(doc):
            raise SystemExit(f"{name}: no {mark} markers")
        with open(path, "w") as fh:
            fh.write(pat.sub(lambda m: m.group(1) + text + "\n" + m.group(2), doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--family", choices=sorted(FAMILIES), default="sign", help="sign: BinConv2d triple (default); dorefa: DorefaConv2d triple")
    ap.add_argument("--out", default=None, help="default: profiles/grouped_chain_bench_line.json (sign), "
                                                "profiles/grouped_codes_chain_bench_line.json (dorefa)")
    ap.add_argument("--kernel-times", action="store_true", help="one more rocprofv3 --kernel-trace --stats pass per shape")
    ap.add_argument("--docs", action="store_true", help="rewrite the table in README.md and DESIGN.md")
    ap.add_argument("--from-json", default=None, help="take the shapes from a recorded line instead of measuring (with --docs)")
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    fam = FAMILIES[a.family]
    dorefa = a.family == "dorefa"
    kernel_name = "grouped code kernel" if dorefa else "grouped plane kernel"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", fam["out"])
    if a.child is not None:
        return child_dorefa(a.child, a.rounds) if dorefa else child(a.child, a.rounds)
    if a.from_json:
        with open(a.from_json) as fh:
            line = json.loads(fh.read().strip().splitlines()[-1])
        print(table(line["shapes"], kernel_name))
        if a.docs:
            write_docs(table(line["shapes"], kernel_name), fam["mark"])
        return
    shapes = []
    for i in range(len(SHAPES)):
        # a child per shape, each under its own limit; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), "--rounds", str(a.rounds), "--family", a.family],
                           stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            raise SystemExit(f"shape {SHAPES[i]}: the measuring process ended with status {p.returncode}; nothing more was started")
        shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr)
    if a.kernel_times:
        import tempfile
        with tempfile.TemporaryDirectory() as work:
            for i, s in enumerate(shapes):
                s["kernel_us"], s["kernel_calls"] = kernel_time_us(i, work, a.family)
    from pytorch_quantize_impls_amd import lazy
    line = {"bench": "grouped_chain_resnext", "batch": BATCH, "rounds": a.rounds, "steps": STEPS, "dtype": "float32 +-1 input",
            "layout": "NCHW", "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": shapes,
            "deferred_below_eager_at_every_shape": all(s["deferred_range_below_eager"] for s in shapes),
            "defer_grouped_shipped": bool(lazy.DEFER_GROUPED)}
    if dorefa:
        line.update({"bench": "grouped_codes_chain_resnext", "dtype": "float32 image of 4-bit codes, code-tagged", "layout": "channels_last"})
        del line["defer_grouped_shipped"]
        line["defer_grouped_codes_shipped"] = bool(lazy.DEFER_GROUPED_CODES)
    text = json.dumps(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    print(table(shapes, kernel_name))
    if a.docs:
        write_docs(table(shapes, kernel_name), fam["mark"])


if __name__ == "__main__":
    main()
