#!/usr/bin/env python
"""Two chained Bi-Real-Net blocks at batch 256, un-modified modules, with and without the residual add inside the deferred sign chain:
one JSON line and a markdown table.

    block:  s = BatchNorm2d(BinConv2d 3x3 s1 p1 (BinaryConnect(x))) + x          two blocks, then BinaryConnect of the second sum

on a real-valued fp32 input, eval mode, ``torch.no_grad()``, implicit hipGraphs off.  Two sides, the same modules and tensors:
  deferred : ``lazy.residual_deferred(True)`` — per block the conv writes fp32 and ONE launch (qt_bn_add_sign_f32) evaluates BatchNorm,
             adds the shortcut and writes the sum and the next conv's operand;
  eager    : ``lazy.residual_deferred(False)`` — how the blocks run without the switch (the path of the commit before it): the ``+``
             is outside the chain grammar, so the conv materialises fp32, BatchNorm, the add and BinaryConnect are library / package
             passes over fp32 tensors, and the next conv packs its operand again.
Both sides end with the sign of the second sum in the form the next binarised conv takes, and are checked to give the same two sums
before anything is timed.  The first shortcut — the input — is NCHW in one run of a shape and channels-last in another.

Method (tools/bench_grouped_chain.py): every (shape, layout) runs in a child process of its own under a time limit, nothing more is
started after a child that fails or overruns; inside a child every side is warmed up, then the two sides take turns within each of
``--rounds`` rounds; a round times ``steps`` forwards with the host clock around a run that ends in a device synchronise.  Reported
per side: the median round and the range of the rounds.  ``bytes``, from the shapes alone (E = elements of one activation), per block:
  eager    : conv result 4E; BatchNorm 8E; add 12E; BinaryConnect 8E + E/8 (image and plane); the next conv's operand pack 4E + E/2
             from an NCHW image, E/8 + E/2 from the plane of a channels-last one                         = 36.6E (NCHW), 32.8E (channels-last)
  deferred : conv result 4E; the pass reads it and the shortcut and writes the sum and the nibble operand 12E + E/2   = 16.5E
  (a conv-epilogue form, not built, would be 8.5E: shortcut in, sum and operand out.)
``hbm_share`` = (bytes / 8 TB/s) / median time of the two blocks on that side; the convs' own operand and weight traffic is in the time
and not in the bytes.  ``kernel``: the new kernel's HBM bound (12.5E / 8 TB/s) beside its measured time.

    python tools/bench_residual_chain.py [--rounds 9] [--out profiles/residual_chain_bench_line.json] [--docs] [--kernel-times]

``--docs`` rewrites the table between the ``residual-chain-table`` markers of README.md and DESIGN.md.  ``--kernel-times`` adds the
residual kernel's own time per case (``kernel_us``) from one separate ``rocprofv3 --kernel-trace --stats`` pass of each child, with no
counters in that run.
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
#: (channels, map): the four stages of a binarised ResNet-18 body
SHAPES = [(64, 56), (128, 28), (256, 14), (512, 7)]
LAYOUTS = ("nchw", "channels_last")
CASES = [(s, lay) for s in SHAPES for lay in LAYOUTS]
HBM_BYTES_PER_S = 8e12
CHILD_LIMIT_S = 300
STEPS = 20
BLOCKS = 2
MARK = "residual-chain-table"
KERNEL = "rs_"                  # rs_rows_kernel / rs_nchw_kernel (csrc/resid_sign.hip)


def algorithmic_bytes(C, H, layout):
    e = BATCH * C * H * H
    pack = 4 * e + e // 2 if layout == "nchw" else e // 8 + e // 2
    return {"eager": BLOCKS * (4 * e + 8 * e + 12 * e + 8 * e + e // 8 + pack), "deferred": BLOCKS * (4 * e + 12 * e + e // 2),
            "kernel": 12 * e + e // 2}


def kernel_time_us(index, workdir):
    """Average duration of the residual kernel in one ``rocprofv3 --kernel-trace --stats`` pass of the child of case ``index`` (one
    round; no counters in the run)."""
    import csv
    import glob
    out = os.path.join(workdir, f"kt_{index}")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "rs", "--output-format", "csv", "--",
                        sys.executable, os.path.abspath(__file__), "--child", str(index), "--rounds", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT_S)
    if p.returncode != 0:
        raise SystemExit(f"case {CASES[index]}: the profiled process ended with status {p.returncode}; nothing more was started")
    path = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))[0]
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if r["Name"].startswith(KERNEL) or ("::" + KERNEL) in r["Name"] or (" " + KERNEL) in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    return round(sum(float(r["TotalDurationNs"]) for r in rows) / max(calls, 1) / 1e3, 1), calls


def child(index, rounds):
    import torch
    import torch.nn as nn
    from pytorch_quantize_impls_amd import _lib, lazy
    from pytorch_quantize_impls_amd.functions import BinaryConnect
    from pytorch_quantize_impls_amd.layers import BinConv2d

    (C, H), layout = CASES[index]
    dev = torch.device("cuda:0")
    torch.manual_seed(index)
    g = torch.Generator().manual_seed(index)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.sign, self.conv, self.bn = BinaryConnect(), BinConv2d(C, C, 3, padding=1), nn.BatchNorm2d(C)
            self.conv.binary_input = True          # +-1 by construction: no side stops to ask the device
            self.bn.running_mean.copy_(torch.randn(C, generator=g) * 4)
            self.bn.running_var.copy_((torch.rand(C, generator=g) + 0.5) * 9 * C)
            gamma = torch.rand(C, generator=g) + 0.5
            gamma[::3] *= -1
            self.bn.weight.data.copy_(gamma)
            self.bn.bias.data.copy_(torch.randn(C, generator=g) * 0.5)

        def forward(self, x):
            return self.bn(self.conv(self.sign(x))) + x

    blocks = nn.Sequential(*[Block() for _ in range(BLOCKS)]).to(dev).eval()
    sign = BinaryConnect()
    x = torch.randn(BATCH, C, H, H, generator=g).to(dev)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)

    def forward(on):
        with torch.no_grad(), lazy.residual_deferred(on):
            s1 = blocks[0](x)
            s2 = blocks[1](s1)
            t = sign(s2)
            if isinstance(t, lazy.LazyActivation):
                act = t._qt.force((1, 1))          # the operand the next 3 x 3 conv would ask for
                assert act is not None
            return s1, s2

    def values(pair):
        return [lazy.resolve(t) for t in pair]

    sides = {"deferred": lambda: forward(True), "eager": lambda: forward(False)}
    calls = dict(_lib.call_counts)
    a = values(sides["deferred"]())
    used_on = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    calls = dict(_lib.call_counts)
    b = values(sides["eager"]())
    used_off = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "the two sides disagree"
    assert used_on.get("qt_bn_add_sign_f32") == BLOCKS and "qt_bn_add_sign_f32" not in used_off, (used_on, used_off)
    del a, b

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
    nbytes = algorithmic_bytes(C, H, layout)
    result = {"channels": C, "map": H, "layout": layout, "bytes": nbytes, "launches": {"deferred": used_on, "eager": used_off},
              "kernel_bound_us": round(nbytes["kernel"] / HBM_BYTES_PER_S * 1e6, 1)}
    for s, v in samples.items():
        med = sorted(v)[len(v) // 2]
        result[s] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                     "hbm_share": round(nbytes[s] / HBM_BYTES_PER_S / (med * 1e-6), 3)}
    result["deferred_range_below_eager"] = result["deferred"]["max_us"] < result["eager"]["min_us"]
    print(json.dumps(result))


def table(shapes):
    own = all("kernel_us" in s for s in shapes)
    rows = ["| channels x map, first shortcut | eager: median (range) us | deferred: median (range) us | eager MB, share of 8 TB/s | "
            "deferred MB, share of 8 TB/s | deferred range below eager |" + (" residual kernel alone: us, HBM bound us, share |" if own else ""),
            "|---|---|---|---|---|---|" + ("---|" if own else "")]
    for s in shapes:
        e, d = s["eager"], s["deferred"]
        ok = "yes" if s["deferred_range_below_eager"] else "**no**"
        name = f"{s['channels']} x {s['map']}², {s['layout']}"
        own_col = ""
        if own:
            own_col = f" {s['kernel_us']}, {s['kernel_bound_us']}, {s['kernel_bound_us'] / max(s['kernel_us'], 1e-9):.2f} |"
        rows.append(f"| {name if s['deferred_range_below_eager'] else '**' + name + '**'} | {e['median_us']} ({e['min_us']}–{e['max_us']}) | "
                    f"{d['median_us']} ({d['min_us']}–{d['max_us']}) | {s['bytes']['eager'] / 1e6:.1f}, {e['hbm_share']} | "
                    f"{s['bytes']['deferred'] / 1e6:.1f}, {d['hbm_share']} | {ok} |" + own_col)
    return "\n".join(rows)


def write_docs(text):
    pat = re.compile(rf"(<!-- {MARK}:begin -->\n).*?(<!-- {MARK}:end -->)", re.S)
    for name in ("README.md", "DESIGN.md"):
        path = os.path.join(ROOT, name)
        with open(path) as fh:
            doc = fh.read()
        if not pat.search(doc):
            raise SystemExit(f"{name}: no {MARK} markers")
        with open(path, "w") as fh:
            fh.write(pat.sub(lambda m: m.group(1) + text + "\n" + m.group(2), doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_chain_bench_line.json"))
    ap.add_argument("--kernel-times", action="store_true", help="one more rocprofv3 --kernel-trace --stats pass per case")
    ap.add_argument("--docs", action="store_true", help="rewrite the table in README.md and DESIGN.md")
    ap.add_argument("--from-json", default=None, help="take the cases from a recorded line instead of measuring (with --docs)")
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.rounds)
    if a.from_json:
        with open(a.from_json) as fh:
            line = json.loads(fh.read().strip().splitlines()[-1])
        print(table(line["shapes"]))
        if a.docs:
            write_docs(table(line["shapes"]))
        return
    shapes = []
    for i in range(len(CASES)):
        # a child per case, each under its own limit; the first failure ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), "--rounds", str(a.rounds)],
                           stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            raise SystemExit(f"case {CASES[i]}: the measuring process ended with status {p.returncode}; nothing more was started")
        shapes.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(shapes[-1]), file=sys.stderr)
    if a.kernel_times:
        import tempfile
        with tempfile.TemporaryDirectory() as work:
            for i, s in enumerate(shapes):
                s["kernel_us"], s["kernel_calls"] = kernel_time_us(i, work)
    from pytorch_quantize_impls_amd import lazy
    line = {"bench": "residual_chain_bireal", "batch": BATCH, "blocks": BLOCKS, "rounds": a.rounds, "steps": STEPS,
            "dtype": "float32 real-valued input", "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": shapes,
            "deferred_below_eager_at_every_shape": all(s["deferred_range_below_eager"] for s in shapes),
            "defer_residual_sign_shipped": bool(lazy.DEFER_RESIDUAL_SIGN)}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    print(table(shapes))
    if a.docs:
        write_docs(table(shapes))


if __name__ == "__main__":
    main()
