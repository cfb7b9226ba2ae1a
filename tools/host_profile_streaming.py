#!/usr/bin/env python
"""Host time of the depthwise / grouped streaming-conv wrappers of ``ops``: what one call costs the Python thread before the launch
is in the queue.  These layers are small and launch-bound, so the wrapper's own time is part of the layer's (see the comment above
``ops._p``).  Per wrapper: warm up, 2000 un-synchronised calls timed with time.perf_counter, one synchronise.

    python tools/host_profile_streaming.py [--tree TREE]        # one JSON line {wrapper: microseconds per call}
    python tools/host_profile_streaming.py --against OTHER_TREE [--rounds 5] [--out FILE.json]

``--tree``: the checkout whose package is measured (default: the one this file lies in).  The second form compares two checkouts,
each with its library built — OTHER_TREE need not contain this file, every process runs this one —: fresh processes, alternating
OTHER_TREE and this tree, and per wrapper the rounds, the median and the min - max spread of either; a wrapper of this tree
whose median lies outside the other's spread is marked."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, WARMUP = 2000, 200
# the shapes of tests/_streaming_cases.py at 16 channels and 14 x 14
N, C, H, W, KH, KW = 2, 16, 14, 14, 3, 2
GEO = dict(stride=(2, 1), padding=(1, 0), dilation=(1, 2))


def measure(tree: str):
    import torch
    sys.path.insert(0, tree)
    from pytorch_quantize_impls_amd import ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree) + os.sep), f"measuring {ops.__file__}, not {tree}"

    dev = torch.device("cuda:0")
    Ho, Wo = ops.conv_out_hw(H, W, KH, KW, **GEO)

    def f32(*shape):
        return torch.randn(*shape, device=dev)

    def planes():
        return ops.BitPlanes(sign=torch.zeros((N * H * W, ops.packed_ld(C)), dtype=torch.int32, device=dev), rows=N * H * W, K=C)

    def codes():
        return ops.CodePlanes(codes=torch.zeros((N * H * W, ops.code_ld_bytes(C, 16)), dtype=torch.int8, device=dev), rows=N * H * W,
                              K=C, inv_n=ops.inv_levels(4), bit_width=4, overflow=torch.zeros(1, dtype=torch.int32, device=dev))

    x, shape, pl, cd = f32(N, C, H, W), (N, C, H, W), planes(), codes()
    jobs = {}
    for name, w, kw in (("depthwise", f32(2 * C, 1, KH, KW), {}), ("grouped", f32(12, 4, KH, KW), {"groups": 4})):
        kw = {**GEO, **kw}
        cout = int(w.shape[0])
        go, ab = f32(N, cout, Ho, Wo), (f32(cout), f32(cout))
        epi = ops.CodeEpilogue(*ab, 4, True, overflow=cd.overflow)
        op = {what: getattr(ops, f"{name}_{what}") for what in ("conv2d", "conv2d_grad_input", "conv2d_grad_weight", "conv2d_sign",
                                                                 "conv2d_codes")}
        jobs[f"{name}_conv2d"] = lambda f=op["conv2d"], w=w, kw=kw: f(x, w, None, **kw)
        jobs[f"{name}_conv2d_grad_input"] = lambda f=op["conv2d_grad_input"], w=w, kw=kw, go=go: f(shape, w, go, **kw)
        jobs[f"{name}_conv2d_grad_weight"] = lambda f=op["conv2d_grad_weight"], w=w, kw=kw, go=go: f(x, go, w, **kw)
        jobs[f"{name}_conv2d_sign"] = lambda f=op["conv2d_sign"], w=w, kw=kw, ab=ab: f(pl, w, None, *ab, **kw, shape=shape)
        jobs[f"{name}_conv2d_codes"] = lambda f=op["conv2d_codes"], w=w, kw=kw, epi=epi: f(cd, shape, w, None, epi, **kw)
    out = {}
    for name, job in jobs.items():
        for _ in range(WARMUP):
            job()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            job()
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        out[name] = round(t / CALLS * 1e6, 3)
    print(json.dumps(out))


def compare(other: str, rounds: int, out_path):
    trees = {"other": os.path.abspath(other), "this": HERE}
    runs = {k: [] for k in trees}
    for _ in range(rounds):
        for k, tree in trees.items():
            # a fresh process per round; a failure ends the comparison (nothing more is started on the device)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree], capture_output=True, text=True, timeout=300,
                               check=True)
            runs[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rows = {}
    for name in runs["this"][0]:
        row = {}
        for k in trees:
            v = [r[name] for r in runs[k]]
            row[k] = {"rounds_us": v, "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
        row["this_median_inside_other_spread"] = row["other"]["min_us"] <= row["this"]["median_us"] <= row["other"]["max_us"]
        row["this_median_below_other_min"] = row["this"]["median_us"] < row["other"]["min_us"]
        rows[name] = row
    result = {"calls": CALLS, "rounds": rounds, "shape": {"N": N, "C": C, "H": H, "W": W, "kernel": [KH, KW], **{k: list(v) for k, v in GEO.items()}},
              "wrappers": rows}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--against", help="another checkout of this repository, built, to compare with")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="write the comparison here as JSON")
    a = ap.parse_args()
    compare(a.against, a.rounds, a.out) if a.against else measure(a.tree)
