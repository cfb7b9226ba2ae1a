#!/usr/bin/env python
"""bench.py — headline benchmark of the hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

Workload (config.workload = "c2"): BASELINE.json configs[1] — LinearBin 4096x4096 XNOR-popcount
GEMM, batch 4096 PER GPU (weak scaling: the op is batch-sharded, no collective on the data path).
One "step" = one training-mode LinearBin forward on +-1 activations with fp32 inputs already
resident in HBM, called THROUGH THE MODULE (LinearBin(4096, 4096, bias=False).train()(x), autograd on, binary_input=True):
dispatch -> sign+nibble-pack(x) + sign+nibble-pack(W) (one launch) -> packed GEMM -> y (fp32) + the autograd node, all through
the C-ABI of libqt_hip.so.  value = whole-job tera-ops/s, ops = 2*B*K*N per GPU per step.  "c2_ops_level" = the same two
launches called at the ops level (the headline of rounds 1-5), timed in the same bracket.

For N > 1 the driver launches one rank per GPU with torch.distributed.run; ranks only meet in the
barriers that bracket the timed region and in the MAX reduction of the elapsed time.

A plain run sets up, warms up, times the K headline steps, writes the last step's output if --dump-outputs DIR is given
(DIR/y.npy, float32; a fixed, seeded row sample when the output is larger than DUMP_CAP_BYTES) and prints the line: the
contract keys, config, per-rank times, "dist" and roofline.step_hbm (from the headline's own time).  Everything below takes
runs of its own and happens only with --full (which also writes bench_detail.json); the other flags (--no-extras,
--alexnet-batch, --no-cpu-baseline, ...) select among those legs.

Extra objects on the JSON line (--full): "roofline" (dominant kernel, HIP-event timed inside the timed
region) and "cpu_baseline" (reference op sequence on the host cores, rank 0, N=1 only), "alexnet" (second half
of the metric) and "extra": the other BASELINE configs, each timed by the same process and each with the roofline
SURVEY.md 8(d) prescribes (ops = 2 * MACs, bytes = fp32 activations in + fp32 weights + fp32 activations out per
quantised layer): C2 eval mode on pre-packed operands, C2 with a bias (float-tail parity), C4 (DoReFa ResNet-18 W1A4,
batch 256) and C5 (ternary VGG-16, 256 per GPU): the un-modified module graph (deferred activations, lazy.py), the same
graph module by module, and the explicit fused inference form.  "reference_ops_on_gpu" (C2 and AlexNet) is a second
BASELINE leg beside cpu_baseline: the reference's op sequence (oracle/torch_port.py: torch.sign + F.linear / F.conv2d in
fp32 + the torch modules) executed by ROCm PyTorch on this same GPU — what the un-modified reference gets here; like the
CPU leg it is only reported, never part of `value`, and it is the only other place bench.py touches oracle/.

--strong: strong scaling — the GLOBAL batch is fixed (C2: --batch rows, AlexNet / C4 / C5: their batch) and split
over the ranks ("scaling": "strong"); default is weak scaling (batch per GPU fixed).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
VALU_PEAK_TOPS = 2516.6        # 256 CU x 4 SIMD x 32 lanes x 2.4 GHz x 32 MAC / 2 lane-ops x 2 ops
MFMA_FP4_PEAK_TFLOPS = 10000.0  # dense MXFP4 (MI355X_MICROARCH.md)
EVENT_EVERY = 10                # GEMM launches bracketed by HIP events: every 10th timed step (a pair costs ~7.6 us of stream time)
DUMP_CAP_BYTES = 32 << 20       # --dump-outputs: all ranks together write at most this much (a fixed row sample of larger outputs)
DUMP_SEED = 0


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096, help="rows per GPU")
    ap.add_argument("--in-features", type=int, default=4096)
    ap.add_argument("--out-features", type=int, default=4096)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget-s", type=float, default=12.0)
    ap.add_argument("--gemm", default="auto", choices=["auto", "valu", "mfma"],
                    help="packed GEMM formulation (auto = fastest available for the shape)")
    ap.add_argument("--alexnet-batch", type=int, default=256, help="images per GPU (0 = skip)")
    ap.add_argument("--alexnet-iters", type=int, default=10)
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) | gloo (smoke tests)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group (and run the data-parallel training extra) even with ONE rank: exercises "
                         "the RCCL init / barrier / all-reduce path on a 1-GPU box")
    ap.add_argument("--share-device", action="store_true",
                    help="smoke test only: every rank uses cuda:0 (exercise the N>1 code path on a 1-GPU box)")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling: --batch / --alexnet-batch / --c4-batch / --c5-batch are GLOBAL and split over the ranks")
    ap.add_argument("--no-extras", action="store_true", help="skip the 'extra' object (C2 eval / bias, C4, C5)")
    ap.add_argument("--c4-batch", type=int, default=256, help="C4 images per GPU (global with --strong; 0 = skip)")
    ap.add_argument("--c5-batch", type=int, default=256, help="C5 images per GPU (global with --strong, e.g. 2048; 0 = skip)")
    ap.add_argument("--extra-iters", type=int, default=10)
    ap.add_argument("--train-batch", type=int, default=256, help="AlexNet-Bin training-step extra at N = 1 (0 = skip)")
    ap.add_argument("--launch-check", action="store_true",
                    help="only bring the ranks up (self-launch when no launcher is around), meet in the barrier / MAX reduction the "
                         "timed region uses and print the 'dist' object: runs without a GPU (tests/test_dist_gloo.py)")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement of the line: ops-level leg, kernel roofline, C2 layer legs, reference ops "
                         "on the GPU, AlexNet, the extra configs, CPU baseline, bench_detail.json (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32; a fixed, "
                         f"seeded sample of rows when the output of all ranks is larger than {DUMP_CAP_BYTES >> 20} MiB)")
    return ap.parse_args()


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            # no launcher around this process: re-execute under torch.distributed.run (one rank per GPU, rendezvous on 127.0.0.1)
            # — `python bench.py --gpus 8` alone is a complete command; rank 0 of the child job prints the single JSON line
            return self_launch(args.gpus)
        sys.exit(f"--gpus {args.gpus} but the launcher started {world} ranks (WORLD_SIZE): pass --gpus {world}")
    if args.launch_check:
        return launch_check(args, world, rank)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a HIP device (there is no CPU fallback for the product path)")
    if args.share_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                                   # --force-dist without a launcher
            os.environ.setdefault("MASTER_PORT", "29517")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if args.dist_backend == "nccl":
            dist_mod.init_process_group("nccl", device_id=dev)
        else:
            dist_mod.init_process_group(args.dist_backend)
        dist = dist_mod

    from pytorch_quantize_impls_amd import _lib, ops
    from pytorch_quantize_impls_amd.functions import _fused

    if args.strong:
        for name in ("batch", "alexnet_batch", "c4_batch", "c5_batch"):
            g = getattr(args, name)
            if g % world:
                sys.exit(f"--strong: --{name.replace('_', '-')} {g} is not divisible by {world} ranks")
            setattr(args, name, g // world)
    B, K, N = args.batch, args.in_features, args.out_features
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x5EED + rank)
    # synthetic data of the config's shape: +-1 activations (fp32), W ~ N(0, 1/K), bias = 0
    x = torch.randn((B, K), device=dev, generator=gen).sign_()
    x[x == 0] = 1
    w = torch.randn((N, K), device=dev, generator=gen) * (1.0 / K) ** 0.5
    y = torch.empty((B, N), device=dev, dtype=torch.float32)

    gemm_impl = ops.select_gemm_impl(args.gemm, B, N, K)

    ev_pairs = []

    # The headline step goes THROUGH THE MODULE: LinearBin(K, N, bias=False) in training mode, autograd on (the
    # weight requires grad: the layer's autograd node saves its inputs), the layer's dispatch and output view inside the timed
    # region.  binary_input=True is the layer's documented "the caller guarantees +-1 activations" (what a BinaryConnect in front of
    # the layer establishes in the reference's models, layers/binary_layers.py:42-46); the default None asks the device per call
    # and is reported in c2_layer_forward.detect_on_device.  The two ops the layer ends in are timed beside it (c2_ops_level).
    from pytorch_quantize_impls_amd.layers import LinearBin
    layer = LinearBin(K, N, bias=False).to(dev)
    layer.weight.data.copy_(w)
    layer.train()
    layer.binary_input = True
    assert layer.weight.requires_grad and torch.is_grad_enabled()

    def step():
        return layer(x)

    def ops_step(record=False):
        xp, wp = ops.pack_linear_operands(x, w, "binary", gemm_impl)   # both operands, one launch on the mfma route
        if record:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.packed_gemm(xp, wp, None, out=y, impl=gemm_impl)
            e1.record()
            ev_pairs.append((e0, e1))
        else:
            ops.packed_gemm(xp, wp, None, out=y, impl=gemm_impl)

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    calls_before = dict(_lib.call_counts)
    for _ in range(args.warmup):
        y_layer = step()
    sync_all()
    t0 = time.perf_counter()
    for i in range(args.steps):
        y_layer = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0        # this rank's K steps are complete; the MAX over the ranks is taken below
    sync_all()                                # closing barrier + synchronize of the bracket (its own latency — ~0.3 ms for an RCCL
    #                                           barrier, measured with --force-dist — is not K steps of work and is not billed)
    headline_calls = {k: v - calls_before.get(k, 0) for k, v in _lib.call_counts.items() if v != calls_before.get(k, 0)}
    assert y_layer.grad_fn is not None, "the headline step must be the training-mode forward with its autograd node"
    per_rank_ms = [elapsed / args.steps * 1e3]
    if dist is not None:
        # every rank's own step time travels with the line, so a SCALE run is self-checking (a straggler or a rank that
        # did no work shows up here); `ms_per_step` / `value` use the MAX over the ranks as the contract says
        per_rank_ms = [t_ / args.steps * 1e3 for t_ in gather_per_rank(dist, dev, world, elapsed)]
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"y": y_layer}, rank, world)

    ops_per_step = 2.0 * B * K * N
    value = world * ops_per_step * args.steps / elapsed / 1e12
    roofline, c2_ops_level = {}, None
    if args.full:
        # ---- the same work at the ops level (the two C-ABI wrappers the layer ends in), same bracket; HIP events bracket the GEMM on
        # every EVENT_EVERY-th step only: a recorded pair costs ~7.6 us of stream time per step (tools/bench_step_overheads.py)
        for _ in range(args.warmup):
            ops_step()
        sync_all()
        t0 = time.perf_counter()
        for i in range(args.steps):
            ops_step(record=(i % EVENT_EVERY == 0))
        torch.cuda.synchronize()
        ops_elapsed = time.perf_counter() - t0
        sync_all()
        if dist is not None:
            tt = torch.tensor([ops_elapsed], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ops_elapsed = float(tt.item())
        same_as_ops = bool(torch.equal(y_layer.detach(), y))

        gemm_ms = sum(a.elapsed_time(b) for a, b in ev_pairs) / len(ev_pairs)
        # what an event pair measures around NOTHING on a busy stream (marker packets only): the part of the bracket that is
        # not kernel time; calibrated outside the timed region, behind the same pack kernel as in a step
        empty = []
        for _ in range(20):
            ops.pack_linear_operands(x, w, "binary", gemm_impl)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            empty.append((e0, e1))
        torch.cuda.synchronize()
        empty_ms = sorted(a.elapsed_time(b) for a, b in empty)[len(empty) // 2]

        # the same launch as a burst behind the pack kernel, one event pair around BURST launches, marker cost subtracted:
        # per-launch time with only the ~1 us kernel-to-kernel hand-over on top of the kernel duration rocprofv3 reports
        BURST = 50
        xp_b, wp_b = ops.pack_linear_operands(x, w, "binary", gemm_impl)
        b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.pack_linear_operands(x, w, "binary", gemm_impl)
        b0.record()
        for _ in range(BURST):
            ops.packed_gemm(xp_b, wp_b, None, out=y, impl=gemm_impl)
        b1.record()
        torch.cuda.synchronize()
        burst_ms = max(b0.elapsed_time(b1) - empty_ms, 0.0) / BURST

        # ---- roofline of the dominant kernel (the packed GEMM) ------------------------------------
        gemm_bytes = ops.packed_gemm_algorithmic_bytes(B, N, K, gemm_impl)  # DESIGN.md "Kernels"
        timing = {"kernel_ms": burst_ms,
                  "kernel_ms_what": f"{BURST} launches back to back behind the pack kernel, one HIP-event pair around the burst, the "
                                    "cost of an empty event pair subtracted; `achieved` and `frac` use THIS figure; the rocprofv3 "
                                    "--kernel-trace --stats average of the same command is quoted beside it (rocprof_avg_us, from "
                                    "profiles/pmc_latest.json, refreshed by tools/collect_profiles.sh)",
                  "kernel_ms_in_step_bracket": gemm_ms,
                  "kernel_ms_in_step_bracket_what": f"HIP-event pair around the single launch on every {EVENT_EVERY}th step of the timed "
                                                    "region; includes the marker packets / kernel boundary (~3-5 us)",
                  "event_pair_empty_ms": empty_ms}
        if gemm_impl == "mfma":
            achieved = ops_per_step / (burst_ms * 1e-3) / 1e12
            roofline = {"bound": "mfma", "kernel_name": ops.nib_gemm_kernel_name(B, N, K),
                        "kernel": ops.nib_gemm_kernel_name(B, N, K) + " (fp4 MFMA packed GEMM; name from the library's own dispatch)",
                        "achieved": achieved, "peak": MFMA_FP4_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / MFMA_FP4_PEAK_TFLOPS,
                        "frac_on_in_step_bracket": ops_per_step / (gemm_ms * 1e-3) / 1e12 / MFMA_FP4_PEAK_TFLOPS,
                        "traffic": None, **timing,
                        "hbm_equiv": {"algorithmic_bytes": gemm_bytes,
                                      "achieved_GBs": gemm_bytes / (burst_ms * 1e-3) / 1e9,
                                      "frac_of_8TBs": gemm_bytes / (burst_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}}
        else:
            achieved = gemm_bytes / (burst_ms * 1e-3) / 1e9
            valu = ops_per_step / (burst_ms * 1e-3) / 1e12
            roofline = {"bound": "hbm", "kernel_name": "popc_gemm_kernel", "kernel": "popc_gemm_kernel (xnor popcount GEMM, VALU)", "achieved": achieved,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                        **timing, "algorithmic_bytes": gemm_bytes,
                        "note": "at this shape the popcount formulation is VALU-bound, not HBM-bound "
                                "(SURVEY.md 8d); the instruction ceiling is reported beside it",
                        "valu_ceiling": {"achieved_TOPS": valu, "peak_TOPS": VALU_PEAK_TOPS,
                                         "frac": valu / VALU_PEAK_TOPS}}
    step_bytes = 4.0 * (B * K + N * K + B * N) + 4.0 * N  # fp32 in / fp32 out, SURVEY.md 8d
    step_ms = elapsed / args.steps * 1e3
    roofline["step_hbm"] = {"algorithmic_bytes": step_bytes,
                            "achieved_GBs": step_bytes / (step_ms * 1e-3) / 1e9,
                            "frac_of_8TBs": step_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}

    if args.full:
        # HBM-side bytes per launch: counters cannot be read from inside the process, so this is QUOTED from the committed PMC
        # passes of this same command (tools/collect_profiles.sh refreshes profiles/pmc_latest.json), not measured in this run
        roofline["traffic"], src, roofline["rocprof_avg_us"] = pmc_traffic(gemm_impl)
        roofline["traffic_source"] = None if src is None else f"quoted (not measured in this run): {src}"

        c2_ops_level = {"ms_per_step": ops_elapsed / args.steps * 1e3, "TOPS": world * ops_per_step * args.steps / ops_elapsed / 1e12,
                        "what": "ops.pack_linear_operands + ops.packed_gemm called directly (rounds 1-5's headline): the layer's dispatch, "
                                "autograd node and output view are NOT in this figure", "same_result_as_headline": same_as_ops}
    result = {
        "metric": "XNOR-popcount GEMM TOPS (LinearBin 4096x4096 forward, batch 4096 per GPU)",
        "value": value, "unit": "TOPS", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": step_ms, "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None,
        "dtype": "u32 bit planes (xor+popcount), int32 accumulate, fp32 in/out"
                 if gemm_impl != "mfma" else "fp4-e2m1 (+-1 exact) MFMA, fp32 accumulate, fp32 in/out",
        "data": "synthetic",
        "config": {"workload": "c2: LinearBin(4096, 4096).train().forward(x) on fp32 +-1 activations = sign+pack(x) + sign+pack(W) + packed GEMM, "
                               "timed through the module (autograd node included)",
                   "timed_through": "LinearBin.forward (train mode, autograd on, binary_input=True)", "headline_calls": headline_calls,
                   "batch_per_gpu": B, "in_features": K, "out_features": N, "global_batch": B * world,
                   "parallelism": f"batch-shard x{world}, no collective", "gemm_impl": gemm_impl,
                   # un-tagged inputs of the layer-level legs (AlexNet / C4 / C5) are checked for +-1 on the device; "verify" =
                   # one 4-byte readback per un-tagged input per forward (functions/_fused.py); the C2 step itself packs
                   # through ops.* and asks nothing
                   "detect_mode": _fused.detect_mode(), "float_split": ops.current_float_split(),
                   "legs": "every leg of this line runs with detect_mode and float_split above unless its own object says otherwise "
                           "(with_remembered_range_verdicts: detect_mode 'remember'; Lin/Log layers: bf16x3); real-valued first layers: "
                           "AlexNet conv1 on the direct kernel (per-tile two-term fp16 split), VGG conv1 on bf16 triples", "deferred_activations": "on (lazy.ENABLED, lazy.DEFER_CODES): bit-identical "
                   "to the module-by-module graph on this device"},
        "roofline": roofline,
        "per_rank_ms_per_step": per_rank_ms,
        "dist": {"initialised": dist is not None, "backend": (dist.get_backend() if dist is not None else None),
                 "world_size_seen_by_the_process_group": (dist.get_world_size() if dist is not None else 1),
                 "devices": sorted({local_rank}) if dist is None else None,
                 "scaling_measured": "this line is ONE point; the driver computes efficiency from the per-N lines. No N > 1 run "
                                     "has been possible for this repo so far (1-GPU boxes): multi-GPU behaviour is unmeasured"},
    }
    if c2_ops_level is not None:
        result["c2_ops_level"] = c2_ops_level
    if dist is not None:
        names = [None] * world
        dist.all_gather_object(names, f"rank {rank}: cuda:{local_rank} {torch.cuda.get_device_name(dev)} "
                                      f"[{getattr(torch.cuda.get_device_properties(dev), 'uuid', '')}]")
        result["dist"]["devices"] = names
    result["dist"]["self_check"] = dist_self_check(args.gpus, result["dist"]["world_size_seen_by_the_process_group"],
                                                   result["dist"]["devices"] if dist is not None else None)

    if args.full:
        # ---- the same step THROUGH THE MODULE: LinearBin(K, N).train().forward(x) — the layer's dispatch, its
        # autograd node (the weight requires grad: inputs are saved for backward) and the output view are inside this figure; the
        # headline above calls the two ops the layer ends in.  binary_input=True = "the caller guarantees +-1 activations" (what a
        # BinaryConnect in front of the layer establishes in the reference's models); the default None asks the device per call
        # (detect_mode 'verify': one 4-byte readback = a host sync per forward), reported beside it.
        result["c2_layer_forward"] = bench_c2_layer(args, dev, dist, world, x, w, y, ops_per_step, sync_all)
        result["c2_layer_forward"]["headline_is_this_leg"] = "value / ms_per_step above ARE the binary_input=True, autograd-on form of this leg"

        # ---- the reference's own op sequence on THIS GPU (torch.sign + masked write + F.linear fp32 through ROCm PyTorch):
        # what the un-modified QuantTorch package gets here; per-rank work like the headline, a reported baseline only
        if not args.no_extras:
            from oracle import torch_port
            with torch.no_grad():
                yr = torch_port.linear_bin_forward(x, w)
                same = bool(torch.equal(yr, y))
                del yr
                for _ in range(2):
                    torch_port.linear_bin_forward(x, w)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    torch_port.linear_bin_forward(x, w)
                torch.cuda.synchronize()
                ref_ms = (time.perf_counter() - t0) / 10 * 1e3
            result["reference_ops_on_gpu"] = {"value": ops_per_step / (ref_ms * 1e-3) / 1e12, "unit": "TOPS (per GPU)",
                                              "ms_per_step": ref_ms, "same_result": same,
                                              "what": "oracle/torch_port.linear_bin_forward on the device tensors, 10 calls"}

        # ---- BinaryNet-AlexNet images/s (second half of BASELINE.json's metric) ---------------------------
        if args.alexnet_batch > 0:
            result["alexnet"] = bench_alexnet(args, dev, dist, world, rank)
        if not args.no_extras:
            result["extra"] = bench_extras(args, dev, dist, world, rank, x, w)

        # ---- parity gate + CPU baseline (rank 0, N = 1 only) --------------------------------------------
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            from oracle import torch_port
            xc, wc = x.cpu(), w.cpu()
            ref = torch_port.linear_bin_forward(xc, wc)
            result["parity_vs_cpu_port"] = bool(torch.equal(ref, y.cpu()))
            # the host has far more logical CPUs than MKL scales to: use the fastest thread count
            nthreads, _ = torch_port.best_thread_count(lambda: torch_port.linear_bin_forward(xc, wc))
            med, iters = torch_port.time_callable(lambda: torch_port.linear_bin_forward(xc, wc),
                                                  budget_s=args.cpu_budget_s)
            result["cpu_baseline"] = {
                "value": ops_per_step / med / 1e12, "unit": "TOPS", "cores": torch.get_num_threads(),
                "kind": "port", "ms_per_step": med * 1e3,
                "sample": f"{iters} full-size calls of the reference op sequence "
                          f"(torch.sign + masked write + F.linear fp32, B={B} K={K} N={N}), median",
                "host": _cpu_model()}
            # "plus a 1-thread run" — the same op sequence on ONE host core (bounded: 2 calls)
            torch.set_num_threads(1)
            med1, it1 = torch_port.time_callable(lambda: torch_port.linear_bin_forward(xc, wc), budget_s=0.0, warmup=0,
                                                 min_iters=2, max_iters=2)
            torch.set_num_threads(nthreads)
            result["cpu_baseline"]["one_thread"] = {"value": ops_per_step / med1 / 1e12, "unit": "TOPS", "cores": 1,
                                                    "ms_per_step": med1 * 1e3, "sample": f"{it1} full-size calls"}
    if rank == 0:
        result["calls"] = {k: int(v) for k, v in _lib.call_counts.items()}
        detail_paths = write_detail(result) if args.full else ()
        line = compact_line(result, detail_paths)
        print(line)
        sys.stdout.flush()
    if dist is not None:
        dist.destroy_process_group()


LINE_TARGET_BYTES = 6144        # what the final stdout line aims at
LINE_CAP_BYTES = 12288          # hard cap, asserted: round 4's 27 KB line could not be parsed by the driver (BENCH_r04 parsed: null)
C2_HBM_TARGET = 0.70            # north_star: >= 70 % of the HBM-bound roofline for the C2 step
C2_CEILING_CLAIMED = 0.44       # the builder's stated ceiling of the two-launch step (profiles/r3_cu_partition.md)


def gather_per_rank(dist, dev, world, seconds):
    """Every rank's own elapsed time of one timed run (seconds), in rank order; [seconds] without a process group.  Rides beside
    each whole-job number so that a SCALE run is self-checking: a straggler or a rank that did no work shows up here."""
    if dist is None:
        return [float(seconds)]
    gdev = dev if dist.get_backend() == "nccl" else torch.device("cpu")
    got = [torch.zeros(1, device=gdev, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(got, torch.tensor([float(seconds)], device=gdev, dtype=torch.float64))
    return [float(g.item()) for g in got]


def dist_self_check(n_gpus, world_seen, device_names):
    """The N > 1 line checks itself: the process group has as many ranks as --gpus asked for and every rank
    sits on its own device.  ``device_names``: one 'rank r: cuda:i <name> [uuid/pci]' string per rank (None at N = 1)."""
    distinct = None if device_names is None else len({str(n).split(": ", 1)[-1].split(" ")[0] for n in device_names}) == len(device_names)
    ok = bool(world_seen == n_gpus and (distinct is None or distinct or n_gpus == 1))
    return {"world_size_matches_gpus": bool(world_seen == n_gpus), "distinct_devices": distinct, "ok": ok}


def _pick(d, *keys):
    """d[k] for the keys that exist (a leg that was skipped or failed simply leaves its keys out of the compact line)."""
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def _r(v, nd=4):
    """Round floats for the compact line (the detail file keeps every digit)."""
    if isinstance(v, float):
        return float(f"{v:.{nd + 2}g}") if v != 0.0 else 0.0
    if isinstance(v, dict):
        return {k: _r(x, nd) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_r(x, nd) for x in v]
    return v


def dump_outputs(out_dir, arrays, rank=0, world=1):
    """--dump-outputs: each named output of the last timed step as out_dir/<name>.npy in float32 (<name>_rank<r>.npy with more
    than one rank).  Each rank may write DUMP_CAP_BYTES / world, so the ranks together stay within DUMP_CAP_BYTES; a larger
    output is written as the rows picked by a generator seeded with DUMP_SEED, in ascending order: the same rows for the same
    shape in every run, so that two builds can be compared output for output."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    cap = DUMP_CAP_BYTES // max(1, world)
    for name, t in arrays.items():
        t = t.detach().float()
        rows = t.shape[0]
        row_bytes = t[0].numel() * 4 if rows else 0
        if rows and rows * row_bytes > cap:
            keep = max(1, cap // row_bytes)
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(rows, size=keep, replace=False))
            t = t[torch.from_numpy(idx).to(t.device)]
        fname = name if world == 1 else f"{name}_rank{rank}"
        np.save(os.path.join(out_dir, fname + ".npy"), t.cpu().numpy())


def write_detail(result):
    """The full result object (every leg, per-block rooflines, call counters: ~27 KB) goes to side files, never to stdout:
    bench_detail.json next to bench.py and gpurun_out/bench_detail.json (the directory gpurun merges back)."""
    paths = []
    for rel in ("bench_detail.json", os.path.join("gpurun_out", "bench_detail.json")):
        path = os.path.join(ROOT, rel)
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(result, fh, indent=1)
            paths.append(rel)
        except OSError:
            pass
    return paths


def compact_line(result, detail_paths=()):
    """The ONE JSON line of the bench contract, from the full result object: the contract keys verbatim, the roofline of the
    dominant kernel with its own verdict against north_star's target, the CPU baseline, the per-rank times, and one small
    object per other BASELINE config.  Everything else lives in bench_detail.json.  Pure function of `result` (no device),
    so tests/test_bench_line_cpu.py runs it on canned numbers and asserts the size cap and the key set."""
    rf = result.get("roofline", {})
    step_hbm = rf.get("step_hbm", {})
    roofline = _pick(rf, "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "rocprof_avg_us")
    if "kernel_name" in rf:
        roofline["kernel"] = rf["kernel_name"]
    roofline["traffic_measured_in_this_run"] = False if rf.get("traffic") is not None else None
    roofline["algorithmic_bytes"] = rf.get("hbm_equiv", {}).get("algorithmic_bytes", rf.get("algorithmic_bytes"))
    frac_hbm = step_hbm.get("frac_of_8TBs")
    roofline["step_hbm"] = {"algorithmic_bytes": step_hbm.get("algorithmic_bytes"), "achieved_GBs": step_hbm.get("achieved_GBs"),
                            "frac_of_8TBs": frac_hbm, "target": C2_HBM_TARGET,
                            "target_met": (None if frac_hbm is None else bool(frac_hbm >= C2_HBM_TARGET)),
                            "ceiling_claimed": C2_CEILING_CLAIMED, "why": "profiles/r3_cu_partition.md"}
    cfg = _pick(result.get("config", {}), "workload", "timed_through", "batch_per_gpu", "in_features", "out_features", "global_batch", "parallelism",
                "gemm_impl", "detect_mode", "float_split")
    out = {k: result.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                      "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = cfg
    out["roofline"] = roofline
    cb = result.get("cpu_baseline")
    if cb is not None:
        out["cpu_baseline"] = _pick(cb, "value", "unit", "cores", "kind", "sample", "host")
        if "one_thread" in cb:
            out["cpu_baseline"]["one_thread"] = _pick(cb["one_thread"], "value", "cores")
    if "parity_vs_cpu_port" in result:
        out["parity_vs_cpu_port"] = result["parity_vs_cpu_port"]
    out["per_rank_ms_per_step"] = result.get("per_rank_ms_per_step")
    out["dist"] = _pick(result.get("dist", {}), "initialised", "backend", "world_size_seen_by_the_process_group", "self_check")
    if isinstance(result.get("c2_ops_level"), dict):
        out["c2_ops_level"] = _pick(result["c2_ops_level"], "ms_per_step", "TOPS", "same_result_as_headline")
    cl = result.get("c2_layer_forward")
    if isinstance(cl, dict):
        out["c2_layer_forward"] = _pick(cl, "ms_per_step", "TOPS", "same_result_as_ops_level_step", "error")
        out["c2_layer_forward"]["what"] = "re-run of the headline form (LinearBin.train().forward, binary_input=True); detect_on_device_ms = binary_input=None"
        if "detect_on_device" in cl:
            out["c2_layer_forward"]["detect_on_device_ms"] = cl["detect_on_device"].get("ms_per_step")
    if "reference_ops_on_gpu" in result:
        out["reference_ops_on_gpu"] = _pick(result["reference_ops_on_gpu"], "value", "ms_per_step", "same_result")
    a = result.get("alexnet")
    if isinstance(a, dict):
        al = _pick(a, "images_per_s", "batch_per_gpu", "ms_per_forward", "frac_of_matrix_floor", "per_rank_ms_per_forward")
        al["workload"] = "c3: BinaryNet-AlexNet 3x224x224 eval forward, un-modified module graph, whole job over all ranks"
        x_ = a.get("xnor_flavour", {})
        al["xnor_images_per_s"] = x_.get("images_per_s")
        al["xnor_vs_binarynet"] = x_.get("vs_binarynet_flavour")
        al["fused_images_per_s"] = a.get("fused", {}).get("images_per_s")
        al["same_logits_fused_vs_module_graph"] = a.get("fused", {}).get("same_logits_as_module_graph")
        al["reference_ops_on_gpu_images_per_s"] = a.get("reference_ops_on_gpu", {}).get("images_per_s")
        if "cpu_baseline" in a:
            al["cpu_images_per_s"] = a["cpu_baseline"].get("images_per_s")
            al["cpu_cores"] = a["cpu_baseline"].get("cores")
        ar = a.get("roofline", {})
        al["roofline"] = _pick(ar, "bound", "dominant_block", "achieved", "peak", "unit", "frac", "dominant_block_ms", "matrix_floor_ms")
        al["block_ms"] = {r["block"]: r["ms"] for r in ar.get("blocks", []) if "ops" in r}
        out["alexnet"] = al
    ex = result.get("extra")
    if isinstance(ex, dict):
        e = {}
        c4 = ex.get("c4_dorefa_resnet18_w1a4", {})
        if c4:
            e["c4"] = {leg: _pick(c4[leg], "images_per_s", "ms_per_forward") | _pick(c4[leg].get("roofline", {}), "frac_of_matrix_peak")
                       for leg in ("module_graph", "module_graph_eager", "module_graph_hipgraph", "fused", "fused_hipgraph") if isinstance(c4.get(leg), dict)}
            e["c4"]["module_graph"]["implicit_hipgraph_replays"] = c4.get("module_graph", {}).get("implicit_hipgraph", {}).get("replays")
        c5 = ex.get("c5_ternary_vgg16", {})
        if c5:
            e["c5"] = {leg: _pick(c5[leg], "images_per_s", "ms_per_forward") | _pick(c5[leg].get("roofline", {}), "frac_of_matrix_peak")
                       for leg in ("module_graph", "fused") if isinstance(c5.get(leg), dict)}
            e["c5"]["global_batch"] = c5.get("global_batch")
            e["c5"]["per_rank_ms_per_forward"] = c5.get("per_rank_ms_per_forward")
        ev = ex.get("c2_eval_prepacked", {})
        if ev:
            e["c2_eval"] = _pick(ev, "layer_forward_us", "gemm_only_us", "TOPS_layer", "same_as_train_mode")
        if "c2_bias_tail" in ex:
            e["c2_bias_tail"] = _pick(ex["c2_bias_tail"], "norm_err_vs_fp64", "tolerance", "pass")
        hb = ex.get("popcount_gemm_hbm_regime", {}).get("shapes")
        if hb:
            big = max(hb, key=lambda r_: r_["bytes"])
            e["popcount_hbm_regime"] = _pick(big, "M", "N", "K", "us", "GBs", "frac_of_8TBs", "bit_exact")
        for key, short in (("n2_training_step_alexnet_bin", "train_alexnet_bin"), ("n2_training_step_alexnet_xnor", "train_alexnet_xnor"),
                           ("n2_training_step_dorefa_resnet18_w1a4", "train_dorefa_resnet18")):
            t = ex.get(key)
            if isinstance(t, dict):
                e[short] = _pick(t, "ms_per_step", "images_per_s", "loss", "loss_reference_ops", "first_step_ties", "global_batch", "error")
                if "reference_ops_on_gpu" in t:
                    e[short]["reference_ops_on_gpu_ms"] = t["reference_ops_on_gpu"].get("ms_per_step")
                if "dense_library_calls_in_the_steps" in t:
                    e[short]["dense_library_calls"] = t["dense_library_calls_in_the_steps"]
        out["extra"] = e
    if detail_paths:
        out["detail"] = {"files": list(detail_paths), "what": "full result object: every leg, per-block rooflines, C-ABI call counters"}
    out = _r(out)
    line = json.dumps(out, separators=(",", ":"))
    if len(line) > LINE_TARGET_BYTES:                       # shed the optional objects first, the contract keys never
        for key in ("extra", "reference_ops_on_gpu"):
            out.pop(key, None)
            line = json.dumps(out, separators=(",", ":"))
            if len(line) <= LINE_TARGET_BYTES:
                break
    assert len(line) < LINE_CAP_BYTES, f"bench line is {len(line)} bytes (cap {LINE_CAP_BYTES}): the driver cannot parse long lines"
    assert "\n" not in line
    return line


def self_launch(nproc: int):
    """`python bench.py --gpus N` without a launcher: run this same command line as N ranks of one node under
    torch.distributed.run (what the driver does by hand), inherit stdout / stderr, and exit with the job's status."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:       # a free rendezvous port on the loopback
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")                   # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or nproc) // nproc)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def launch_check(args, world: int, rank: int):
    """--launch-check: the rendezvous, barrier and MAX reduction of the timed region with no device work (host tensors, so the
    gloo backend serves it on a machine without a GPU); rank 0 prints one JSON line."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    backend = args.dist_backend if (args.dist_backend != "nccl" or torch.cuda.is_available()) else "gloo"
    if backend == "nccl":
        lr = 0 if args.share_device else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(lr)
        dist.init_process_group("nccl", device_id=torch.device("cuda", lr))
        tdev = torch.device("cuda", lr)
    else:
        dist.init_process_group(backend)
        tdev = torch.device("cpu")
    dist.barrier()
    tt = torch.tensor([float(rank + 1)], device=tdev, dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    ranks = [None] * world
    dist.all_gather_object(ranks, (rank, os.getpid()))
    # the per-rank lists of the C3 / C5 legs (gather_per_rank) and the self-check, through the code the measured run uses: each
    # rank contributes a distinct stand-in time, rank 0 assembles the same compact line (tests/test_dist_gloo.py reads it)
    per = gather_per_rank(dist, tdev, world, 1e-3 * (rank + 1))
    names = [None] * world
    dist.all_gather_object(names, f"rank {rank}: {'cuda' if backend == 'nccl' else 'host-process'}:{rank if backend != 'nccl' else lr} launch-check")
    if rank == 0:
        fake = {"metric": "launch-check", "n_gpus": args.gpus, "per_rank_ms_per_step": [p_ * 1e3 for p_ in per],
                "dist": {"initialised": True, "backend": dist.get_backend(), "world_size_seen_by_the_process_group": dist.get_world_size(),
                         "devices": names, "self_check": dist_self_check(args.gpus, dist.get_world_size(), names)},
                "alexnet": {"images_per_s": 0.0, "per_rank_ms_per_forward": [p_ * 1e3 for p_ in per]},
                "extra": {"c5_ternary_vgg16": {"module_graph": {"images_per_s": 0.0}, "global_batch": 256 * world,
                                               "per_rank_ms_per_forward": [p_ * 1e3 for p_ in per]}}}
        line = json.loads(compact_line(fake))
        print(json.dumps({"launch_check": True, "n_gpus": args.gpus,
                          "dist": {"initialised": True, "backend": dist.get_backend(),
                                   "world_size_seen_by_the_process_group": dist.get_world_size(),
                                   "max_over_ranks": float(tt.item()), "ranks": sorted(r for r, _ in ranks),
                                   "distinct_processes": len({p for _, p in ranks}),
                                   "self_check": line["dist"]["self_check"]},
                          "compact_line_per_rank": {"c3": line["alexnet"]["per_rank_ms_per_forward"],
                                                    "c5": line["extra"]["c5"]["per_rank_ms_per_forward"]}}))
    dist.destroy_process_group()


def bench_c2_layer(args, dev, dist, world, x, w, y_ops, ops_per_step, sync_all):
    """C2 timed through `LinearBin.forward` in training mode (layers/binary_layers.py:42-46 of the reference)."""
    from pytorch_quantize_impls_amd.layers import LinearBin
    B, K = x.shape
    N = w.shape[0]
    layer = LinearBin(K, N, bias=False).to(dev)
    layer.weight.data.copy_(w)
    layer.train()
    out = {"what": "LinearBin(4096, 4096, bias=False).train()(x), x = fp32 +-1 resident in HBM, autograd on (weight.requires_grad): "
                   "dispatch + sign/pack of both operands + packed GEMM + autograd node; same barrier / synchronize bracket and MAX "
                   "over ranks as the headline"}

    def run(n):
        for _ in range(max(3, args.warmup)):
            yl = layer(x)
        sync_all()
        t0 = time.perf_counter()
        for _ in range(n):
            yl = layer(x)
        torch.cuda.synchronize()
        e = time.perf_counter() - t0
        sync_all()
        if dist is not None:
            tt = torch.tensor([e], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            e = float(tt.item())
        return e / n * 1e3, yl

    try:
        layer.binary_input = True
        ms, yl = run(args.steps)
        out.update({"ms_per_step": ms, "TOPS": world * ops_per_step / (ms * 1e-3) / 1e12, "binary_input": True,
                    "same_result_as_ops_level_step": bool(torch.equal(yl.detach(), y_ops)), "has_grad_fn": yl.grad_fn is not None})
        with torch.no_grad():
            ms_ng, _ = run(args.steps)
        out["no_grad"] = {"ms_per_step": ms_ng, "TOPS": world * ops_per_step / (ms_ng * 1e-3) / 1e12}
        layer.binary_input = None
        ms_d, yd = run(max(5, args.steps // 4))
        out["detect_on_device"] = {"ms_per_step": ms_d, "TOPS": world * ops_per_step / (ms_d * 1e-3) / 1e12,
                                   "same_result": bool(torch.equal(yd.detach(), y_ops)),
                                   "what": "binary_input=None: the un-tagged activation is checked for +-1 on the device every call"}
    except Exception as exc:  # noqa: BLE001 — a side leg must not void the headline
        out["error"] = f"{type(exc).__name__}: {exc}"
    return out


def bench_alexnet(args, dev, dist, world, rank):
    """BinaryNet-AlexNet (models/Alexnet/Alexnet_Bin.py topology) eval-mode
    forward, 3x224x224, batch per GPU = --alexnet-batch, channels_last, weights pre-quantised and
    pre-packed by .eval() (the reference's eval protocol)."""
    import bench_models
    B = args.alexnet_batch
    torch.manual_seed(1234 + rank)
    model = bench_models.AlexNetBin()
    bench_models.randomize_bn(model)
    model = model.to(dev).to(memory_format=torch.channels_last).eval()
    x = torch.randn((B, 3, 224, 224), device=dev).contiguous(memory_format=torch.channels_last)
    def timed(fn):
        """`alexnet_iters` forwards, barrier + sync on both sides, MAX over ranks; best of 3 such runs (a
        one-off host stall of tens of ms otherwise dominates a 5-forward sample)."""
        best, last = None, None
        with torch.no_grad():
            for _ in range(3):
                last = fn(x)
            for _ in range(3):
                torch.cuda.synchronize()
                if dist is not None:
                    dist.barrier()
                t0 = time.perf_counter()
                for _ in range(args.alexnet_iters):
                    last = fn(x)
                torch.cuda.synchronize()
                e = time.perf_counter() - t0
                per = gather_per_rank(dist, dev, world, e)
                if dist is not None:
                    tt = torch.tensor([e], device=dev, dtype=torch.float64)
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    e = float(tt.item())
                if best is None or e < best:
                    best, timed.per_rank_ms = e, [p_ / args.alexnet_iters * 1e3 for p_ in per]
        return best, last

    from pytorch_quantize_impls_amd import lazy
    lazy.STATS.clear()
    el, y = timed(model)
    stats = dict(lazy.STATS)
    out = {"images_per_s": world * B * args.alexnet_iters / el, "batch_per_gpu": B,
           "ms_per_forward": el / args.alexnet_iters * 1e3, "per_rank_ms_per_forward": list(timed.per_rank_ms),
           "mode": "eval (pre-packed weights), channels_last, the reference's module-by-module nn.Sequential graph, un-modified; "
                   "binarised convs return deferred activations (lazy.py) so the graph executes as the fused chain; "
                   "best of 3 runs of alexnet_iters forwards",
           "deferred_convs_per_forward": stats.get("deferred", 0) / max(1, 3 + 3 * args.alexnet_iters),
           "materialised": stats.get("materialised", 0),
           "macs_per_image": 4.9349e9, "finite": bool(torch.isfinite(y).all())}
    # the same un-modified graph with deferral switched off: every module computes its fp32 output (r1 / early-r2 numbers)
    with lazy.eager():
        ele, ye = timed(model)
    out["module_by_module_eager"] = {"images_per_s": world * B * args.alexnet_iters / ele,
                                     "ms_per_forward": ele / args.alexnet_iters * 1e3,
                                     "same_logits_as_deferred": bool(torch.equal(ye, y)),
                                     "same_argmax_as_deferred": bool(torch.equal(ye.argmax(1), y.argmax(1)))}
    # same network fused for inference (layers.fused): every BinConv2d emits BatchNorm-threshold bits, MaxPool runs
    # on bits, FC blocks use the BN+Hardtanh+sign+pack kernel: no fp32 activation between binarised layers
    fused = bench_models.FusedAlexNetBin(model, fold="device")
    elf, yf = timed(fused)
    out["fused"] = {"images_per_s": world * B * args.alexnet_iters / elf,
                    "ms_per_forward": elf / args.alexnet_iters * 1e3,
                    "same_logits_as_module_graph": bool(torch.equal(yf, y)),
                    "same_logits_as_unfused": bool(torch.equal(yf, ye)),
                    "bn_fold": "device (thresholds of this device's F.batch_norm: bit-identical to the module graph)"}
    out["roofline"] = alexnet_roofline(model, fused, x, B)
    floor = out["roofline"]["matrix_floor_ms"]
    out["frac_of_matrix_floor"] = floor / out["ms_per_forward"]
    out["module_by_module_eager"]["frac_of_matrix_floor"] = floor / out["module_by_module_eager"]["ms_per_forward"]
    out["fused"]["frac_of_matrix_floor"] = floor / out["fused"]["ms_per_forward"]
    # SURVEY 8d asks for the train-mode form as well: the quantised layers in training mode (sign + pack of W on every
    # call, STE autograd nodes), BatchNorm kept on its running statistics for determinism
    from pytorch_quantize_impls_amd.layers import BinConv2d, LinearBin
    qlayers = [m for m in model.modules() if isinstance(m, (BinConv2d, LinearBin))]
    for m in qlayers:
        m.train()
    elt, yt = timed(model)
    for m in qlayers:
        m.eval()
    out["train_mode_layers"] = {"images_per_s": world * B * args.alexnet_iters / elt,
                                "ms_per_forward": elt / args.alexnet_iters * 1e3,
                                "frac_of_matrix_floor": floor / (elt / args.alexnet_iters * 1e3),
                                "same_logits_as_eval": bool(torch.equal(yt, ye))}
    # the reference's own op sequence (torch.sign + F.conv2d / F.linear fp32 + the torch modules) on THIS GPU: what the
    # un-modified QuantTorch package gets from ROCm PyTorch (MIOpen / hipBLASLt) for the same eval forward
    from oracle import torch_port

    def ref_ops(xin):
        h = torch_port.sequential_forward(model.features, xin)
        return torch_port.sequential_forward(model.classifieur, h.reshape(h.size(0), 256 * 6 * 6))
    elr, yr = timed(ref_ops)
    out["reference_ops_on_gpu"] = {"images_per_s": world * B * args.alexnet_iters / elr,
                                   "ms_per_forward": elr / args.alexnet_iters * 1e3,
                                   "same_argmax_as_module_by_module": bool(torch.equal(yr.argmax(1), ye.argmax(1))),
                                   "what": "oracle/torch_port.sequential_forward: the reference's eval-mode ops in torch on the device"}
    out["xnor_flavour"] = bench_alexnet_xnor(args, dev, world, timed, x, out)
    # small-batch serving: the un-modified module graph at batch 1 / 8 / 32, eager (host-bound: ~25 Python-driven launches)
    # and replayed as a hipGraph captured from the same model (utils.graphed; per-rank latencies, no aggregation)
    if not args.no_extras:
        from pytorch_quantize_impls_amd import utils
        serving = {}
        for sb in (1, 8, 32):
            xs = torch.randn((sb, 3, 224, 224), device=dev).contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                want = model(xs)
                gm = utils.graphed(model, xs)
                same = bool(torch.equal(gm(xs), want))

                def lat(fn, n=30):
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / n * 1e3
                te, tg = lat(lambda: model(xs)), lat(lambda: gm(xs))
                with lazy.eager():
                    tm = lat(lambda: model(xs))
                # utils.auto_graphed: the wrapper a serving loop would use — eager on the first call with a signature,
                # captured on the second, replayed (input copied in, output copied out) from then on
                am = utils.auto_graphed(model)
                same_a = bool(torch.equal(am(xs), want)) and bool(torch.equal(am(xs), want))
                ta = lat(lambda: am(xs))
            serving[f"batch_{sb}"] = {"eager_ms": te, "module_by_module_eager_ms": tm, "hipgraph_ms": tg,
                                      "hipgraph_images_per_s": sb / tg * 1e3, "same_logits": same,
                                      "auto_graphed_ms": ta, "auto_graphed_same_logits": same_a, "auto_graphed_replays": am.replays,
                                      "auto_graphed_capture_failures": dict(am.capture_failures)}
            del gm, am
        out["serving_small_batch"] = serving
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cb = B                       # the same batch as the GPU leg (one forward = ~1 s on the box's host)
        cpu_model = bench_models.AlexNetBin()
        cpu_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        cpu_model.eval()
        xc = x[:cb].cpu().contiguous()
        from oracle import torch_port
        with torch.no_grad():
            torch_port.best_thread_count(lambda: cpu_model(xc), probe_iters=1)
            med, iters = torch_port.time_callable(lambda: cpu_model(xc), budget_s=min(args.cpu_budget_s, 8.0))
        out["cpu_baseline"] = {"images_per_s": cb / med, "batch": cb, "cores": torch.get_num_threads(),
                               "kind": "port", "sample": f"{iters} forwards of the same topology on CPU tensors, median"}
        nthr = torch.get_num_threads()
        torch.set_num_threads(1)
        x1 = xc[:4].contiguous()
        with torch.no_grad():
            med1, it1 = torch_port.time_callable(lambda: cpu_model(x1), budget_s=0.0, warmup=1, min_iters=2, max_iters=2)
        torch.set_num_threads(nthr)
        out["cpu_baseline"]["one_thread"] = {"images_per_s": 4 / med1, "batch": 4, "cores": 1, "sample": f"{it1} forwards"}
    return out


def bench_alexnet_xnor(args, dev, world, timed, x, bin_out):
    """The XNOR-Net flavour BASELINE config 3 is named after: utils.xnor_net_convert of the same topology —
    XNORConv2d(dim = [0, 1]) / LinearXNOR (layers/xnor_layers.py, functions/xnor_connect.py:93-169).  Behind a BinaryConnect every
    conv is  sum_taps alpha[i, j] * (integer dot over Cin): one fp4 matrix-core pass with the taps' alphas applied on the
    accumulators (csrc/conv_taps.hip); the first layer (real pixels x real sign(W) * alpha) runs on the direct first-layer kernel with
    two-term fp16 weights; LinearXNOR on packed bits runs in integer form (alpha as three 7-bit digits, one split-K int8 GEMM)."""
    import bench_models
    from pytorch_quantize_impls_amd import lazy
    from pytorch_quantize_impls_amd.layers import XNORConv2d, LinearXNOR, FusedFeatureClassifier
    from pytorch_quantize_impls_amd.functions import _fused
    B = args.alexnet_batch
    torch.manual_seed(4321)
    xm = bench_models.alexnet_xnor()
    for mod in xm.modules():            # the converter hands out fresh layers: give them weights of a trained-looking scale
        if isinstance(mod, (XNORConv2d, LinearXNOR)):
            mod.weight.data.normal_(0, 0.05)
            mod.bias.data.zero_()
    bench_models.randomize_bn(xm)
    xm = xm.to(dev).to(memory_format=torch.channels_last).eval()
    before = dict(_fused.LIBRARY_PATHS)
    lazy.STATS.clear()
    el, y = timed(xm)
    stats = dict(lazy.STATS)
    iters = args.alexnet_iters
    out = {"what": bench_alexnet_xnor.__doc__.split("\n")[0],
           "images_per_s": world * B * iters / el, "ms_per_forward": el / iters * 1e3, "batch_per_gpu": B,
           "mode": "eval, channels_last, the un-modified module graph (deferred activations), best of 3 runs",
           "deferred_convs_per_forward": stats.get("deferred", 0) / max(1, 3 + 3 * iters), "materialised": stats.get("materialised", 0),
           "finite": bool(torch.isfinite(y).all()),
           "vs_binarynet_flavour": (el / iters * 1e3) / bin_out["ms_per_forward"]}
    with lazy.eager():
        ele, ye = timed(xm)
    out["module_by_module_eager"] = {"images_per_s": world * B * iters / ele, "ms_per_forward": ele / iters * 1e3,
                                     "same_logits_as_deferred": bool(torch.equal(ye, y))}
    fused = FusedFeatureClassifier(xm.features, xm.classifieur, (256, 6, 6), fold="device")
    elf, yf = timed(fused)
    out["fused"] = {"images_per_s": world * B * iters / elf, "ms_per_forward": elf / iters * 1e3,
                    "same_logits_as_module_graph": bool(torch.equal(yf, y)),
                    "vs_binarynet_flavour_fused": (elf / iters * 1e3) / bin_out["fused"]["ms_per_forward"]}
    out["roofline"] = alexnet_roofline(xm, fused, x, B)
    out["dense_library_calls"] = {k: v - before.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != before.get(k, 0)}
    out["parity"] = ("tests/test_gpu_r4.py: reference digests (power-of-two-per-tap weights, bit-exact), fp64 vectors of the reference "
                     "functions forward + backward <= 1e-5, deferred graph == module-by-module graph (torch.equal)")
    return out


BF16_PEAK_TFLOPS = 2500.0       # dense bf16 MFMA (MI355X_MICROARCH.md); fp16 has the same rate


def alexnet_roofline(model, fused, x, B):
    """Per-block roofline of the fused AlexNet forward, measured live: every block of the fused form (conv [+ pool] +
    BatchNorm-threshold epilogue; FC + BatchNorm + sign) is run alone, 10 launches back to back inside one HIP-event pair.
    ops = 2 * MACs of SURVEY Appendix A.1 (full taps, padding counted); peak = the matrix-core peak of the element type the
    block's contraction runs in (conv1: real pixels, exact bf16 split -> bf16 peak; the other blocks: fp4); bytes = what the
    packed path moves algorithmically (input plane + packed weights + output bits), against 8 TB/s.  The floor of the whole
    forward = sum of ops / peak over the blocks; every leg of the 'alexnet' object is given as a fraction of it."""
    from pytorch_quantize_impls_amd.layers import BinConv2d, LinearBin, XNORConv2d, LinearXNOR
    from pytorch_quantize_impls_amd.layers.fused import FusedConvPoolBnSign
    BinConv2d, LinearBin = (BinConv2d, XNORConv2d), (LinearBin, LinearXNOR)        # both flavours of config 3
    net = fused.net if hasattr(fused, "net") else fused
    blocks = list(net.features.children()) + list(net.classifier.children())
    rows, floor_ms = [], 0.0
    with torch.no_grad():
        act = x
        i = 0
        feats = list(net.features.children())
        for bi, blk in enumerate(blocks):
            if bi == len(feats):
                act = act.flatten_hwc()
            inp = act
            for _ in range(3):
                out_ = blk(inp)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                out_ = blk(inp)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 10
            act = out_
            conv = blk.conv if isinstance(blk, FusedConvPoolBnSign) else (blk if isinstance(blk, LinearBin) else None)
            if conv is None:
                rows.append({"block": type(blk).__name__, "ms": ms})
                continue
            w = conv.weight
            if isinstance(conv, BinConv2d):
                N_, C_, H_, W_ = (int(v) for v in inp.shape)
                from pytorch_quantize_impls_amd import ops as _ops
                Ho, Wo = _ops.conv_out_hw(H_, W_, conv.kernel_size[0], conv.kernel_size[1], conv.stride, conv.padding, conv.dilation)
                macs = float(N_ * Ho * Wo * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3])
                real_in = bi == 0
                in_bytes = N_ * C_ * H_ * W_ * (4.0 if real_in else 0.5)          # fp32 pixels / fp4 nibble plane
                out_bytes = N_ * w.shape[0] * Ho * Wo / 8.0                          # threshold bits (before pooling)
                name = f"conv{i + 1} {C_}->{w.shape[0]} k{conv.kernel_size[0]} s{conv.stride[0]} @{H_}"
            else:
                N_ = int(inp.shape[0])
                macs = float(N_ * w.shape[0] * w.shape[1])
                real_in = False
                in_bytes = N_ * w.shape[1] / 8.0
                out_bytes = N_ * w.shape[0] * 4.0
                name = f"fc {w.shape[1]}->{w.shape[0]}"
            i += 1
            peak = BF16_PEAK_TFLOPS if real_in else MFMA_FP4_PEAK_TFLOPS
            w_bytes = w.numel() * (2.0 if real_in else 0.5)
            ops_ = 2.0 * macs
            nbytes = in_bytes + w_bytes + out_bytes
            floor_ms += ops_ / (peak * 1e12) * 1e3
            rows.append({"block": name, "ms": ms, "ops": ops_, "achieved_TFLOPs": ops_ / (ms * 1e-3) / 1e12,
                         "peak_TFLOPs": peak, "peak": "bf16 MFMA dense" if real_in else "fp4 MFMA dense",
                         "frac": ops_ / (ms * 1e-3) / 1e12 / peak, "algorithmic_bytes_packed": nbytes,
                         "frac_of_8TBs": nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
    timed_rows = [r for r in rows if "ops" in r]
    dom = max(timed_rows, key=lambda r: r["ms"])
    total = sum(r["ms"] for r in rows)
    return {"what": alexnet_roofline.__doc__.split("\n")[0],
            "bound": "mfma", "dominant_block": dom["block"], "achieved": dom["achieved_TFLOPs"], "peak": dom["peak_TFLOPs"],
            "unit": "TFLOP/s", "frac": dom["frac"], "dominant_block_ms": dom["ms"], "sum_of_blocks_ms": total,
            "matrix_floor_ms": floor_ms, "blocks": rows,
            "kernel_names": "profiles/r4d_bench_kernel_stats.csv lists the kernels of each block (conv1: conv_first_direct_kernel<real weights?, "
                            "threshold bits, 18> + pool_bits_kernel; conv2-5: mfma_gemm_kernel<ElemFp4 conv-valid, bits epilogue> (XNOR flavour: "
                            "<ElemFp4Taps>) [+ pool_bits_kernel]; fc: mfma_gemm_kernel<ElemFp4 skinny> (XNOR flavour: bits_alpha_digits_kernel + mfma_gemm_kernel<ElemI8, 256x256, split-K> + digit_reduce_kernel; 10-way head: xnor_head_kernel))"}


def _layer_stats(model, x):
    """SURVEY.md 8(d) figures of one forward: ops = 2 * MACs and algorithmic bytes = 4 * (inputs + weights + outputs) summed
    over the quantised Linear / Conv2d layers (full taps, padding counted), from forward hooks on the un-fused model."""
    from pytorch_quantize_impls_amd.layers.common import QLayer
    acc = {"macs": 0.0, "bytes": 0.0, "layers": 0}

    def hook(mod, inp, out):
        xin = inp[0]
        w = mod.weight
        if out.dim() == 4:
            macs = out.shape[0] * out.shape[1] * out.shape[2] * out.shape[3] * w.shape[1] * w.shape[2] * w.shape[3]
        else:
            macs = out.numel() * w.shape[1]
        acc["macs"] += float(macs)
        acc["bytes"] += 4.0 * (xin.numel() + w.numel() + out.numel())
        acc["layers"] += 1

    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, QLayer)]
    with torch.no_grad():
        model(x)
    for h in hs:
        h.remove()
    return acc


def _net_line(name, B, world, iters, el, stats, peak_tflops, peak_name, extra=None, fp32_activations=False):
    """``fp32_activations``: the leg really moves SURVEY 8(d)'s fp32 bytes (module by module); the fused / deferred legs keep
    activations as bit / nibble / code planes, so an fp32-byte rate would be meaningless there (> 8 TB/s) and is not given."""
    ms = el / iters * 1e3
    ops_ = 2.0 * stats["macs"]
    d = {"images_per_s": world * B * iters / el, "batch_per_gpu": B, "ms_per_forward": ms,
         "roofline": {"bound": "mfma", "ops_per_forward": ops_, "quantised_layers": stats["layers"],
                      "achieved_TFLOPs": ops_ / (ms * 1e-3) / 1e12, "peak_TFLOPs": peak_tflops, "peak": peak_name,
                      "frac_of_matrix_peak": ops_ / (ms * 1e-3) / 1e12 / peak_tflops}}
    if fp32_activations:
        d["roofline"].update({"algorithmic_bytes_fp32": stats["bytes"], "hbm_equiv_GBs": stats["bytes"] / (ms * 1e-3) / 1e9,
                              "frac_of_8TBs": stats["bytes"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
    if extra:
        d.update(extra)
    return d


def bench_extras(args, dev, dist, world, rank, x, w):
    """The BASELINE configs the headline does not cover, timed in this process (driver-visible), N ranks like the headline."""
    import bench_models
    from pytorch_quantize_impls_amd import ops
    from pytorch_quantize_impls_amd.functions import BinaryConnectDeterministic
    from pytorch_quantize_impls_amd.layers import LinearBin, FusedFeatureClassifier
    out = {}
    iters = args.extra_iters

    def timed(fn, n=iters):
        best = None
        with torch.no_grad():
            for _ in range(3):
                fn()
            for _ in range(3):
                torch.cuda.synchronize()
                if dist is not None:
                    dist.barrier()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                e = time.perf_counter() - t0
                per = gather_per_rank(dist, dev, world, e)
                if dist is not None:
                    tt = torch.tensor([e], device=dev, dtype=torch.float64)
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    e = float(tt.item())
                if best is None or e < best:
                    best, timed.per_rank_ms = e, [p_ / n * 1e3 for p_ in per]
        return best

    # ---- C2, eval mode: weights pre-packed by .eval(), activation handed over packed by BinaryConnect
    B, K = x.shape
    N = w.shape[0]
    layer = LinearBin(K, N, bias=False).to(dev)
    layer.weight.data.copy_(w)
    layer.eval()
    with torch.no_grad():
        xs = BinaryConnectDeterministic.apply(x)                 # +-1 fp32 image + sign plane (tag)
        y_eval = layer(xs)
        impl = ops.select_gemm_impl("auto", B, N, K)
        xp, wp = ops.pack_linear_operands(x, w, "binary", impl)
        yb = torch.empty((B, N), device=dev)
        n2 = 50
        t_layer = timed(lambda: layer(xs), n2)
        t_gemm = timed(lambda: ops.packed_gemm(xp, wp, None, out=yb, impl=impl), n2)
    bytes_packed = B * K / 8.0 + N * K / 8.0 + 4.0 * B * N          # SURVEY 8(d) bytes_packed (1 bit / element operands)
    bytes_operand = ops.packed_gemm_algorithmic_bytes(B, N, K, impl)
    ops2 = 2.0 * B * K * N
    out["c2_eval_prepacked"] = {
        "workload": "LinearBin.eval() forward on a BinaryConnect-tagged activation (bit plane -> operand format -> packed GEMM); "
                    "and the packed GEMM alone on pre-packed operands",
        "layer_forward_us": t_layer / n2 * 1e6, "gemm_only_us": t_gemm / n2 * 1e6,
        "TOPS_layer": world * ops2 * n2 / t_layer / 1e12, "TOPS_gemm_only": world * ops2 * n2 / t_gemm / 1e12,
        "roofline": {"bytes_packed_1bit": bytes_packed, "hbm_floor_us": bytes_packed / (HBM_PEAK_GBS * 1e9) * 1e6,
                     "frac_of_8TBs_layer": bytes_packed / (t_layer / n2) / 1e9 / HBM_PEAK_GBS,
                     "frac_of_8TBs_gemm_only": bytes_packed / (t_gemm / n2) / 1e9 / HBM_PEAK_GBS,
                     "operand_format_bytes": bytes_operand,
                     "matrix_frac_gemm_only": ops2 / (t_gemm / n2) / 1e12 / MFMA_FP4_PEAK_TFLOPS if impl == "mfma" else None},
        "same_as_train_mode": None}
    # ---- C2 with a bias ~ N(0, 1): the float tail, against the fp64 evaluation and the CPU port
    gb = torch.Generator(device=dev)
    gb.manual_seed(77)
    bias = torch.randn((N,), device=dev, generator=gb)
    with torch.no_grad():
        y_b = ops.packed_gemm(xp, wp, bias, impl=impl)
        y_i = ops.packed_gemm(xp, wp, None, impl=impl)
        out["c2_eval_prepacked"]["same_as_train_mode"] = bool(torch.equal(y_i, y_eval))
        ref64 = y_i.double() + bias.double()                       # exact integers + bias in fp64
        err = float((y_b.double() - ref64).abs().max() / ref64.abs().max())
    tail = {"bias": "N(0,1)", "norm_err_vs_fp64": err, "tolerance": 1e-5, "pass": err <= 1e-5}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import torch_port
        rows = slice(0, 512)
        ref = torch_port.linear_bin_forward(x[rows].cpu(), w.cpu(), bias.cpu())
        tail["norm_err_vs_cpu_port_512_rows"] = float((y_b[rows].cpu() - ref).abs().max() / ref.abs().max())
    out["c2_bias_tail"] = tail

    # ---- the XNOR-popcount GEMM where it IS HBM-bound (north_star's named formulation): a handful of rows on one side, the packed
    # weight planes streamed once (csrc/popc_stream.hip: K along the lanes, DPP wavefront reduction).  Per call inside a captured
    # hipGraph of 20 calls (no launch gaps); bytes = 1-bit operands + the fp32 result (SURVEY 8d bytes_packed).
    try:
        rows_s = []
        with torch.no_grad():
            for (Ms, Ns, Ks) in [(1, 4096, 4096), (1, 4096, 9216), (8, 4096, 9216), (1, 16384, 16384), (256, 10, 4096),
                                 (1, 65536, 65536)]:        # the last one: 537 MB of weight bits, beyond the 256 MB MALL
                gs = torch.Generator(device=dev)
                gs.manual_seed(Ms + Ns + Ks)
                xs_ = torch.randn((Ms, Ks), device=dev, generator=gs)
                ws_ = torch.randn((Ns, Ks), device=dev, generator=gs)
                xps, wps = ops.sign_pack(xs_)[0], ops.sign_pack(ws_)[0]
                ys_ = torch.empty((Ms, Ns), device=dev)
                fn = lambda: ops.xnor_gemm(xps, wps, out=ys_)     # noqa: E731
                fn()
                if Ns * Ks <= (1 << 28):
                    exact = bool(torch.equal(ys_, torch.nn.functional.linear(torch.where(xs_ < 0, -1.0, 1.0).double(),
                                                                             torch.where(ws_ < 0, -1.0, 1.0).double()).float()))
                    exact_what = "fp64 of sign(x) . sign(W)^T"
                else:                                        # fp64 weights would take 34 GB: the tiled popcount kernel instead
                    exact = bool(torch.equal(ys_.clone(), ops.xnor_gemm(xps, wps, variant=1)))
                    exact_what = "the tiled popcount kernel (itself oracle-tested)"
                del xs_, ws_
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    fn()
                    with torch.cuda.graph(gr, stream=side):
                        for _ in range(20):
                            fn()
                torch.cuda.current_stream().wait_stream(side)
                t_s = timed(gr.replay, 20) / (20 * 20)
                byt = (Ms + Ns) * Ks / 8.0 + 4.0 * Ms * Ns
                rows_s.append({"M": Ms, "N": Ns, "K": Ks, "us": t_s * 1e6, "bytes": byt, "GBs": byt / t_s / 1e9,
                               "frac_of_8TBs": byt / t_s / 1e9 / HBM_PEAK_GBS, "bit_exact": exact, "bit_exact_against": exact_what})
                del xps, wps, gr
        out["popcount_gemm_hbm_regime"] = {
            "kernel": "popc_stream_kernel (xor + v_bcnt accumulate, lanes along K, DPP reduction)", "bound": "hbm",
            "peak_GBs": HBM_PEAK_GBS, "shapes": rows_s,
            "what": "LinearBin / classifier-head forward on pre-packed 1-bit planes at batch <= 32 or <= 32 output features; per "
                    "call inside a hipGraph of 20 calls; small shapes are launch-latency bound (~2.5 us floor); 1 x 16384 x 16384 "
                    "(33.5 MB of weight bits) is re-read from the memory-side cache by the repeated calls, 1 x 65536 x 65536 "
                    "(537 MB) is not: that row is the HBM figure"}
    except Exception as e:                                        # an extra: it may not void the headline
        out["popcount_gemm_hbm_regime"] = {"error": repr(e)}

    # ---- C4: DoReFa ResNet-18 W1A4, 3 x 32 x 32
    if args.c4_batch > 0:
        Bc = args.c4_batch
        torch.manual_seed(4 + rank)
        m4 = bench_models.DorefaResNet18(w_bits=1, a_bits=4)
        bench_models.randomize_bn(m4, seed=3)
        for m in m4.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.mul_(4.0)
        m4 = m4.to(dev).to(memory_format=torch.channels_last).eval()
        x4 = torch.randn((Bc, 3, 32, 32), device=dev).contiguous(memory_format=torch.channels_last)
        st4 = _layer_stats(m4, x4)
        from pytorch_quantize_impls_amd import lazy
        f4 = bench_models.FusedDorefaResNet18(m4, fold="device")

        def eager4():
            with lazy.eager():
                return m4(x4)
        def deferred4():
            return m4(x4)
        with torch.no_grad():
            ye4 = eager4()
            yf4 = f4(x4)
            agree = float((yf4.argmax(1) == ye4.argmax(1)).float().mean())
            same_fused = bool(torch.equal(yf4, ye4))
            agree_d = float((deferred4().argmax(1) == ye4.argmax(1)).float().mean())
            same_default = bool(torch.equal(m4(x4), ye4))
        el_u = timed(eager4)
        # the un-modified model, called the way a user calls it: since round 6 such a model replays its forward as a hipGraph by
        # itself from the third identical call on (utils/implicit.py, opt-out); "module_graph_eager" = the same with that switched off
        from pytorch_quantize_impls_amd import utils
        with utils.implicit_graphs(False):
            el_d_eager = timed(deferred4, 2 * iters)
        el_d = timed(deferred4, 2 * iters)
        implicit4 = utils.implicit_graph_stats(m4)
        with torch.no_grad():
            same_implicit = bool(torch.equal(deferred4(), ye4))
        el_f = timed(lambda: f4(x4), 2 * iters)
        # the deferred forward is ~1.7 ms of Python for < 1 ms of GPU work: replayed as a hipGraph (utils.graphed captures
        # the un-modified module; same kernels, no host work)
        from pytorch_quantize_impls_amd import utils
        g4 = utils.graphed(m4, x4)
        with torch.no_grad():
            same_g = bool(torch.equal(g4(x4), deferred4()))
        el_g = timed(lambda: g4(x4), 2 * iters)
        a4 = utils.auto_graphed(m4)                      # "auto-capture a hipGraph on the second identical call"
        with torch.no_grad():
            same_a4 = bool(torch.equal(a4(x4), deferred4())) and bool(torch.equal(a4(x4), deferred4()))
        el_a = timed(lambda: a4(x4), 2 * iters)
        # ... and the opt-in fused form the same way (its eager time is host-bound as well: 26 launches)
        fused_graph = {}
        try:
            gf4 = utils.graphed(f4, x4)
            with torch.no_grad():
                same_gf = bool(torch.equal(gf4(x4), yf4))
            el_gf = timed(lambda: gf4(x4), 2 * iters)
            fused_graph = {"fused_hipgraph": _net_line("c4", Bc, world, 2 * iters, el_gf, st4, 5000.0,
                                                       "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                                                       {"same_logits_as_fused": same_gf})}
            del gf4
        except Exception as exc:
            fused_graph = {"fused_hipgraph": {"error": f"{type(exc).__name__}: {exc}"}}
        out["c4_dorefa_resnet18_w1a4"] = {
            # the un-modified module graph: DorefaConv2d layers return deferred activations, BatchNorm / shortcut add / ReLU /
            # nnDorefaQuant are recorded and run in the conv's code epilogue (lazy.py); the fp32 stem stays module by module
            "module_graph": _net_line("c4", Bc, world, 2 * iters, el_d, st4, 5000.0,
                                      "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                                      {"argmax_agreement_with_unfused": agree_d,
                                       "same_logits_as_module_by_module": same_default and same_implicit,
                                       "implicit_hipgraph": implicit4,
                                       "bn_arithmetic": "this device's eval-mode F.batch_norm, emulated and verified "
                                                        "(layers.fused.device_bn_fold)"}),
            "module_graph_eager": _net_line("c4", Bc, world, 2 * iters, el_d_eager, st4, 5000.0,
                                            "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                                            {"what": "utils.implicit_graphs(False): every forward dispatched from Python (rounds 1-5's module_graph)"}),
            "module_graph_hipgraph": _net_line("c4", Bc, world, 2 * iters, el_g, st4, 5000.0,
                                               "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                                               {"same_logits_as_module_graph": same_g}),
            "module_graph_auto_graphed": _net_line("c4", Bc, world, 2 * iters, el_a, st4, 5000.0,
                                                   "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                                                   {"same_logits_as_module_graph": same_a4, "replays": a4.replays, "capture_failures": dict(a4.capture_failures),
                                                    "what": "utils.auto_graphed(model): eager first call, captured on the second, "
                                                            "replayed after (input copied in, logits copied out)"}),
            "unfused": _net_line("c4", Bc, world, iters, el_u, st4, 5000.0, "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                                 fp32_activations=True),
            "fused": _net_line("c4", Bc, world, 2 * iters, el_f, st4, 5000.0, "int8 MFMA ~5 POP/s dense (guide); u-bench 4.54",
                               {"argmax_agreement_with_unfused": agree, "same_logits_as_module_by_module": same_fused}),
            **fused_graph,
            "note": "32 x 32 maps (SURVEY 8d): the fused form is 26 launches of 5-25 us inside the hipGraph, ~4.5 us of each is the fixed "
                    "cost of a launch boundary (profiles/r5_c4_direct_conv.md, tools/probes/c4_graph_seq.sh)"}
    # ---- C5: ternary VGG-16, 3 x 224 x 224 (2048 over 8 GPUs = 256 per GPU)
    if args.c5_batch > 0:
        Bv = args.c5_batch
        torch.manual_seed(5 + rank)
        m5 = bench_models.TernaryVGG16(num_classes=1000, image=224)
        bench_models.randomize_bn(m5, seed=5)
        m5 = m5.to(dev).to(memory_format=torch.channels_last).eval()
        m5.features[0].binary_input = False
        x5 = torch.randn((Bv, 3, 224, 224), device=dev).contiguous(memory_format=torch.channels_last)
        st5 = _layer_stats(m5, x5)
        from pytorch_quantize_impls_amd import lazy
        f5 = FusedFeatureClassifier(m5.features, m5.classifier, (512, 7, 7), fold="device")
        with torch.no_grad():
            yf5, yd5 = f5(x5), m5(x5)
            with lazy.eager():
                ye5 = m5(x5)
            agree5 = float((yf5.argmax(1) == ye5.argmax(1)).float().mean())
            same5 = bool(torch.equal(yf5, yd5))
            same5e = bool(torch.equal(yd5, ye5))
            del yf5, yd5, ye5

        def eager5():
            with lazy.eager():
                return m5(x5)
        el_u5 = timed(eager5, 3)
        el_d5 = timed(lambda: m5(x5), iters)
        per_rank_d5 = list(timed.per_rank_ms)
        el_f5 = timed(lambda: f5(x5), iters)
        out["c5_ternary_vgg16"] = {
            # the reference's module-by-module graph, un-modified; convs return deferred activations (lazy.py)
            "module_graph": _net_line("c5", Bv, world, iters, el_d5, st5, MFMA_FP4_PEAK_TFLOPS, "fp4 MFMA 10 PF dense",
                                      {"same_logits_as_fused_form": same5, "same_logits_as_module_by_module": same5e}),
            # the same graph with deferral off: every module writes its fp32 output
            "unfused": _net_line("c5", Bv, world, 3, el_u5, st5, MFMA_FP4_PEAK_TFLOPS, "fp4 MFMA 10 PF dense", fp32_activations=True),
            "fused": _net_line("c5", Bv, world, iters, el_f5, st5, MFMA_FP4_PEAK_TFLOPS, "fp4 MFMA 10 PF dense",
                               {"argmax_agreement_with_unfused": agree5}),
            "parity": "every conv / FC shape of the net exact against the device dense conv at full 224 x 224 geometry (batch 2 - 64) and the "
                      "last block against a batch-256 reference digest (tests/test_gpu_configs.py, test_gpu_r4.py); the whole net against the "
                      "CPU execution at 64 x 64 and at the full 224 x 224 geometry (sign ties counted, logits <= 1e-5 with the codes "
                      "forced); here: deferred == fused == module-by-module logits (torch.equal) at full size",
            "global_batch": Bv * world, "per_rank_ms_per_forward": per_rank_d5}
    # ---- training step: BinaryNet-AlexNet forward + backward at the headline batch, this backend vs the
    # reference's op sequence through ROCm PyTorch on the same GPU (tools/bench_train_step.py holds both forms)
    if args.train_batch and world == 1 and dist is None:
        import importlib.util
        spec = importlib.util.spec_from_file_location("bench_train_step", os.path.join(ROOT, "tools", "bench_train_step.py"))
        bts = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bts)
        torch.manual_seed(0)
        Bt = args.train_batch
        mt = bench_models.AlexNetBin().to(dev).to(memory_format=torch.channels_last).train()
        xt = torch.randn(Bt, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
        tt = torch.randint(0, 10, (Bt,), device=dev)
        before = dict(_fused_library_paths())
        from pytorch_quantize_impls_amd import lazy_train
        lazy_train.STATS.clear()
        t_ours, loss_ours = bts.step_time(mt, mt, xt, tt)
        chain_stats = {k: v for k, v in lazy_train.STATS.items() if k.startswith(("fused:", "replayed:"))}
        lib_used = {k: v - before.get(k, 0) for k, v in _fused_library_paths().items() if v != before.get(k, 0)}
        with lazy_train.eager():         # every module by itself: torch / MIOpen pooling, BatchNorm, Hardtanh between the layers
            t_mbm, loss_mbm = bts.step_time(mt, mt, xt, tt)
        # the same step with every [MaxPool, BatchNorm, Hardtanh, BinaryConnect] run on this backend's training-chain kernels
        # (layers.fuse_sequential_training: opt-in, shares the parameters) instead of torch / MIOpen
        mf = bench_models.TrainFusedAlexNetBin(mt)
        t_fused, loss_fused = bts.step_time(mf, mt, xt, tt)
        t_ref, loss_ref = bts.step_time(lambda t: bts.ref_forward(mt, t), mt, xt, tt, n=3)
        try:
            ties = bts.tie_report(mt, xt, tt)
        except Exception as exc:  # noqa: BLE001 — an extra must not void the headline measurement
            ties = {"error": f"{type(exc).__name__}: {exc}"}
        out["n2_training_step_alexnet_bin"] = {
            "workload": f"BinaryNet-AlexNet 3x224x224 batch {Bt}, training mode, forward + backward (nll loss), fp32 master weights, "
                        "channels_last; no optimizer step (the reference's trainers are out of scope)",
            "ms_per_step": t_ours, "images_per_s": Bt / t_ours * 1e3,
            "what": "the un-modified module graph: the [MaxPool, BatchNorm, Hardtanh, BinaryConnect] runs between the layers reach the "
                    "fused training nodes by themselves (lazy_train.py)",
            "recorded_chains_all_timed_steps": chain_stats,
            "module_by_module": {"ms_per_step": t_mbm, "images_per_s": Bt / t_mbm * 1e3, "loss": loss_mbm,
                                 "what": "with lazy_train.eager(): torch / MIOpen pooling, BatchNorm, Hardtanh kernels between the layers"},
            "with_fused_training_chain": {"ms_per_step": t_fused, "images_per_s": Bt / t_fused * 1e3, "loss": loss_fused,
                                          "what": "bench_models.TrainFusedAlexNetBin: pooling / BatchNorm(batch statistics) / Hardtanh / "
                                                  "sign forward + backward on csrc/train_chain.hip (opt-in fuse_sequential_training)"},
            "reference_ops_on_gpu": {"ms_per_step": t_ref, "images_per_s": Bt / t_ref * 1e3,
                                     "what": "torch.sign + F.conv2d / F.linear fp32 + the STE of functions/binary_connect.py:31-38 via autograd, "
                                             "same model, same GPU"},
            # real-valued pixels: conv1's fp32 rounding differs between the routes, a few signs flip behind the training-mode
            # BatchNorm, so the two losses agree to ~1e-3 only; on +-1 pixels the forward passes are identical (the parity test)
            "loss": loss_ours, "loss_reference_ops": loss_ref,
            # the gap between the two losses, explained: sign flips at the activation quantisers (tools/bench_train_step.tie_report)
            "first_step_ties": ties,
            "dense_library_calls_in_the_steps": lib_used,
            "gradient_parity": "tests/test_gpu_r3.py::test_alexnet_training_step_vs_fp64_of_the_reference_op_sequence and "
                               "::test_alexnet_training_step_with_the_fused_training_chain (<= 1e-5 normalised vs fp64 on the CPU)"}
        del mt, xt
        # the XNOR-Net flavour in training mode: per-tap scaled forward, grad_input on the flipped taps, grad_weight on the +-1
        # weight-gradient routes + the XNOR-Net combination (functions/xnor_connect.py:149-168); never takes the line down
        try:
            from pytorch_quantize_impls_amd.layers import XNORConv2d as _XC, LinearXNOR as _XL
            torch.manual_seed(0)
            mx = bench_models.alexnet_xnor()
            for mod in mx.modules():
                if isinstance(mod, (_XC, _XL)):
                    mod.weight.data.normal_(0, 0.05)
                    mod.bias.data.zero_()
            mx = mx.to(dev).to(memory_format=torch.channels_last).train()
            xt = torch.randn(Bt, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
            before = dict(_fused_library_paths())
            t_x, loss_x = bts.step_time(mx, mx, xt, tt)
            lib_x = {k: v - before.get(k, 0) for k, v in _fused_library_paths().items() if v != before.get(k, 0)}
            out["n2_training_step_alexnet_xnor"] = {
                "workload": f"XNOR-Net AlexNet (xnor_net_convert of the config-3 topology) 3x224x224 batch {Bt}, training mode, forward + "
                            "backward (nll loss), channels_last, un-modified module graph",
                "ms_per_step": t_x, "images_per_s": Bt / t_x * 1e3, "loss": loss_x,
                "vs_binarynet_flavour_step": t_x / t_ours,
                "dense_library_calls_in_the_steps": lib_x,
                "gradient_parity": "tests/test_gpu_r4.py::test_xnor_conv_function_vs_reference_fp64 / test_xnor_dense_function_vs_reference_fp64 "
                                   "(<= 1e-5 vs the fp64 evaluation of the reference functions)"}
            del mx, xt
        except Exception as exc:
            out["n2_training_step_alexnet_xnor"] = {"error": f"{type(exc).__name__}: {exc}"}
        # C4's network in training mode (models/Resnet/Resnet_bin.py:63-97 shapes: 3 x 32 x 32): the module graph (DorefaConv2d
        # forward / backward on this backend, BatchNorm / relu / add are torch's and MIOpen's) and the form with every
        # BatchNorm [+ shortcut] -> ReLU -> quantiser run as one FusedTrainBnActQuant node (csrc/train_chain.hip)
        try:
            torch.manual_seed(0)
            mr = bench_models.DorefaResNet18(w_bits=1, a_bits=4).to(dev).to(memory_format=torch.channels_last).train()
            xr = torch.randn(Bt, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
            before = dict(_fused_library_paths())
            lsm = lambda net: (lambda t: torch.nn.functional.log_softmax(net(t), 1))      # noqa: E731
            t_r, loss_r = bts.step_time(lsm(mr), mr, xr, tt, n=10)
            with lazy_train.eager():
                t_rm, loss_rm = bts.step_time(lsm(mr), mr, xr, tt, n=10)
            t_rf, loss_rf = bts.step_time(lsm(bench_models.TrainFusedDorefaResNet18(mr)), mr, xr, tt, n=10)
            lib_r = {k: v - before.get(k, 0) for k, v in _fused_library_paths().items() if v != before.get(k, 0)}
            # serving-style: range verdicts remembered (no host sync per layer; a broken assumption gives NaN, never a wrong
            # number) — eager, and the whole forward + backward captured once as a hipGraph and replayed
            from pytorch_quantize_impls_amd.functions import _fused as _ff
            remembered = {}
            try:
                with _ff.detect_scope("remember"):        # thread-local; the Functions carry it into their backward
                    fused_r = bench_models.TrainFusedDorefaResNet18(mr)
                    t_m, _ = bts.step_time(lsm(mr), mr, xr, tt, n=10)
                    t_f, _ = bts.step_time(lsm(fused_r), mr, xr, tt, n=10)
                remembered = {"module_graph_ms_per_step": t_m, "fused_chain_ms_per_step": t_f}
                from pytorch_quantize_impls_amd import utils as _utils
                gstep = _utils.GraphedTrainStep(fused_r, lambda o_, t_: torch.nn.functional.nll_loss(torch.nn.functional.log_softmax(o_, 1), t_),
                                                xr, tt)
                for _ in range(2):
                    loss_g = gstep(xr, tt)
                torch.cuda.synchronize()
                t0g = time.perf_counter()
                for _ in range(10):
                    loss_g = gstep(xr, tt)
                torch.cuda.synchronize()
                remembered["fused_chain_as_hipgraph_ms_per_step"] = (time.perf_counter() - t0g) / 10 * 1e3
                remembered["hipgraph_loss"] = float(loss_g.detach())
                del gstep
            except Exception as exc:
                remembered["error"] = f"{type(exc).__name__}: {exc}"
            out["n2_training_step_dorefa_resnet18_w1a4"] = {
                "workload": f"DoReFa ResNet-18 W1A4 3x32x32 batch {Bt}, training mode, forward + backward (nll loss), channels_last; "
                            "fp32 stem conv and classifier are torch's, as in the reference",
                "ms_per_step": t_r, "images_per_s": Bt / t_r * 1e3, "loss": loss_r,
                "what": "the un-modified module graph: BatchNorm [+ shortcut] [-> ReLU] -> nnDorefaQuant behind every DorefaConv2d reaches the "
                        "fused training node by itself (lazy_train.py); the fp32 stem's BatchNorm stays MIOpen's",
                "module_by_module": {"ms_per_step": t_rm, "images_per_s": Bt / t_rm * 1e3, "loss": loss_rm,
                                     "what": "with lazy_train.eager(): MIOpen BatchNorm, torch add / relu, separate quantiser pass"},
                "with_fused_training_chain": {"ms_per_step": t_rf, "images_per_s": Bt / t_rf * 1e3, "loss": loss_rf,
                                              "what": "bench_models.TrainFusedDorefaResNet18: BatchNorm(batch statistics) + shortcut add + "
                                                      "ReLU + k-bit quantiser forward + backward as one node per conv "
                                                      "(layers.FusedTrainBnActQuant, opt-in)"},
                "with_remembered_range_verdicts": dict(remembered, what="_fused.detect_scope('remember'): no host sync per layer for "
                                                       "'do these codes fit int8?'; hipGraph = utils.GraphedTrainStep (forward + loss + backward captured once; every replay copies the batch in)"),
                "dense_library_calls_in_the_steps": lib_r,
                "note": "many small launches (3 x 32 x 32 maps): ~1100 kernels per step in the module graph; "
                        "tools/probes/train_resnet_prof.py has the per-kernel split",
                "gradient_parity": "tests/test_gpu_r3.py::test_dorefa_kbit_conv_training_vs_fp64, "
                                   "::test_dorefa_training_chain_vs_fp64_of_the_module_chain (<= 1e-5 normalised vs fp64), "
                                   "::test_dorefa_resnet18_training_step_with_the_fused_training_chain"}
            del mr, xr
        except Exception as exc:        # never take the line down
            out["n2_training_step_dorefa_resnet18_w1a4"] = {"error": f"{type(exc).__name__}: {exc}"}
    elif args.train_batch and dist is not None:
        # data-parallel step, one process per GPU: per-GPU batch fixed (weak scaling), gradients averaged by the bucketed
        # all-reduce of utils/data_parallel.py (RCCL over xGMI) issued after backward (overlap=False, see below).  BatchNorm
        # runs on PER-SHARD batch statistics (plain nn.BatchNorm2d, no SyncBatchNorm: SURVEY 8e "or per-shard stats"), so the
        # step is the data-parallel step of the reference's modules, not the single-GPU step at the global batch.
        # Never allowed to take the line down.
        try:
            import importlib.util
            from pytorch_quantize_impls_amd.utils import GradientSynchronizer, broadcast_parameters
            spec = importlib.util.spec_from_file_location("bench_train_step", os.path.join(ROOT, "tools", "bench_train_step.py"))
            bts = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(bts)
            torch.manual_seed(0)
            Bt = args.train_batch
            mt = bench_models.AlexNetBin().to(dev).to(memory_format=torch.channels_last).train()
            broadcast_parameters(mt)
            # collectives issued from this thread after backward (overlap=False): one less moving part in a run nobody can watch
            sync = GradientSynchronizer(mt.parameters(), overlap=False)
            xt = torch.randn(Bt, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
            tt = torch.randint(0, 10, (Bt,), device=dev)

            def dp_step():
                mt.zero_grad(set_to_none=True)
                loss = torch.nn.functional.nll_loss(mt(xt), tt)
                loss.backward()
                sync.wait()
                return loss
            for _ in range(2):
                dp_step()
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(5):
                dp_step()
            torch.cuda.synchronize()
            e = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
            dist.all_reduce(e, op=dist.ReduceOp.MAX)
            t_dp = float(e.item()) / 5 * 1e3
            grad_bytes = sum(p.numel() * 4 for p in mt.parameters() if p.requires_grad)
            out["n2_training_step_alexnet_bin"] = {
                "workload": f"BinaryNet-AlexNet training step, data parallel over {world} GPUs, batch {Bt} per GPU, forward + backward + "
                            f"bucketed gradient all-reduce after backward (utils/data_parallel.GradientSynchronizer(overlap=False), backend {args.dist_backend}), no optimizer step",
                "ms_per_step": t_dp, "images_per_s": Bt * world / t_dp * 1e3, "global_batch": Bt * world,
                "gradient_bytes_per_step": grad_bytes, "buckets": len(sync.buckets),
                "batchnorm": "per-shard batch statistics (no cross-rank reduction of the statistics)"}
            sync.remove()
            del mt, xt
        except Exception as exc:  # noqa: BLE001 — an extra must not void the headline measurement
            out["n2_training_step_alexnet_bin"] = {"error": f"{type(exc).__name__}: {exc}"}
    return out


def _fused_library_paths():
    from pytorch_quantize_impls_amd.functions import _fused
    return _fused.LIBRARY_PATHS


def pmc_traffic(gemm_impl):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of
    this same command (profiles/pmc_latest.json; counters cannot be collected from inside the
    process).  FETCH_SIZE is doubled (gfx950 half-count of wide coalesced reads, MI355X_MICROARCH.md
    HBM section); WRITE_SIZE as reported."""
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        with open(path) as fh:
            d = json.load(fh)
        k = d["kernels"]["mfma_gemm_kernel" if gemm_impl == "mfma" else "popc_gemm_kernel"]
        return (2.0 * k["FETCH_SIZE_KiB"] + k["WRITE_SIZE_KiB"]) * 1024.0, k.get("source", d.get("source", path)), k.get("rocprof_avg_us")
    except (OSError, KeyError, ValueError):
        return None, None, None


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip() + f" ({os.cpu_count()} logical)"
    except OSError:
        pass
    return f"unknown ({os.cpu_count()} logical)"


if __name__ == "__main__":
    main()
