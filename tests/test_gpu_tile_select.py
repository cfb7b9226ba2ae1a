"""The fp4 GEMM runs the tile its describe entry point names: one case per rung of the automatic rule (csrc/tile_select.h
select_gemm), each under the profiler and against the exact integer product."""
import re

import pytest
import torch

import _routes as R

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import ops  # noqa: E402

# (M, N, K, row stride in words or None = the packers' default, the rung the shape was chosen for)
CASES = [
    (256, 256, 1024, None, "64x64, 512-byte stages, pipe=1"),          # M <= 256, strides of whole 512-byte stages
    (512, 256, 512, None, "128x64, 256-byte stages, pipe=1"),          # M <= 512, strides of whole 256-byte stages
    (1024, 64, 256, None, "256x64, pipe=1"),
    (8192, 1280, 256, None, "256x256, pipe=2 (ping-pong)"),
    (8192, 1152, 256, None, "256x192, pipe=2 (ping-pong)"),
    (24576, 1152, 256, None, "384x192, pipe=2 (ping-pong)"),
    (40960, 128, 256, None, "256x128, pipe=2 (ping-pong)"),
    (1024, 256, 200, 28, "256x64, pipe=0"),                            # ragged K, stride not a multiple of 32 words: the generic kernel
]


def _text(t):
    """GemmCfg tuple (WM, WN, TMW, TNW, PIPE, ABL, SB, CONV, OCC) -> the tile text of qt_nib_gemm_describe."""
    wm, wn, tmw, tnw, pipe, _, sb = t[:7]
    stages = f"{sb}-byte stages, " if sb != (64 if pipe == 2 else 128) else ""
    return f"{32 * wm * tmw}x{32 * wn * tnw}, {stages}pipe={pipe}{' (ping-pong)' if pipe == 2 else ''}"


@pytest.mark.parametrize("M,N,K,ld,rung", CASES, ids=[c[4].split(",")[0] + f"/pipe{c[4].split('pipe=')[1][0]}" for c in CASES])
def test_nib_gemm_runs_the_described_tile(M, N, K, ld, rung):
    from torch.profiler import ProfilerActivity, profile
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(M + N + K)
    x = (torch.randint(0, 2, (M, K), generator=g, device=dev) * 2 - 1).float()
    w = (torch.randint(0, 2, (N, K), generator=g, device=dev) * 2 - 1).float()
    xp, wp = ops.sign_pack_nib(x, ld=ld), ops.sign_pack_nib(w, ld=ld)
    described = ops.nib_gemm_kernel_name(M, N, K, ld=xp.ld)
    assert xp.ld == wp.ld and described == f"mfma_gemm_kernel<ElemFp4, {rung}>", (xp.ld, described)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        y = ops.nib_gemm(xp, wp)
        torch.cuda.synchronize()
    ran = [m for m in (re.search(r"GemmCfg<ElemFp4, ([\d, ]+)>", e.key.replace("(anonymous namespace)::", "")) for e in prof.key_averages()) if m]
    assert len(ran) == 1, [e.key for e in prof.key_averages()]
    t = tuple(int(v) for v in ran[0].group(1).split(","))
    assert f"mfma_gemm_kernel<ElemFp4, {_text(t)}>" == described, (R.GEMM_CFG.get(t, t), described)
    want = x.double() @ w.double().t()                      # +-1 sums of K <= 1024 terms: exact integers
    assert y.dtype == torch.float32 and torch.equal(y.double(), want)
