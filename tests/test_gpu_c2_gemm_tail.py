"""The row-wide store tail of the 256x256 ping-pong GEMM (csrc/mfma_gemm_kernel.h, GemmCfg::ROW_STORES) against exact sums.

Whole tiles with a 16-byte aligned result leave through a 32 x 64 transpose patch per wave as 256-byte row stores; ragged tiles and
misaligned results keep the guarded epilogues.  The operands are +-1, so the int64 product on the CPU is the only right answer and
every comparison is exact.  Shapes: one tile at one ring-full of K (four 64-byte stages), one stage more, and a longer K; 2 x 2
tiles (tile offsets); a ragged shape (guarded path, partial tiles beside whole ones); a result view with ldy > N; a misaligned ldy.
One 4096 x 2048 result reaches the size at which the stores take their write-through form (the form the C2 step runs).
Every result is a view into a buffer of sentinels: nothing outside [0, M) x [0, N) may change.  All cases name the tile through
qt_nib_gemm_variant's number 20 (the automatic rule sends shapes this small to the skinny tiles) and ask qt_gemm_tile_describe what
that number launches; the profiler confirms the kernel instance for one fp4 case and for the fp16 case.

The fp16 two-term linear runs the same configuration on real-valued operands: its result must equal, bit for bit, the one the
kernel gave before the store tail changed (tests/golden/c2_tail_f16x2_256x256x512.npy) — the summation order over K is unchanged."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _routes as R

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, ops, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2_tail_f16x2_256x256x512.npy")
PP256 = 20                      # qt_nib_gemm_variant / qt_f16_gemm_variant
SENTINEL = -12345.5

#        name                  M    N    K     extra columns of the result buffer (ldy = N + extra)
CASES = [("one ring",          256, 256, 512,  0),
         ("ring + 1 stage",    256, 256, 576,  0),
         ("K 1024",            256, 256, 1024, 0),
         ("2x2 tiles",         512, 512, 1024, 0),
         ("ragged",            300, 260, 640,  0),
         ("ldy > N",           256, 256, 512,  64),
         ("ldy misaligned",    256, 256, 512,  3)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _tile(M, N, ld):
    buf = ctypes.create_string_buffer(64)
    rc = _lib.load().qt_gemm_tile_describe(_lib.DEFINES["QT_GEMM_FAMILY_DENSE"], PP256, M, N, ld, ld, buf, 64)
    assert rc == 0, rc
    return buf.value.decode()


def _mfma_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return R.mfma_routes([e.key for e in prof.key_averages() if "mfma_gemm_kernel" in e.key])


def _fp4(dev, M, N, K, extra, seed, bias=False):
    """(result view, whole buffer, exact int64 sums) of one +-1 GEMM on the 256x256 ping-pong tile."""
    x, w = synth.pm1(seed, (M, K)), synth.pm1(seed + 1, (N, K))
    b = synth.uniform(seed + 2, (N,), -4.0, 4.0).round().astype(np.float32) if bias else None
    want = x.astype(np.int64) @ w.astype(np.int64).T + (b.astype(np.int64) if bias else 0)
    xn, wn = ops.sign_pack_nib(torch.from_numpy(x).to(dev)), ops.sign_pack_nib(torch.from_numpy(w).to(dev))
    assert _tile(M, N, xn.ld) == "PP256" and xn.ld == wn.ld
    buf = torch.full((M + 2, N + extra), SENTINEL, dtype=torch.float32, device=dev)
    y = buf[:M, :N]
    ops.nib_gemm(xn, wn, bias=None if b is None else torch.from_numpy(b).to(dev), out=y, variant=PP256)
    return y, buf, want


@pytest.mark.parametrize("name,M,N,K,extra", CASES, ids=[c[0] for c in CASES])
def test_exact_sums(dev, name, M, N, K, extra):
    y, buf, want = _fp4(dev, M, N, K, extra, seed=100 + K + extra, bias=(name == "2x2 tiles"))
    got = y.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), name
    outside = buf.clone()
    outside[:M, :N] = SENTINEL
    assert bool((outside == SENTINEL).all()), (name, "wrote outside the result")


def test_streamed_result(dev):
    """A result of 8 Mi elements (4096 x 2048: the smallest M x N at which the epilogue streams its result out): the write-through
    form of the row-wide stores, the one the C2 step runs, on 16 x 8 tiles with a bias.  K = 512 keeps every sum below 2^10, so the
    fp64 product (BLAS) is exact and is converted to the same int64 sums as above."""
    M, N, K = 4096, 2048, 512
    assert M * N == 8 << 20
    x, w = synth.pm1(300, (M, K)), synth.pm1(301, (N, K))
    b = synth.uniform(302, (N,), -4.0, 4.0).round().astype(np.float32)
    want = (x.astype(np.float64) @ w.astype(np.float64).T).astype(np.int64) + b.astype(np.int64)
    xn, wn = ops.sign_pack_nib(torch.from_numpy(x).to(dev)), ops.sign_pack_nib(torch.from_numpy(w).to(dev))
    assert _tile(M, N, xn.ld) == "PP256"
    buf = torch.full((M + 1, N + 4), SENTINEL, dtype=torch.float32, device=dev)
    ops.nib_gemm(xn, wn, bias=torch.from_numpy(b).to(dev), out=buf[:M, :N], variant=PP256)
    assert np.array_equal(buf[:M, :N].cpu().numpy(), want.astype(np.float32))
    assert bool((buf[M:] == SENTINEL).all()) and bool((buf[:, N:] == SENTINEL).all())


def test_kernel_instance(dev):
    x = ops.sign_pack_nib(torch.from_numpy(synth.pm1(7, (256, 512))).to(dev))
    assert _mfma_kernels(lambda: ops.nib_gemm(x, x, variant=PP256)) == {"PP256<ElemFp4>"}


def f16_two_term(dev, profile=False):
    """The fp16 two-term linear at 256 x 256 x 512 on the 256x256 ping-pong tile: real activations, binary weights."""
    x = torch.from_numpy(synth.normal(21, (256, 512)) * 3.0).to(dev)
    w = torch.from_numpy(synth.uniform(22, (256, 512), -1.5, 1.5)).to(dev)
    b = torch.from_numpy(synth.normal(23, (256,))).to(dev)
    xp, wp = ops.split_bf16x3(x, terms=2), ops.weight_bf16x3(w, "binary", terms=2)
    if profile:
        assert _mfma_kernels(lambda: ops.bf16_gemm(xp, wp, b, variant=PP256)) == {"PP256<ElemF16>"}
    return ops.bf16_gemm(xp, wp, b, variant=PP256).cpu().numpy()


def test_f16_two_term_bits_unchanged(dev):
    want = np.load(GOLDEN)
    got = f16_two_term(dev, profile=True)
    assert got.shape == want.shape == (256, 256) and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        ("elements that differ", int((got.view(np.uint32) != want.view(np.uint32)).sum()), float(np.abs(got - want).max()))
    # ... and the values are the linear's: well inside the two-term split's 1e-5 of the fp64 product
    x, w = synth.normal(21, (256, 512)).astype(np.float32) * np.float32(3.0), synth.uniform(22, (256, 512), -1.5, 1.5)
    ref = x.astype(np.float64) @ np.where(w >= 0, 1.0, -1.0).T + synth.normal(23, (256,)).astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_variant_entry_refuses_other_tiles(dev):
    x = torch.from_numpy(synth.normal(31, (8, 64))).to(dev)
    xp, wp = ops.split_bf16x3(x, terms=2), ops.weight_bf16x3(x, "binary", terms=2)
    with pytest.raises(_lib.QtStatusError):
        ops.bf16_gemm(xp, wp, variant=21)
