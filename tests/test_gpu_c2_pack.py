"""fp32 -> fp4 nibble-plane packs (qt_sign_pack_nib_f32, qt_ternary_pack_nib_f32, qt_pack_pair_nib_f32) against a
host restatement of the format: safeSign -> 0x2 / 0xA, TernaryConnectDeterministic -> 0x2 / 0xA / 0x0, element k of a
row in nibble k % 8 of word k // 8, every word past K zero.  The shapes cover partial 256-slot units (row strides that
are not a multiple of 128 words), padded strides, strided rows, K tails (scalar kernel) and operand pairs of very
different row counts (the pair kernel splits its workgroups between the two)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_quantize_impls_amd import ops, synth  # noqa: E402
from pytorch_quantize_impls_amd.layers import LinearBin, LinearTer  # noqa: E402
from oracle import oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _nib_ref(x, ld, ternary=False):
    x = np.asarray(x, dtype=np.float32)
    rows, K = x.shape
    s = np.where(x < 0, np.float32(-1), np.float32(1)).astype(np.float32)
    if ternary:
        t = np.where((x - np.float32(0.5) * s).astype(np.float32) < 0, np.float32(-1), np.float32(1))
        q = (s + t) * np.float32(0.5)
    else:
        q = s
    nib = np.where(q == 0, 0x0, np.where(q < 0, 0xA, 0x2)).astype(np.uint32)
    full = np.zeros((rows, ld * 8), dtype=np.uint32)
    full[:, :K] = nib
    full = full.reshape(rows, ld, 8)
    return np.bitwise_or.reduce(full << (4 * np.arange(8, dtype=np.uint32)), axis=2)


def _words(p):
    return p.words.cpu().numpy().view(np.uint32)


def _special(x):
    """sprinkle values the encoders must treat exactly: +-0, +-0.5 (ternary threshold), NaN, +-inf"""
    x = x.copy()
    flat = x.reshape(-1)
    vals = np.array([0.0, -0.0, 0.5, -0.5, np.nan, np.inf, -np.inf, 1e-40, -1e-40], dtype=np.float32)
    idx = np.arange(0, flat.size, 7)[: 4 * len(vals)]
    flat[idx] = np.resize(vals, idx.size)
    return x


SHAPES = [(255, 300), (257, 1000), (300, 4096), (1, 4), (7, 2052), (64, 2048), (3, 12), (5, 31), (9, 1001)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K", SHAPES)
def test_single_operand_packs_equal_the_format(dev, rows, K):
    x = _special(synth.normal(rows * 7 + K, (rows, K)) * 0.8)
    xt = torch.from_numpy(x).to(dev)
    for ld in (None, O.packed_ld_nib(K) + 36):      # default stride (multiple of 32 words) and one past a 256-slot unit
        p = ops.sign_pack_nib(xt, ld)
        assert np.array_equal(_words(p), _nib_ref(x, p.words.shape[1])), (rows, K, ld)
        p = ops.ternary_pack_nib(xt, ld)
        assert np.array_equal(_words(p), _nib_ref(x, p.words.shape[1], ternary=True)), (rows, K, ld)


@pytest.mark.gpu
def test_pack_of_strided_rows(dev):
    x = _special(synth.normal(41, (300, 1500)))
    xt = torch.from_numpy(x).to(dev)[:, 100:1100]     # row stride 1500 floats, 16-byte aligned start
    p = ops.sign_pack_nib(xt)
    assert np.array_equal(_words(p), _nib_ref(x[:, 100:1100], p.words.shape[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(4096, 4096, 4096), (1, 4096, 1024), (4096, 1, 1024), (255, 257, 300),
                                   (257, 255, 1000), (2, 3, 4), (300, 77, 2048)])
def test_pair_pack_equals_the_format(dev, M, N, K):
    x = _special(synth.normal(M + 3 * K, (M, K)))
    w = _special(synth.uniform(N + 5 * K, (N, K), -1.5, 1.5))
    xt, wt = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    for kind in ("binary", "ternary"):
        xp, wp = ops.pack_linear_operands(xt, wt, kind, "mfma")
        assert np.array_equal(_words(xp), _nib_ref(x, xp.words.shape[1])), (M, N, K, kind)
        assert np.array_equal(_words(wp), _nib_ref(w, wp.words.shape[1], ternary=kind == "ternary")), (M, N, K, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(255, 257, 300), (257, 255, 1000), (300, 300, 4100)])
def test_layers_through_the_pair_pack_equal_the_oracle(dev, M, N, K):
    x = np.where(synth.normal(M * 3 + K, (M, K)) < 0, -1.0, 1.0).astype(np.float32)
    w = synth.uniform(N * 5 + K, (N, K), -1.5, 1.5)
    b = synth.normal(N + 1, (N,))
    for cls, ref in ((LinearBin, O.linear_bin_forward), (LinearTer, O.linear_ter_forward)):
        layer = cls(K, N, bias=True).to(dev).train()
        layer.weight.data.copy_(torch.from_numpy(w))
        layer.bias.data.copy_(torch.from_numpy(b))
        y = layer(torch.from_numpy(x).to(dev)).detach().cpu().numpy()
        want = ref(x, w) + b[None, :].astype(np.float32)
        assert np.array_equal(y, want.astype(np.float32)), (cls.__name__, M, N, K)
