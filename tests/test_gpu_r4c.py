"""Round-4 GPU parity, part c: DoReFa layers beyond the int8 code range (VERDICT r3 "missing" item 5).

  * bit_width = 8: the weight levels c = 255 w_q are odd integers up to 255 — not int8, but exact in fp16 and bf16 — so the layer
    runs on the split-activation x exact-level-image routes, forward and both gradients, training and eval mode
    (layers/dorefa_layers.py:41-45,77-82; functions/dorefa_connect.py:99-111);
  * eval-mode k-bit layers on an activation WITHOUT usable int8 codes (a real-valued input, codes beyond +-127): the same routes
    instead of the dense library;
  * bit_width = 32: the identity quantiser (functions/dorefa_connect.py:19-20,100-101) — two real operands on the six-term planes.
Every case against the fp64 evaluation of the reference expression F.linear / F.conv2d(x, weight_op(W), b), <= 1e-5 normalised
(SURVEY 8d), with _fused.LIBRARY_PATHS watched."""
import copy

import pytest
import torch

from conftest import norm_err

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib  # noqa: E402
from pytorch_quantize_impls_amd.functions import _fused, nnDorefaQuant  # noqa: E402
from pytorch_quantize_impls_amd.layers import DorefaConv2d, LinearDorefa  # noqa: E402

TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture()
def all_shapes_on_the_routes():
    old = _fused.BWD_MFMA_MIN_MACS
    _fused.BWD_MFMA_MIN_MACS = 0
    yield
    _fused.BWD_MFMA_MIN_MACS = old


def n(t):
    return t.detach().cpu().numpy()


def _lib_delta(before):
    return {k: v - before.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != before.get(k, 0)}


def _fp64_layer(layer, x, gout=None):
    """The reference expression in fp64 on the CPU: training mode quantises the weight, eval mode uses the stored image.
    The quantised VALUES are the device layer's own fp32 image (the elementwise quantiser is pinned bit for bit elsewhere; with
    255 levels an fp64 evaluation of tanh / max|tanh| rounds a handful of the 36 864 weights of a 3 x 3 layer to the neighbouring
    level, 2 / 255 away — a difference of the reference's precision, not of this backend); the gradient still flows through the
    fp64 quantiser graph (straight-through: it does not depend on the rounding)."""
    ref = copy.deepcopy(layer).cpu().double()
    xr = x.detach().cpu().double().requires_grad_(gout is not None)
    if layer.training:
        w = ref.weight_op.forward(ref.weight)
        with torch.no_grad():
            wq_dev = layer.weight_op.forward(layer.weight).detach().cpu().double()
        w = w + (wq_dev - w).detach()
    else:
        w = ref.weight
    if isinstance(ref, torch.nn.Conv2d):
        y = torch.nn.functional.conv2d(xr, w, ref.bias, ref.stride, ref.padding, ref.dilation, ref.groups)
    else:
        y = torch.nn.functional.linear(xr, w, ref.bias)
    if gout is None:
        return y.detach()
    y.backward(gout.detach().cpu().double())
    return y.detach(), xr.grad, ref.weight.grad, (ref.bias.grad if ref.bias is not None else None)


# ---- bit_width = 8 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coded", [True, False])
@pytest.mark.parametrize("Cin,Cout,ksz,s,p,H", [(64, 64, 3, 1, 1, 16), (64, 128, 3, 2, 1, 16), (64, 128, 1, 2, 0, 16)])
def test_dorefa_8bit_conv_training_vs_fp64(dev, all_shapes_on_the_routes, coded, Cin, Cout, ksz, s, p, H):
    torch.manual_seed(80 + Cin + ksz + s)
    conv = DorefaConv2d(Cin, Cout, ksz, stride=s, padding=p, bias=True, bit_width=8).to(dev).train()
    conv.weight.data.normal_(0, 0.7)
    raw = (torch.rand(6, Cin, H, H, device=dev) * 1.4).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x = nnDorefaQuant(4)(raw) if coded else raw * 1.0
    x.retain_grad()
    lib_before = dict(_fused.LIBRARY_PATHS)
    before = dict(_lib.call_counts)
    y = conv(x)
    gout = torch.randn_like(y)
    y.backward(gout)
    lib_now = _lib_delta(lib_before)
    if coded:
        assert not lib_now, lib_now
    else:
        assert set(lib_now) <= {"conv grad_weight outside the matrix-core route"}, lib_now
    assert _lib.call_counts["qt_conv2d_implicit"] - before.get("qt_conv2d_implicit", 0) >= 2     # forward + grad_x
    # the levels really leave int8: the route under test is not the int8 one
    lv = torch.round(conv.weight_op.forward(conv.weight).detach() * 255.0)
    assert float(lv.abs().max()) == 255.0 and bool((torch.remainder(lv, 2) == 1).all())
    ry, rgx, rgw, rgb = _fp64_layer(conv, x, gout)
    assert norm_err(n(y), n(ry)) <= TOL
    assert norm_err(n(x.grad), n(rgx)) <= TOL
    assert norm_err(n(conv.weight.grad), n(rgw)) <= 2 * TOL        # through tanh / max|tanh| of the weight quantiser in fp32
    assert norm_err(n(conv.bias.grad), n(rgb)) <= TOL


@pytest.mark.parametrize("coded", [True, False])
def test_dorefa_8bit_linear_training_vs_fp64(dev, all_shapes_on_the_routes, coded):
    torch.manual_seed(88)
    lin = LinearDorefa(300, 70, bias=True, bit_width=8).to(dev).train()
    lin.weight.data.normal_(0, 0.7)
    raw = (torch.rand(96, 300, device=dev) * 1.3).requires_grad_(True)
    x = nnDorefaQuant(3)(raw) if coded else raw * 1.0
    x.retain_grad()
    lib_before = dict(_fused.LIBRARY_PATHS)
    y = lin(x)
    gout = torch.randn_like(y)
    y.backward(gout)
    lib_now = _lib_delta(lib_before)
    assert not lib_now, lib_now
    ry, rgx, rgw, rgb = _fp64_layer(lin, x, gout)
    assert norm_err(n(y), n(ry)) <= TOL
    assert norm_err(n(x.grad), n(rgx)) <= TOL
    assert norm_err(n(lin.weight.grad), n(rgw)) <= 2 * TOL
    assert norm_err(n(lin.bias.grad), n(rgb)) <= TOL


@pytest.mark.parametrize("k_w", [3, 8])
@pytest.mark.parametrize("act", ["real", "codes", "beyond_int8"])
def test_dorefa_kbit_eval_layers_without_int8_codes_vs_fp64(dev, k_w, act):
    """Eval mode (weight holds the quantised image): k <= 7 on a coded activation keeps the int8 route; a real-valued activation,
    codes beyond +-127 and 8-bit weights take the level routes — none of them the dense library."""
    torch.manual_seed(k_w)
    conv = DorefaConv2d(64, 96, 3, stride=1, padding=1, bias=True, bit_width=k_w).to(dev)
    lin = LinearDorefa(320, 72, bias=True, bit_width=k_w).to(dev)
    conv.weight.data.normal_(0, 0.7)
    lin.weight.data.normal_(0, 0.7)
    conv.eval()
    lin.eval()
    scale = {"real": 1.3, "codes": 1.3, "beyond_int8": 40.0}[act]
    xc = (torch.rand(4, 64, 12, 12, device=dev) * scale).contiguous(memory_format=torch.channels_last)
    xl = torch.rand(64, 320, device=dev) * scale
    if act != "real":
        xc, xl = nnDorefaQuant(4)(xc), nnDorefaQuant(4)(xl)
    lib_before = dict(_fused.LIBRARY_PATHS)
    before = dict(_lib.call_counts)
    with torch.no_grad():
        yc, yl = conv(xc), lin(xl)
        yc2, yl2 = conv(xc), lin(xl)                     # second call: cached level planes
    assert not _lib_delta(lib_before), _lib_delta(lib_before)
    if k_w <= 7 and act == "codes":                  # the int8 route: no split of the activation
        assert all(_lib.call_counts.get(k, 0) == before.get(k, 0) for k in ("qt_f16x2_pack_f32", "qt_bf16x3_pack_f32"))
    else:
        assert any(_lib.call_counts.get(k, 0) > before.get(k, 0) for k in ("qt_f16x2_pack_f32", "qt_bf16x3_pack_f32"))
    assert torch.equal(yc, yc2) and torch.equal(yl, yl2)
    assert norm_err(n(yc), n(_fp64_layer(conv, xc))) <= TOL
    assert norm_err(n(yl), n(_fp64_layer(lin, xl))) <= TOL


# ---- bit_width = 32: the identity quantiser --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False])
def test_dorefa_32bit_layers_vs_fp64(dev, training):
    torch.manual_seed(32)
    conv = DorefaConv2d(32, 48, 3, stride=1, padding=1, bias=True, bit_width=32).to(dev).train(training)
    lin = LinearDorefa(200, 40, bias=True, bit_width=32).to(dev).train(training)
    xc = torch.randn(4, 32, 10, 10, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xl = torch.randn(48, 200, device=dev).requires_grad_(True)
    lib_before = dict(_fused.LIBRARY_PATHS)
    yc, yl = conv(xc), lin(xl)
    gc, gl = torch.randn_like(yc), torch.randn_like(yl)
    yc.backward(gc)
    yl.backward(gl)
    lib_now = _lib_delta(lib_before)
    # the one contraction of two real operands without an own route: the conv's weight gradient (counted, not hidden)
    assert set(lib_now) <= {"conv grad_weight outside the matrix-core route"}, lib_now
    for layer, x, y, g in ((conv, xc, yc, gc), (lin, xl, yl, gl)):
        ry, rgx, rgw, rgb = _fp64_layer(layer.train(), x, g)
        layer.train(training)
        assert norm_err(n(y), n(ry)) <= TOL
        assert norm_err(n(x.grad), n(rgx)) <= TOL
        assert norm_err(n(layer.weight.grad), n(rgw)) <= TOL
        assert norm_err(n(layer.bias.grad), n(rgb)) <= TOL


# ---- LinearXNOR on packed +-1 activations: the digit-plane int8 form ------------------------------------------------------------------

import numpy as np  # noqa: E402
from pytorch_quantize_impls_amd import ops, packed  # noqa: E402
from pytorch_quantize_impls_amd.functions import BinaryConnectDeterministic  # noqa: E402
from pytorch_quantize_impls_amd.layers import LinearXNOR  # noqa: E402


@pytest.mark.parametrize("M,N,K", [(768, 4096, 9216), (768, 10, 4096), (15, 7, 100), (300, 1000, 1024), (256, 192, 64)])
def test_i8_gemm_splitk_partial_sums_are_exact(dev, M, N, K):
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    ld = ops.code_ld_bytes(K)
    x = torch.zeros((M, ld), dtype=torch.int8, device=dev)
    w = torch.zeros((N, ld), dtype=torch.int8, device=dev)
    x[:, :K] = torch.randint(-127, 128, (M, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
    w[:, :K] = torch.randint(-1, 2, (N, K), device=dev, generator=g, dtype=torch.int32).to(torch.int8)
    kslice, nslice = ops.splitk_plan(M, N, ld)
    assert kslice * nslice == ld and kslice % 64 == 0
    ldp = (N + 3) // 4 * 4
    part = torch.full((nslice, M, ldp), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("qt_i8_gemm_splitk", x.data_ptr(), ld // 4, w.data_ptr(), ld // 4, part.data_ptr(), ldp, M, N, kslice, nslice, M * ldp,
              torch.cuda.current_stream().cuda_stream)
    got = part[:, :, :N].double().sum(0)
    want = x[:, :K].double() @ w[:, :K].double().t()
    assert torch.equal(got, want)
    for z in range(nslice):                                     # every slice holds ITS bytes of K, nothing else
        k0, k1 = z * kslice, min(K, (z + 1) * kslice)
        wz = x[:, k0:k1].double() @ w[:, k0:k1].double().t() if k1 > k0 else torch.zeros_like(want)
        assert torch.equal(part[z, :, :N].double(), wz)


def _xnor_linear_fp64(x_pm1, w, bias):
    """functions/xnor_connect.py:112-115 in fp64: alpha = mean(|W|, 0, keepdim), y = x . (sign(W) * alpha)^T + b — applied to
    the weight the layer HOLDS: in eval mode that is the quantised image, which the op quantises again like upstream (with an
    all-zero output feature alpha shrinks by (N - 1) / N the second time)."""
    w64 = w.double().cpu()
    wq = torch.sign(w64) * w64.abs().mean(0, keepdim=True)
    y = x_pm1.double().cpu() @ wq.t()
    return y + bias.double().cpu() if bias is not None else y


@pytest.mark.parametrize("rows,N,K,hwc", [(256, 4096, 9216, (256, 6, 6)), (256, 4096, 4096, None), (256, 10, 4096, None),
                                          (5, 7, 100, None), (33, 70, 96, (6, 4, 4)), (64, 1000, 4096, None), (3, 32, 9216, (256, 6, 6)),
                                          (130, 17, 1030, None)])
def test_xnor_digit_linear_vs_fp64_and_vs_the_pair_route(dev, rows, N, K, hwc):
    torch.manual_seed(rows + N + K)
    lin = LinearXNOR(K, N, bias=True).to(dev)
    lin.weight.data.normal_(0, 0.05)
    lin.weight.data[:, 3] = 0.0                                  # a feature whose alpha is 0
    lin.weight.data[1, :] = 0.0                                  # an output feature of zeros: sign(0) = 0
    lin.bias.data.normal_(0, 1.0)
    lin.eval()
    x = BinaryConnectDeterministic.apply(torch.randn(rows, K, device=dev))
    planes = packed.lookup(x, packed.ROWS_LAST)
    assert planes is not None
    if hwc is not None:
        # the fused chain hands the features over in (h, w, c) order; the layer counts them in (c, h, w) order
        C, H, W = hwc
        xh = x.view(rows, C, H, W).permute(0, 2, 3, 1).reshape(rows, K).contiguous()
        planes = ops.sign_pack(xh)[0]
    act = packed.PackedActivation(planes, (rows, K))
    before = dict(_lib.call_counts)
    with torch.no_grad():
        y = _fused.packed_xnor_linear(lin, act, hwc=hwc)
        y2 = _fused.packed_xnor_linear(lin, act, hwc=hwc)
    route = "qt_xnor_head_i8" if N <= ops.XNOR_HEAD_MAX_N else "qt_i8_gemm_splitk"
    assert _lib.call_counts[route] - before.get(route, 0) == 2
    assert torch.equal(y, y2)
    if N <= ops.XNOR_HEAD_MAX_N:          # the one-launch head form and the split-K GEMM form: the same exact integer sum, the same bits
        old_n = ops.XNOR_HEAD_MAX_N
        try:
            ops.XNOR_HEAD_MAX_N = 0
            with torch.no_grad():
                yg = _fused.packed_xnor_linear(lin, act, hwc=hwc)
        finally:
            ops.XNOR_HEAD_MAX_N = old_n
        assert torch.equal(y, yg)
    ref = _xnor_linear_fp64(x, lin.weight.detach(), lin.bias)
    assert norm_err(n(y), n(ref)) <= TOL, norm_err(n(y), n(ref))
    old = _fused.XNOR_LINEAR_DIGITS
    try:
        _fused.XNOR_LINEAR_DIGITS = False
        with torch.no_grad():
            yp = _fused.packed_xnor_linear(lin, act, hwc=hwc)
    finally:
        _fused.XNOR_LINEAR_DIGITS = old
    assert norm_err(n(y), n(yp)) <= TOL
    # the module-by-module execution (fp32 activation carrying its sign planes) takes the same operands: same bits
    if hwc is None:
        with torch.no_grad():
            assert torch.equal(lin(x), y)


def test_xnor_digit_linear_falls_back_on_non_finite_alpha(dev):
    lin = LinearXNOR(128, 16, bias=False).to(dev)
    lin.weight.data.normal_(0, 0.05)
    lin.weight.data[2, 5] = float("inf")
    lin.eval()
    assert _fused.xnor_linear_digits(lin) is None
    x = BinaryConnectDeterministic.apply(torch.randn(8, 128, device=dev))
    with torch.no_grad():
        y = lin(x)
    assert not bool(torch.isfinite(y).all())                    # the reference's inf / NaN come through the pair route


# ---- reference digests of LinearXNOR at the classifier shapes (tests/golden/make_golden_r4c.py G19) -----------------------------------

import hashlib  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402

from conftest import GOLDEN_DIR  # noqa: E402
from pytorch_quantize_impls_amd import synth  # noqa: E402


def _g19_operands(seed, B, K, N):
    """The operands make_golden_r4c.py fed the reference: x +-1, |W[n, k]| = 2^e[k], bias multiples of 1/4."""
    x = synth.pm1(seed, (B, K))
    e = np.floor(synth.uniform(seed + 1, (K,), -6.0, -2.0)).astype(np.int32)
    sgn = synth.pm1(seed + 2, (N, K))
    w = (sgn * np.exp2(e.astype(np.float32))[None, :]).astype(np.float32)
    b = (np.round(synth.normal(seed + 3, (N,)) * 4) / 4).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("name", ["xnor_fc1_b256", "xnor_fc2_b256", "xnor_fc3_b256", "xnor_fc_ragged"])
@pytest.mark.parametrize("route", ["eval_digits", "eval_digits_gemm_only", "eval_packed_hwc", "eval_pairs", "train"])
def test_linear_xnor_reproduces_the_reference_digest(dev, name, route):
    """alpha[k] a power of two per input feature: the reference's fp32 result is exact whatever the summation order, and its SHA-256
    must come out of every route of this backend — the digit-plane int8 GEMM, the one-launch head, the fp16 pair route (eval and
    training-mode forward), and the packed activation whose bits arrive in (h, w, c) order."""
    with open(os.path.join(GOLDEN_DIR, "golden_hashes_r4c.json")) as fh:
        c = json.load(fh)["cases"][name]
    B, K, N = c["B"], c["K"], c["N"]
    x, w, b = _g19_operands(c["seed"], B, K, N)
    lin = LinearXNOR(K, N, bias=True).to(dev)
    lin.weight.data.copy_(torch.from_numpy(w))
    lin.bias.data.copy_(torch.from_numpy(b))
    xt = BinaryConnectDeterministic.apply(torch.from_numpy(x).to(dev))
    old_d, old_n = _fused.XNOR_LINEAR_DIGITS, ops.XNOR_HEAD_MAX_N
    before = dict(_lib.call_counts)
    try:
        if route == "train":
            lin.train()
            with torch.no_grad():
                y = lin(xt)
        else:
            lin.eval()
            assert torch.equal(lin.weight.detach().cpu(), torch.from_numpy(w))       # sign(W) * alpha == W: the image is a fixed point
            _fused.XNOR_LINEAR_DIGITS = route != "eval_pairs"
            if route == "eval_digits_gemm_only":
                ops.XNOR_HEAD_MAX_N = 0
            with torch.no_grad():
                if route == "eval_packed_hwc":
                    if K != 9216:
                        pytest.skip("the (h, w, c) hand-over is fc1's")
                    xh = xt.view(B, 256, 6, 6).permute(0, 2, 3, 1).reshape(B, K).contiguous()
                    act = packed.PackedActivation(ops.sign_pack(xh)[0], (B, K))
                    y = _fused.packed_xnor_linear(lin, act, hwc=(256, 6, 6))
                else:
                    y = lin(xt)
    finally:
        _fused.XNOR_LINEAR_DIGITS, ops.XNOR_HEAD_MAX_N = old_d, old_n
    used = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v != before.get(k, 0)}
    if route in ("eval_digits", "eval_packed_hwc"):
        assert used.get("qt_xnor_head_i8" if N <= 32 else "qt_i8_gemm_splitk", 0) == 1, used
    elif route == "eval_digits_gemm_only":
        assert used.get("qt_i8_gemm_splitk", 0) == 1 and "qt_xnor_head_i8" not in used, used
    else:
        assert used.get("qt_bits_alpha_pairs_f16x2", 0) == 1 and "qt_i8_gemm_splitk" not in used, used
    a = np.ascontiguousarray(y.detach().float().cpu().numpy(), dtype=np.float32)
    assert a.shape == (B, N)
    assert hashlib.sha256(a.tobytes()).hexdigest() == c["sha256_f32"], (float(a.astype(np.float64).sum()), c["sum"])


# ---- fp64 vectors of the REFERENCE's 8- / 32-bit DoReFa layers (tests/golden/make_golden_r4d.py G20) ----------------------------------

@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(GOLDEN_DIR, "golden_r4d_v1.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", ["conv8_s1_codes", "conv8_s2_real", "conv8_1x1_codes", "lin8_codes", "lin8_real", "conv32_s1", "lin32"])
def test_dorefa_8_and_32_bit_layers_vs_reference_fp64_vectors(dev, g20, all_shapes_on_the_routes, name):
    """Forward, grad_input, grad_weight and grad_bias of this backend's training-mode layers against the reference's own layers run in
    double precision (layers/dorefa_layers.py:11-82): <= 1e-5 normalised (2e-5 for the weight gradient through tanh / max|tanh|)."""
    g = {k: g20[f"g20_{name}_{k}"] for k in ("x", "w", "b", "go", "y", "gx", "gw", "gb", "geom")}
    geom = [int(v) for v in g["geom"]]
    bits, coded = geom[-2], bool(geom[-1])
    if name.startswith("conv"):
        B, Cin, Cout, H, k, s, p = geom[:7]
        layer = DorefaConv2d(Cin, Cout, k, stride=s, padding=p, bias=True, bit_width=bits)
    else:
        B, K, N = geom[:3]
        layer = LinearDorefa(K, N, bias=True, bit_width=bits)
    layer = layer.to(dev).train()
    layer.weight.data.copy_(torch.from_numpy(g["w"]))
    layer.bias.data.copy_(torch.from_numpy(g["b"]))
    raw = torch.from_numpy(g["x"]).to(dev)
    if raw.dim() == 4:
        raw = raw.contiguous(memory_format=torch.channels_last)
    raw.requires_grad_(True)
    x = nnDorefaQuant(4)(raw) if coded else raw * 1.0        # the stored activation IS a 4-bit image: the quantiser reproduces it
    if coded:
        assert torch.equal(x.detach().cpu(), torch.from_numpy(g["x"]))
    x.retain_grad()
    lib_before = dict(_fused.LIBRARY_PATHS)
    y = layer(x)
    y.backward(torch.from_numpy(g["go"]).to(dev))
    lib_now = _lib_delta(lib_before)
    allowed = set() if (coded or not name.startswith("conv")) else {"conv grad_weight outside the matrix-core route"}
    assert set(lib_now) <= allowed, lib_now
    assert norm_err(n(y), g["y"]) <= TOL
    assert norm_err(n(x.grad), g["gx"]) <= TOL
    assert norm_err(n(layer.weight.grad), g["gw"]) <= 2 * TOL
    assert norm_err(n(layer.bias.grad), g["gb"]) <= TOL


# ---- seeded geometry fuzz of the direct first-layer kernel (K axis in 8-byte groups, odd k-step counts, LDS offset table) ------------------

def test_first_layer_direct_conv_geometry_fuzz(dev):
    """40 random strided few-channel geometries (kernel 2 .. 11, stride 2 .. 4, 1 .. 4 channels, ragged maps, both storage orders,
    +-1 / 0 and real-valued weights, fp32 and threshold-bit epilogues) against the fp64 conv on the CPU: <= 1e-5 normalised; the
    threshold bits equal the float formula on the fp32 route's own output."""
    rng = np.random.default_rng(20260930)
    done = 0
    for _ in range(200):
        C = int(rng.integers(1, 5)); s = int(rng.integers(2, 5)); k = int(rng.integers(s, 12)); p = int(rng.integers(0, 4))
        H = int(rng.integers(k + 2, 60)); W = int(rng.integers(k + 2, 60)); N = int(rng.integers(1, 4)); Cout = int(rng.choice([5, 32, 40, 64, 96, 200]))
        if not ops.first_direct_applicable(C, (k, k), s, p, 1) or (H + 2 * p - k) // s + 1 <= 0 or (W + 2 * p - k) // s + 1 <= 0:
            continue
        real = bool(rng.integers(0, 2))
        x = torch.randn(N, C, H, W, device=dev) * float(rng.choice([0.01, 1.0, 300.0]))
        if rng.integers(0, 2):
            x = x.contiguous(memory_format=torch.channels_last)
        w = torch.randint(-1, 2, (Cout, C, k, k), device=dev).float()
        if real:
            w = w * (0.02 + torch.rand(1, 1, k, k, device=dev))                  # sign(W) * alpha[tap]
        b = torch.randn(Cout, device=dev)
        fw = ops.pack_first_layer_weight(w, s, real=real)
        y = ops.conv_first_direct(x, fw, b, s, p)
        if y is None:
            continue
        ref = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), s, p)
        Ho, Wo = ref.shape[2], ref.shape[3]
        got = y.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2)
        assert norm_err(n(got), n(ref)) <= TOL, (C, s, k, p, H, W, Cout, real, norm_err(n(got), n(ref)))
        al, be = torch.randn(Cout, device=dev), torch.randn(Cout, device=dev)
        bits = ops.conv_first_direct(x, fw, b, s, p, epi=(al, be))
        want = ops.sign_pack(((y * al + be)).contiguous())[0]                 # the float formula fl(fl(v * alpha) + beta) < 0 on the fp32 route
        assert torch.equal(bits.sign[:, :want.sign.shape[1]], want.sign), (C, s, k, p, H, W, Cout, real)
        done += 1
        if done == 40:
            break
    assert done >= 25, done


# ---- BatchNorm / sign / pack pass that also writes the next GEMM's nibble rows ---------------------------------------------------------

@pytest.mark.parametrize("rows,C", [(256, 4096), (64, 36), (33, 100), (40, 256), (7, 1000)])
def test_pool_affine_sign_pack_nib_rows_equal_the_separate_expansion(dev, rows, C):
    torch.manual_seed(rows + C)
    x = torch.randn(rows, C, device=dev)
    al, be = torch.randn(C, device=dev), torch.randn(C, device=dev)
    plain, _ = ops.pool_affine_sign_pack(x, al, be)
    both, _ = ops.pool_affine_sign_pack(x, al, be, want_nib=True)
    assert plain.nib is None and both.nib is not None
    assert torch.equal(plain.sign, both.sign)
    want = ops.bits_to_nib(plain)
    assert both.nib.words.shape == want.words.shape and torch.equal(both.nib.words, want.words)
    assert ops.to_impl(both, "mfma") is both.nib


# ---- per-tap scaled conv on the un-scaled conv's wide tiles (end of round 4: csrc/tile_select.h select_conv_taps) -----------------------

@pytest.mark.parametrize("Cin,Cout,H,k,p,B,tile", [
    (64, 256, 30, 3, 1, 64, "256x256"),        # M = 57 600: 225 tiles -> ConvPP256 / ConvVPP256
    (128, 768, 13, 3, 1, 256, "256x256"),      # AlexNet conv4's widths (two k-steps per tap)
    (64, 576, 27, 5, 2, 128, "384x192"),       # M = 93 312: the 384-row tile's rounds pay (prefer_384_rows)
    (192, 576, 14, 3, 1, 96, "256x192"),       # three k-steps per tap: boundaries alternate between stage start and mid-stage
])
def test_xnor_taps_conv_on_the_wide_tiles_vs_fp64(dev, Cin, Cout, H, k, p, B, tile):
    """XNORConv2d's integer-per-tap core (functions/xnor_connect.py:140-159: alpha = mean(|W|, [0, 1]) per tap) at sizes that take the
    256x256 / 384x192 / 256x192 ping-pong tiles, padded and on the physically padded plane (un-padded kernels): the two executions
    are bit-identical, and <= 1e-5 normalised against the fp64 evaluation of conv2d(x, sign(W) * alpha)."""
    from pytorch_quantize_impls_amd import ops
    g = torch.Generator(device=dev).manual_seed(Cin + Cout + k)
    x = torch.randn((B, Cin, H, H), device=dev, generator=g).sign_().contiguous(memory_format=torch.channels_last)
    w = torch.randn((Cout, Cin, k, k), device=dev, generator=g) * 0.05
    px = ops.pack_pixels_nib(x, ld=ops.pixel_ld_nib_taps(Cin))
    ws = ops.pack_conv_weight_nib(w, "sign", cw=px.ld)
    ts = ops.xnor_tap_prep(w)
    y0 = ops.conv2d_nib_taps(px, (B, Cin, H, H), ws, (k, k), ts.fwd, None, 1, p, 1)
    xp = torch.nn.functional.pad(x, (p, p, p, p)).contiguous(memory_format=torch.channels_last)
    pxp = ops.pack_pixels_nib(xp, ld=ops.pixel_ld_nib_taps(Cin))
    v = pxp.words.view(B, H + 2 * p, H + 2 * p, -1)
    v[:, :p] = 0; v[:, -p:] = 0; v[:, :, :p] = 0; v[:, :, -p:] = 0          # padding pixels are fp4 zeros, not +1
    y1 = ops.conv2d_nib_taps(pxp, (B, Cin, H + 2 * p, H + 2 * p), ws, (k, k), ts.fwd, None, 1, 0, 1)
    assert torch.equal(y0, y1), tile
    alpha = w.double().abs().mean(dim=(0, 1))
    ref = torch.nn.functional.conv2d(x.double(), torch.sign(w).double() * alpha[None, None], None, 1, p)
    assert norm_err(n(y0), n(ref.permute(0, 2, 3, 1).reshape(-1, Cout))) <= TOL, tile          # the kernel's result is NHWC rows


@pytest.mark.parametrize("Cin,Cout,H,k,p,B", [(64, 256, 30, 3, 1, 64), (128, 768, 13, 3, 1, 256), (64, 576, 27, 5, 2, 128)])
def test_xnor_taps_conv_wide_tile_epilogues_equal_the_float_predicate(dev, Cin, Cout, H, k, p, B):
    """The threshold-bit and nibble-plane epilogues of the wide tiles (their epilogue code is where the compiler's spills sit):
    bit = [(y + b) * alpha + beta < 0] evaluated on the fp32 result of the same conv, word for word; the nibble plane is the bit
    plane expanded (qt_bits_to_nib_pad) with its zero halo."""
    from pytorch_quantize_impls_amd import ops
    g = torch.Generator(device=dev).manual_seed(3 * Cin + Cout + k)
    x = torch.randn((B, Cin, H, H), device=dev, generator=g).sign_().contiguous(memory_format=torch.channels_last)
    w = torch.randn((Cout, Cin, k, k), device=dev, generator=g) * 0.05
    bias = torch.randn((Cout,), device=dev, generator=g) * 0.3
    px = ops.pack_pixels_nib(x, ld=ops.pixel_ld_nib_taps(Cin))
    ws = ops.pack_conv_weight_nib(w, "sign", cw=px.ld)
    ts = ops.xnor_tap_prep(w)
    args = (px, (B, Cin, H, H), ws, (k, k), ts.fwd, bias, 1, p, 1)
    y = ops.conv2d_nib_taps(*args)
    al = torch.rand((Cout,), device=dev, generator=g) * 2 - 1                      # negative BatchNorm slopes included
    be = (torch.rand((Cout,), device=dev, generator=g) * 2 - 1) * float(y.abs().mean())
    bits = ops.conv2d_nib_taps(*args, epi=(al, be))
    want = ops.sign_pack(torch.where(y * al < -be, -1.0, 1.0).contiguous())[0]
    nw = (Cout + 31) // 32
    M = B * H * H
    assert torch.equal(bits.sign.view(M, -1)[:, :nw], want.sign.view(M, -1)[:, :nw])
    frac = float((y * al < -be).float().mean())
    assert 0.2 < frac < 0.8                                                           # a real threshold, not all-0 / all-1 planes
    nib = ops.conv2d_nib_taps(*args, epi=ops.NibEpilogue(al, be, (1, 1)))
    want_n = ops.bits_to_nib_pad(bits, B, H, H, (1, 1), ld=ops.pixel_ld_nib(Cout))
    assert nib.rows == want_n.rows and torch.equal(nib.words, want_n.words)


@pytest.mark.parametrize("Cin,Cout,H,k,p,B", [(256, 64, 30, 3, 1, 64), (576, 64, 27, 5, 2, 128)])
def test_xnor_grad_input_on_the_wide_tiles_vs_fp64(dev, Cin, Cout, H, k, p, B):
    """grad_x of an XNOR-Net conv (functions/xnor_connect.py:154-155) at sizes whose transposed conv takes the 256x256 / 384x192
    tiles of the fp16-pair per-tap kernel: <= 1e-5 normalised against the fp64 conv2d_input of sign(W) * alpha."""
    from pytorch_quantize_impls_amd import ops
    g = torch.Generator(device=dev).manual_seed(Cin + 7 * Cout + k)
    w = torch.randn((Cout, Cin, k, k), device=dev, generator=g) * 0.05
    gout = torch.randn((B, Cout, H, H), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    ts = ops.xnor_tap_prep(w)
    before = dict(_lib.call_counts)
    gx = ops.conv2d_grad_input_taps((B, Cin, H, H), w, gout, ts.bwd, 1, p, 1)
    assert gx is not None and _lib.call_counts["qt_conv2d_implicit_taps"] == before.get("qt_conv2d_implicit_taps", 0) + 1
    alpha = w.double().abs().mean(dim=(0, 1))
    ref = torch.nn.grad.conv2d_input((B, Cin, H, H), torch.sign(w).double() * alpha[None, None], gout.double(), 1, p)
    assert norm_err(n(gx), n(ref)) <= TOL
