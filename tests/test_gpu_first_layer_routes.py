"""The forward route ladder of real-valued first-layer convs (functions/_fused.py ``first_layer_conv_routes``), rung by rung,
against digests RECORDED FROM THE COMMIT BEFORE THE LADDER EXISTED (tests/golden/first_layer_routes_v1.json: SHA-256 of the
result's bytes and the C-ABI call counts of the forward, written by ``python tests/test_gpu_first_layer_routes.py OUT.json`` with
that commit's package first on the import path).  Only entry points whose signatures the ladder left alone are called:
``_fused.quant_conv2d_forward``, an eval-mode ``FusedConvPoolBnSign`` and the functional ``XNORConv2d``.  Every case asserts the
bytes, the rung that ran (its entry point in ``_lib.call_counts``) and that the forward made exactly the recorded launches."""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from pytorch_quantize_impls_amd import _lib, ops, synth
from pytorch_quantize_impls_amd.functions import _fused, xnor_connect
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, XNORConv2d, FusedConvPoolBnSign, fused as fused_mod

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_layer_routes_v1.json")

# (C, Cout, k, stride, padding, dilation, H, W): the smallest shapes at which each rung can still go wrong
G_3X3 = (3, 64, 3, 1, 1, 1, 5, 7)            # first3x3: odd sizes, two row tiles
G_3X3_POOL = (3, 64, 3, 1, 1, 1, 6, 8)
G_DIRECT = (3, 32, 3, 1, 1, 1, 6, 6)         # direct3x3 on pair pixels (triples under bf16x3); d2s with the one-pass kernel off
G_DIRECT5 = (5, 32, 3, 1, 1, 1, 6, 6)        # five channels: triples forced
G_D2S6 = (6, 32, 3, 1, 1, 1, 6, 6)           # six channels: no direct kernel
G_ALEX = (3, 24, 11, 4, 2, 1, 33, 35)        # first_direct; as s2d the rounding adds a row (Ho = 7 of 8) and no column
G_K4S2 = (4, 24, 4, 2, 1, 1, 10, 10)
G_S2D1 = (3, 24, 5, 1, 2, 1, 9, 6)           # stride 1, padded: the s = 1 space-to-depth form
G_PLAIN = (3, 24, 3, 1, 0, 1, 6, 7)
G_DILATED = (3, 24, 3, 1, 1, 2, 6, 7)
G_XNOR3 = (3, 24, 3, 1, 1, 1, 6, 7)

NO_3X3 = {"FIRST_3X3": False}
NO_DIRECT_BLOCK = {"FIRST_3X3": False, "DIRECT_FIRST_LAYER": False}
NO_FIRST_DIRECT = {"FIRST_DIRECT": False}

#: entry points that tell which rung ran (any one of them, and none of the rungs' ahead of it).  "d2s" and "s2d" make the same
#: launches: test_runner_names_the_rung_the_block_takes tells them apart through ``taken``
MARKS = {
    "first3x3": ("qt_conv3x3_first_f32",),
    "direct3x3": ("qt_conv3x3_direct_pairs", "qt_conv3x3_direct_nib"),
    "first_direct": ("qt_conv_first_direct_f32", "qt_conv_first_direct_bits_f32"),
    "first_direct_real": ("qt_conv_first_direct_f32", "qt_conv_first_direct_bits_f32"),
    "s2d": ("qt_f16x2_s2d_pack_f32", "qt_f16x2_s2d_pack_spec_f32", "qt_bf16x3_s2d_pack_f32"),
    "d2s": ("qt_f16x2_s2d_pack_f32", "qt_f16x2_s2d_pack_spec_f32", "qt_bf16x3_s2d_pack_f32"),
    "plain": ("qt_f16x2_pack_f32", "qt_f16x2_absmax_pack_f32", "qt_bf16x3_pack_f32"),
    "bf16x6": ("qt_bf16x6_pack_f32",),
}
_AHEAD = {"s2d": ("first3x3", "direct3x3", "first_direct"), "d2s": ("first3x3", "direct3x3"), "plain": ("first3x3", "first_direct", "s2d"),
          "bf16x6": ("first_direct_real",), "first_direct": ("first3x3",), "direct3x3": ("first3x3",)}


def _cases():
    """(id, rung, entry, kind, geometry, batch, output form, switches).  entry: "forward" = quant_conv2d_forward, "block" =
    FusedConvPoolBnSign, "function" = the functional XNORConv2d.  Output forms: "f32", "bits", "nib11", "nib22", "pool"."""
    out = []

    def add(rung, entry, kind, geom, form, sw=None, batch=2, tag=""):
        name = "-".join(str(v) for v in (rung, entry, kind, "x".join(str(g) for g in geom), f"n{batch}", form)) + tag
        out.append((name, rung, entry, kind, geom, batch, form, sw or {}))

    for kind in ("binary", "ternary"):
        for form in ("f32", "bits", "nib11", "nib22"):
            add("first3x3", "forward", kind, G_3X3, form)
        for form in ("bits", "nib11", "nib22"):
            add("first3x3", "block", kind, G_3X3, form)
        add("first3x3", "block", kind, G_3X3_POOL, "pool")
    add("first3x3", "forward", "binary", G_3X3, "nib11", batch=1)
    for geom, sw, tag in ((G_DIRECT, {}, ""), (G_DIRECT, {"FLOAT_SPLIT": "bf16x3"}, "-bf16x3"), (G_DIRECT5, {}, "")):
        for form in ("bits", "nib11", "pool"):
            add("direct3x3", "block", "binary", geom, form, sw, tag=tag)
    add("direct3x3", "block", "ternary", G_DIRECT, "bits", batch=1)
    add("d2s", "block", "binary", G_DIRECT, "nib11", NO_DIRECT_BLOCK)
    add("d2s", "block", "ternary", G_D2S6, "nib11", NO_DIRECT_BLOCK)
    add("d2s", "block", "binary", G_D2S6, "nib11", NO_DIRECT_BLOCK, batch=1)
    for geom, kind in ((G_ALEX, "binary"), (G_K4S2, "ternary")):
        for form in ("f32", "bits", "nib22"):
            add("first_direct", "forward", kind, geom, form)
    add("first_direct", "block", "binary", G_ALEX, "bits")
    add("first_direct", "block", "binary", G_ALEX, "nib22")
    add("first_direct", "forward", "binary", G_ALEX, "bits", batch=1)
    for geom, kind in ((G_ALEX, "binary"), (G_S2D1, "ternary")):
        for form in ("f32", "bits", "nib11"):
            add("s2d", "forward", kind, geom, form, NO_FIRST_DIRECT)
    add("s2d", "block", "binary", G_ALEX, "nib11", NO_FIRST_DIRECT)
    add("s2d", "forward", "binary", G_ALEX, "bits", NO_FIRST_DIRECT, batch=1)
    for geom, kind in ((G_PLAIN, "binary"), (G_DILATED, "ternary")):
        for form in ("f32", "bits"):
            add("plain", "forward", kind, geom, form)
    add("plain", "forward", "binary", G_PLAIN, "f32", batch=1)
    for rung, geom in (("first_direct_real", G_ALEX), ("bf16x6", G_XNOR3)):
        add(rung, "function", "xnor", geom, "f32")
        add(rung, "block", "xnor", geom, "bits")
        add(rung, "block", "xnor", geom, "nib11")
        add(rung, "block", "xnor", geom, "bits", batch=1)
    return out


CASES = _cases()


def g(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


@contextlib.contextmanager
def switches(sw):
    """The route switches of a case, each set where the package reads it, and put back afterwards."""
    sw = dict(sw)
    split = sw.pop("FLOAT_SPLIT", None)
    homes = {"DIRECT_FIRST_LAYER": fused_mod, "D2S_FIRST_LAYER": fused_mod, "USE_S2D": _fused}
    moved = {k: sw.pop(k) for k in list(sw) if k in homes}
    saved = {k: getattr(homes[k], k) for k in moved}
    for k, v in moved.items():
        setattr(homes[k], k, v)
    try:
        with ops.scope(**sw), ops.float_split(split):
            yield
    finally:
        for k, v in saved.items():
            setattr(homes[k], k, v)


def operands(kind, geom, batch, dev, exact=False, given=None):
    """(image, weight, bias, alpha, beta) from fixed seeds; ``exact``: an image of multiples of 1/8, whose partial sums against
    +-1 / 0 weights are exact in fp32 whatever the order of the accumulation.  ``given``: the caller's own device operands
    (image, weight, bias, alpha, beta[, BatchNorm (running_mean, running_var, weight, bias) of a block]) instead, as they are
    (tests/test_gpu_first_layer_exact.py: designed operands in the storage order under test)."""
    if given is not None:
        return tuple(given[:5])
    C, Cout, k = geom[:3]
    H, W = geom[6:]
    img = synth.normal(71, (batch, C, H, W))
    x = g(np.round(img * 16) / 8 if exact else img * 2.0, dev).contiguous(memory_format=torch.channels_last)
    w = g(synth.uniform(72, (Cout, C, k, k), -1.2, 1.2), dev)
    b = g(synth.uniform(73, (Cout,), -1, 1), dev)
    alpha = g(synth.uniform(74, (Cout,), -1, 1), dev)
    beta = g(synth.uniform(75, (Cout,), -3, 3), dev)
    return x, w, b, alpha, beta


def make_block(kind, geom, form, dev, w, b, bn_stats=None):
    C, Cout, k, st, pd, dl = geom[:6]
    cls = {"binary": BinConv2d, "ternary": TerConv2d, "xnor": XNORConv2d}[kind]
    conv = cls(C, Cout, k, stride=st, padding=pd, dilation=dl).to(dev)
    conv.weight.data.copy_(w)
    conv.bias.data.copy_(b)
    conv.binary_input = False
    conv.eval()
    bn = torch.nn.BatchNorm2d(Cout).to(dev).eval()
    mean, var, gamma, shift = bn_stats if bn_stats is not None else (g(synth.normal(76, (Cout,)), dev), g(synth.uniform(77, (Cout,), 0.5, 4), dev),
                                                                     g(synth.normal(78, (Cout,)), dev), g(synth.normal(79, (Cout,)), dev))
    bn.running_mean.copy_(mean)
    bn.running_var.copy_(var)
    bn.weight.data.copy_(gamma)
    bn.bias.data.copy_(shift)
    blk = FusedConvPoolBnSign(conv, bn, torch.nn.MaxPool2d(2, 2) if form == "pool" else None)
    blk.out_nib_halo = {"nib11": (1, 1), "nib22": (2, 2)}.get(form)
    return blk


def forward_epi(form, alpha, beta):
    if form == "f32":
        return None
    if form == "bits":
        return (alpha, beta)
    return ops.NibEpilogue(alpha, beta, {"nib11": (1, 1), "nib22": (2, 2)}[form])


def run_case(case, dev, exact=False, given=None):
    """Runs one case; returns (result tensor whose bytes are digested, {entry point: calls of the forward}).  ``given``: see ``operands``."""
    _, _, entry, kind, geom, batch, form, sw = case
    st, pd, dl = geom[3:6]
    x, w, b, alpha, beta = operands(kind, geom, batch, dev, exact, given)
    with switches(sw), torch.no_grad():
        blk = make_block(kind, geom, form, dev, w, b, given[5] if given is not None and len(given) > 5 else None) if entry == "block" else None
        torch.cuda.synchronize()
        before = dict(_lib.call_counts)
        if entry == "forward":
            res = _fused.quant_conv2d_forward(x, w, b, st, pd, dl, 1, kind, binary_input=False, epi=forward_epi(form, alpha, beta))
            res = res if form == "f32" else res[0]
        elif entry == "function":
            res = xnor_connect.XNORConv2d([0, 1], False, st, pd, dl, 1).apply(x, w, b)
        else:
            res = blk(x)
            res = res.nib if form.startswith("nib") else res.planes
        calls = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v - before.get(k, 0)}
    if isinstance(res, ops.NibPlanes):
        assert form.startswith("nib"), (form, type(res))
        res = res.words
    elif isinstance(res, ops.BitPlanes):
        assert form in ("bits", "pool"), (form, type(res))
        res = res.sign
    else:
        assert form == "f32" and res.dtype == torch.float32, (form, type(res))
    return res, calls


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rung_reproduces_the_recorded_bytes_and_launches(dev, recorded, case):
    name, rung = case[:2]
    res, calls = run_case(case, dev)
    print(name, digest(res), calls)
    assert any(calls.get(k) for k in MARKS[rung]), (rung, calls)
    for ahead in _AHEAD.get(rung, ()):
        assert not any(calls.get(k) for k in MARKS[ahead]), (rung, ahead, calls)
    assert calls == recorded[name]["calls"]
    assert digest(res) == recorded[name]["sha256"]


DIRECT = [c for c in CASES if c[2] == "forward"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIRECT, ids=[c[0] for c in DIRECT])
def test_runner_names_the_rung_it_took(dev, recorded, case):
    """``first_layer_conv_routes`` called as quant_conv2d_forward calls it: ``taken`` receives the rung, the bytes are the recorded ones."""
    name, rung, _, kind, geom, batch, form, sw = case
    x, w, b, alpha, beta = operands(kind, geom, batch, dev)
    taken = []
    with switches(sw), torch.no_grad():
        y, (N, Cout, Ho, Wo) = _fused.first_layer_conv_routes(x, w, b, *geom[3:6], kind, epi=forward_epi(form, alpha, beta),
                                                              rungs=("first3x3", "first_direct", "s2d", "plain"), taken=taken)
    assert taken == [rung] and (N, Cout) == (batch, geom[1])
    res = y.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2) if form == "f32" else (y.words if form.startswith("nib") else y.sign)
    assert digest(res) == recorded[name]["sha256"]


BLOCKS = [c for c in CASES if c[2] == "block"]
BLOCK_RUNGS = ("first3x3", "direct3x3", "d2s")


@pytest.mark.gpu
@pytest.mark.parametrize("case", BLOCKS, ids=[c[0] for c in BLOCKS])
def test_runner_names_the_rung_the_block_takes(dev, recorded, case):
    """``first_layer_conv_routes`` called as FusedConvPoolBnSign calls it (the layer's cached operands, the block's rungs, the
    folded BatchNorm): ``taken`` names the rung — the call counts cannot tell "d2s" from "s2d", which make the same launches — and
    the conv's bytes are the recorded ones.  A case whose rung belongs to the conv's own ladder comes back None: the block falls
    through to quant_conv2d_forward."""
    name, rung, _, kind, geom, batch, form, sw = case
    x, w, b, _, _ = operands(kind, geom, batch, dev)
    taken = []
    with switches(sw), torch.no_grad():
        blk = make_block(kind, geom, form, dev, w, b)
        conv = blk.conv
        alpha, beta = fused_mod.fold_batchnorm(blk.bn)
        epi = (alpha, beta) if form in ("bits", "pool") else ops.NibEpilogue(alpha, beta, blk.out_nib_halo)
        out = _fused.first_layer_conv_routes(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, kind, epi=epi,
                                             cache=conv._conv_triples, rungs=None if kind == "xnor" else BLOCK_RUNGS,
                                             pooled=form == "pool", taken=taken)
    if kind != "xnor" and rung not in BLOCK_RUNGS:
        assert out is None and taken == []
        return
    assert taken == [rung]
    y, shape = out
    assert shape[:2] == (batch, geom[1])
    if form != "pool":          # (the recorded bytes of a pooled block are the pool's)
        assert digest(y.words if form.startswith("nib") else y.sign) == recorded[name]["sha256"]


# The XNOR rungs have an fp32 form (the function) and a bits form (the block) too, but their weight image sign(W) * alpha is real:
# no input makes the partial sums exact, so the two forms may differ at ties by accumulation order and are not compared here.
TIES = [c for c in CASES if c[2] == "forward" and c[6] == "bits" and c[5] == 2]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIES, ids=[c[0] for c in TIES])
def test_threshold_bits_come_from_the_accumulators_of_the_fp32_output(dev, case):
    """With partial sums that are exact in fp32 (an image of multiples of 1/8), the bit plane of a rung is
    [y * alpha + beta < 0] of that rung's own fp32 output y: the fused chain and the module-by-module execution agree at ties."""
    name, rung, entry, kind, geom, batch, _, sw = case
    bits, calls = run_case(case, dev, exact=True)
    y, calls32 = run_case((name, rung, entry, kind, geom, batch, "f32", sw), dev, exact=True)
    for c in (calls, calls32):
        assert any(c.get(k) for k in MARKS[rung]), (rung, c)
    _, _, _, alpha, beta = operands(kind, geom, batch, dev, exact=True)
    Cout = geom[1]
    yn = y.permute(0, 2, 3, 1).reshape(-1, Cout).cpu().numpy()
    want = ((yn * alpha.cpu().numpy()).astype(np.float32) + beta.cpu().numpy()) < 0
    words = bits.cpu().numpy().view(np.uint32)
    got = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(words.shape[0], -1)[:, :Cout].astype(bool)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


if __name__ == "__main__":      # the recorder: run with the package to record from first on the import path
    device = torch.device("cuda:0")
    rec = {}
    for c in CASES:
        r, n_calls = run_case(c, device)
        rec[c[0]] = {"sha256": digest(r), "calls": dict(sorted(n_calls.items()))}
    with open(sys.argv[1], "w") as fh:
        json.dump({"cases": rec}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", len(rec), "cases from", ops.__file__)
