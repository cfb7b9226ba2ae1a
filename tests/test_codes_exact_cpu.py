"""tests/_codes_exact.py pinned without a GPU: the float64 emulation of the DoReFa code epilogue equals exact rational arithmetic with
one correctly rounded fp32 result per operation; the designed operands are exact at every step and hold the share of exact ties
the GPU cases rely on; realistic parameters leave (next to) no element the reference cannot decide; plane helpers round-trip."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _codes_exact as CX  # noqa: E402

# ---- exact rational arithmetic, one correctly rounded fp32 result per operation -----------------------------------------------
# finite values are Fractions, infinities and NaN Python floats (their arithmetic is IEEE's; signed zeros do not reach a code)


def rn32(x):
    """Round a rational to the nearest fp32 (ties to even, subnormals, overflow to infinity) with integer arithmetic only."""
    if not isinstance(x, Fraction):
        return x
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n = a / ulp
    k, r = divmod(n.numerator, n.denominator)
    if 2 * r > n.denominator or (2 * r == n.denominator and k & 1):
        k += 1
    res = k * ulp
    if res >= Fraction(2) ** 128:
        return math.copysign(math.inf, x)
    return res if x > 0 else -res


def _fin(*v):
    return all(isinstance(t, Fraction) for t in v)


def q_mul(a, b):
    return rn32(a * b) if _fin(a, b) else float(a) * float(b)


def q_add(a, b):
    return rn32(a + b) if _fin(a, b) else float(a) + float(b)


def q_fma(a, b, c):
    if _fin(a, b, c):
        return rn32(a * b + c)
    return float(a) * float(b) + float(c)            # a special operand: no rounding question left


def q_relu(t):
    return Fraction(0) if (t < 0) else t             # NaN < 0 is False


def q_rint(t):
    if not _fin(t):
        return t
    k, r = divmod(t.numerator, t.denominator)
    if 2 * r > t.denominator or (2 * r == t.denominator and k & 1):
        k += 1
    return Fraction(k)


def frac(x):
    x = float(x)
    return Fraction(x) if math.isfinite(x) else x


def rational_chain(e):
    """One element through the epilogue; ``e``: dict of python floats (fp32 values).  Returns (code, ok, t)."""
    v = q_mul(frac(e["acc"]), frac(e["scale"]))
    if e.get("cbias") is not None:
        v = q_add(v, frac(e["cbias"]))
    if e["relu"] == 2:
        v = q_relu(v)
    if e.get("mean") is not None:
        t = q_fma(q_mul(q_add(v, -frac(e["mean"])), frac(e["rs"])), frac(e["alpha"]), frac(e["beta"]))
    else:
        t = q_add(q_mul(v, frac(e["alpha"])), frac(e["beta"]))
    if e.get("u") is not None:
        u = frac(e["u"])
        if e.get("rmean") is not None:
            u = q_fma(q_mul(q_add(u, -frac(e["rmean"])), frac(e["rrs"])), frac(e["ra"]), frac(e["rb"]))
        elif e.get("ra") is not None:
            u = q_add(q_mul(u, frac(e["ra"])), frac(e["rb"]))
        t = q_add(t, u)
    if e.get("rc") is not None:
        t = q_add(t, q_mul(frac(e["rscale"]), frac(e["rc"])))
    if e["relu"] == 1:
        t = q_relu(t)
    q = q_rint(q_mul(frac(e["levels"]), t))
    ok = abs(q) <= 127                                # NaN: False
    return (int(q) if ok else 0), ok, t


def test_rn32_agrees_with_numpy_on_float64_inputs():
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-44, 39, 2000), [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -150,
                         2.0 ** -149 * 1.5, 3.4028235677973366e38, 3.4028235e38, -1e39, 0.0]])
    with np.errstate(over="ignore"):
        for x in xs:
            want = float(np.float32(x))
            got = rn32(Fraction(float(x)))
            assert float(got) == want, (x, got, want)


FORMS = ["device", "device_rc", "device_rf", "device_rf_bn", "folded", "folded_rf_affine", "folded_rc_bias_pre"]
ELEMS = 3000


def _elements(form, rng):
    """Seeded per-element operands as fp32 arrays; every element is its own channel.  A share of the elements is steered onto
    half-integer levels * t, onto the +-127 / +-128 edge, and onto NaN / inf parameters."""
    f = np.float32
    n = ELEMS
    levels = rng.choice([3.0, 15.0, 255.0], n).astype(f)
    e = {"acc": rng.integers(-5000, 5000, n).astype(f), "scale": (rng.random(n) * 0.01 + 1e-4).astype(f), "levels": levels,
         "relu": np.full(n, 2 if form.endswith("pre") else int(rng.integers(0, 2)))}
    dev = form.startswith("device")
    if dev:
        e["mean"], e["rs"] = (rng.standard_normal(n) * 3).astype(f), (1 / np.sqrt(rng.random(n) * 50 + 50)).astype(f)
        e["alpha"], e["beta"] = (rng.random(n) + 0.5).astype(f) * rng.choice([-1, 1], n).astype(f), (rng.standard_normal(n) * 0.3).astype(f)
    else:
        e["alpha"], e["beta"] = (rng.standard_normal(n) * 0.2).astype(f), (rng.standard_normal(n)).astype(f)
    if "_rf" in form:
        e["u"] = (rng.standard_normal(n) * 2).astype(f)
        if form == "device_rf_bn":
            e["rmean"], e["rrs"] = (rng.standard_normal(n)).astype(f), (rng.random(n) * 0.2 + 0.05).astype(f)
            e["ra"], e["rb"] = (rng.random(n) + 0.5).astype(f), (rng.standard_normal(n) * 0.1).astype(f)
        elif form == "folded_rf_affine":
            e["ra"], e["rb"] = (rng.standard_normal(n) * 0.5).astype(f), (rng.standard_normal(n) * 0.5).astype(f)
    if "_rc" in form:
        e["rc"], e["rscale"] = rng.integers(-128, 128, n).astype(f), np.full(n, f(1) / f(15), dtype=f)
    if "bias" in form:
        e["cbias"] = (rng.standard_normal(n)).astype(f)
    # exact ties and the int8 edge: alpha = 1 (rs = 1, mean = 0), scale = 1/4 or 1/2, beta chosen so that levels * t = x.5 or +-127.x
    k = n // 5
    for i in range(k):
        e["scale"][i] = 0.25
        e["alpha"][i] = 1.0
        if dev:
            e["mean"][i], e["rs"][i] = 0.0, 1.0
        for key in ("u", "rc", "cbias"):
            if key in e:
                e[key][i] = 0.0
        if "rb" in e:
            e["ra"][i], e["rb"][i] = 1.0, 0.0
        if "rmean" in e:
            e["rmean"][i], e["rrs"][i] = 0.0, 1.0
        e["relu"][i] = 0
        if i % 2 == 0:       # levels * t = m + 0.5 exactly where levels = 3, 15, 255 times a multiple of 1/2 .. 1/4
            e["levels"][i] = 15.0
            e["acc"][i] = f(4 * rng.integers(-8, 9) + 2)             # acc / 4 = j + 1/2 -> 15 t = 15 j + 7.5
            e["beta"][i] = 0.0
        else:                # q around +-127 / +-128: 15 t = 126.x .. 128.x
            e["levels"][i] = 15.0
            e["acc"][i] = f(rng.choice([-1, 1]) * rng.integers(33, 36))   # acc / 4 = 8.25 .. 8.75 -> 123.75 .. 131.25
            e["beta"][i] = f(rng.integers(-2, 3)) / f(15)
    # NaN / inf parameters and overflowing products
    sp = [float("nan"), float("inf"), float("-inf"), 1e6, -1e6, 0.0, -0.0, 3e38]
    for i in range(k, k + 64):
        key = ["alpha", "beta", "scale"][i % 3]
        e[key][i] = f(sp[(i // 3) % len(sp)])
    if dev:
        for i in range(k + 64, k + 80):
            e["rs"][i] = f(1e30)
    return e


@pytest.mark.parametrize("form", FORMS)
def test_emulation_equals_rational_arithmetic(form):
    rng = np.random.default_rng(FORMS.index(form) + 7)
    e = _elements(form, rng)
    T = {k: torch.from_numpy(np.asarray(v)) for k, v in e.items() if k != "relu"}
    ties = inside = outside = specials = 0
    for relu in (0, 1, 2):
        sel = np.nonzero(e["relu"] == relu)[0]
        if sel.size == 0:
            continue
        idx = torch.from_numpy(sel)
        g = {k: v[idx] for k, v in T.items()}
        # levels differ per element here: run the emulation once per level value
        for lv in (3.0, 15.0, 255.0):
            m = g["levels"] == lv
            if not bool(m.any()):
                continue
            h = {k: v[m] for k, v in g.items()}
            v = CX.conv_value(h["acc"], h["scale"], h.get("cbias"))
            ra = None
            if "rmean" in h:
                ra = (h["ra"], h["rb"], (h["rmean"], h["rrs"]))
            elif "ra" in h:
                ra = (h["ra"], h["rb"])
            p = CX.Epi(h["alpha"], h["beta"], lv, (h["mean"], h["rs"]) if "mean" in h else None, relu, h.get("u"), ra, h.get("rc"),
                       float(h["rscale"][0]) if "rscale" in h else 0.0)
            ref = CX.epilogue(v, p)
            rows = sel[m.numpy()]
            for j, i in enumerate(rows):
                el = {k: (float(val[i]) if k != "relu" else int(val[i])) for k, val in e.items()}
                code, ok, t = rational_chain(el)
                got_t = float(ref["t"][j])
                amb = int(ref["lo"][j]) != int(ref["hi"][j])
                if not amb:
                    assert int(ref["codes"][j]) == code, (form, i, el, int(ref["codes"][j]), code)
                    if isinstance(t, Fraction):
                        assert Fraction(got_t) == t, (form, i, el, got_t, float(t))
                    else:
                        assert (math.isnan(t) and math.isnan(got_t)) or got_t == t, (form, i, el, got_t, t)
                else:
                    assert int(ref["lo"][j]) <= code <= int(ref["hi"][j]), (form, i, el)
                if isinstance(t, Fraction):
                    lt = Fraction(el["levels"]) * t
                    ties += (2 * lt).denominator == 1 and lt.denominator == 2
                    inside += bool(ok) and abs(lt) >= 120          # just inside int8 ...
                    outside += (not ok) and abs(lt) <= 135           # ... and just outside: code 0
                else:
                    specials += 1
    assert ties >= 100 and inside >= 30 and outside >= 30 and specials >= 10, (ties, inside, outside, specials)


def test_fma_ambiguity_is_reported():
    """An fma whose float64 sum is an fp32 midpoint without being exact: the reference names both neighbours, and the rational
    result is one of them."""
    a, b = torch.tensor([2.0 ** -9 * (1 + 2.0 ** -23)]), torch.tensor([2.0 ** -8 * (1 - 2.0 ** -23)])
    c = torch.tensor([128.0])          # a * b + c = 128 + 2^-17 - 2^-63: float64 keeps 128 + 2^-17, the midpoint of 128 and 128 + 2^-16
    r, alt = CX.f_fma(a, b, c)
    assert float(r) != float(alt) and {float(r), float(alt)} == {128.0, 128.0 + 2.0 ** -16}
    assert float(rn32(Fraction(float(a)) * Fraction(float(b)) + 128)) == 128.0
    r, alt = CX.f_fma(torch.tensor([3.0]), torch.tensor([0.5]), torch.tensor([0.25]))      # exact: nothing to tell apart
    assert float(r) == float(alt) == 1.75


# ---- designed operands --------------------------------------------------------------------------------------------------------

DESIGNED = [(64, 64, 3, 8, 8), (40, 52, 3, 9, 11), (40, 50, 3, 9, 11), (128, 128, 3, 4, 4), (64, 128, 1, 8, 8), (512, 64, 3, 4, 4)]


@pytest.mark.parametrize("Cin,Cout,k,H,W", DESIGNED)
@pytest.mark.parametrize("form", ["device", "folded"])
def test_designed_operands_are_exact_and_hold_ties(Cin, Cout, k, H, W, form):
    N = 3
    codes = CX.random_codes((N, Cin, H, W), 0, 3, Cin + H, "cpu")
    w = CX.pm1_weights(Cout, Cin, k, Cout + k, "cpu")
    acc = CX.exact_acc(codes, w, 1, k // 2).permute(0, 2, 3, 1)
    shift = CX.designed_shift(Cin * k * k)
    scale, alpha, beta, stats = CX.designed_params(Cout, shift, 5, "cpu", form)
    rc = CX.random_codes((N, H, W, Cout), 0, 15, 9, "cpu")
    for relu, res in ((1, None), (0, rc), (2, None)):
        p = CX.Epi(alpha, beta, 15.0, stats, relu, res_codes=res, rscale=0.25)
        ref = CX.epilogue(CX.conv_value(acc, CX.kernel_scale(scale)), p)
        # the same chain in plain float64, no intermediate rounding: every step of the fp32 chain was exact
        v = acc * 0.25
        if relu == 2:
            v = v.clamp_min(0)
        t = ((v - stats[0].double()) * stats[1].double() * alpha.double() + beta.double()) if stats is not None else v * alpha.double() + beta.double()
        if res is not None:
            t = t + 0.25 * res.double()
        if relu == 1:
            t = t.clamp_min(0)
        assert torch.equal(ref["t"].double(), t)
        lt = 15.0 * t
        q = torch.round(lt)
        assert torch.equal(torch.where(q.abs() <= 127, q, torch.zeros_like(q)).long(), ref["codes"])
        assert int(CX.sensitive(ref).sum()) == 0
        # the share is taken over the elements the ReLU leaves a spread value: t > 0 behind it, acc > 0 in front of it
        live = (t != 0) if relu == 1 else ((acc > 0) if relu == 2 else torch.ones_like(t, dtype=torch.bool))
        ties = ((lt - torch.floor(lt)) == 0.5) & live
        assert int(ties.sum()) * 100 >= int(live.sum()), (relu, int(ties.sum()), int(live.sum()), shift)


# ---- realistic parameters ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["device", "folded"])
def test_realistic_parameters_leave_the_reference_decided(form):
    """At the GPU module's smallest conv shape (3 x 40 x 9 x 11 -> 52): the elements whose code the reference cannot decide
    (an ambiguous fma) stay within the one-per-million cap, and the codes use the quantiser's range."""
    N, Cin, Cout, H, W = 3, 40, 52, 9, 11
    codes = CX.random_codes((N, Cin, H, W), 0, 15, 1, "cpu")
    w = CX.pm1_weights(Cout, Cin, 3, 2, "cpu")
    acc = CX.exact_acc(codes, w, 1, 1).permute(0, 2, 3, 1)
    inv, E, alpha, beta, stats = CX.realistic_params(Cout, Cin * 9, 3, "cpu", form)
    ref = CX.epilogue(CX.conv_value(acc, CX.kernel_scale(inv, E)), CX.Epi(alpha, beta, 15.0, stats, 1))
    n = ref["codes"].numel()
    assert int(CX.sensitive(ref).sum()) <= CX.waiver_cap(n)
    assert not ref["flag"] and int(ref["codes"].max()) >= 15 and int((ref["codes"] > 0).sum()) * 4 >= n


def test_cancelling_parameters_tell_the_fma_from_multiply_and_add():
    """At the GPU module's smallest full-tile shape (4 x 64 x 8 x 8 -> 64): with the offset parameters a multiply-then-add epilogue
    gives other codes than the fma for at least 5 elements (so a GPU case on them fails for such a kernel), the reference stays
    decided, and no code leaves int8."""
    N, Cin, Cout, H = 4, 64, 64, 8
    codes = CX.random_codes((N, Cin, H, H), 0, 15, 1, "cpu")
    acc = CX.exact_acc(codes, CX.pm1_weights(Cout, Cin, 3, 2, "cpu"), 1, 1).permute(0, 2, 3, 1)
    inv, E, w, b, stats = CX.cancelling_params(Cout, Cin * 9, 3, "cpu")
    v = CX.conv_value(acc, CX.kernel_scale(inv, E))
    ref = CX.epilogue(v, CX.Epi(w, b, 15.0, stats, 1))
    x = CX.f_mul(CX.f_sub(v, stats[0]), stats[1])
    split = CX.quantise(CX.f_relu(CX.f_add(CX.f_mul(x, w), b)), 15.0)[0]
    assert int((split != ref["codes"]).sum()) >= 5, int((split != ref["codes"]).sum())
    assert int(CX.sensitive(ref).sum()) <= CX.waiver_cap(ref["codes"].numel()) and not ref["flag"]
    assert int(ref["codes"].max()) >= 15 and int((ref["codes"] > 0).sum()) * 4 >= ref["codes"].numel()


def test_oracle_agrees_on_the_folded_head_chain():
    """oracle.affine_relu_dorefa_codes (the C restatement's Python twin) and this reference give the same codes for the folded form."""
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((33, 40)) * 2).astype(np.float32)
    alpha, beta = (rng.standard_normal(40) * 0.5).astype(np.float32), rng.standard_normal(40).astype(np.float32)
    got = O.affine_relu_dorefa_codes(x, alpha, beta, 4, relu=True)
    codes = got[0] if isinstance(got, tuple) else got
    ref = CX.epilogue(torch.from_numpy(x), CX.Epi(torch.from_numpy(alpha), torch.from_numpy(beta), 15.0, None, 1))
    assert np.array_equal(np.asarray(codes)[:, :40].astype(np.int64), ref["codes"].numpy())


# ---- plane helpers -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("halo", [(0, 0), (1, 1), (2, 1), (3, 0)])
@pytest.mark.parametrize("C", [3, 40, 64])
def test_plane_round_trip_and_zero_checks(halo, C):
    N, H, W = 2, 5, 4
    q = CX.random_codes((N, C, H, W), -128, 127, C, "cpu")
    q[0, 0, 0, 0], q[-1, -1, -1, -1] = 127, -128          # corners non-zero so that a shifted border shows
    plane = CX.encode_plane(q, halo)
    assert plane.shape == (N * (H + 2 * halo[0]) * (W + 2 * halo[1]), CX.code_ld(C)) and plane.dtype == torch.int8
    assert torch.equal(CX.decode_plane(plane, N, H, W, C, halo), q)
    if CX.code_ld(C) > C:
        bad = plane.clone()
        bad.view(N, H + 2 * halo[0], W + 2 * halo[1], -1)[1, halo[0], halo[1], C] = 1
        with pytest.raises(AssertionError, match="pad bytes"):
            CX.decode_plane(bad, N, H, W, C, halo)
    if any(halo):
        bad = plane.clone()
        bad.view(N, H + 2 * halo[0], W + 2 * halo[1], -1)[0, 0, 0, 0] = 1
        with pytest.raises(AssertionError, match="halo border"):
            CX.decode_plane(bad, N, H, W, C, halo)


def test_exact_acc_refuses_sums_past_2_24():
    with pytest.raises(AssertionError, match="2\\^24"):
        CX.exact_acc(torch.zeros(1, 16384, 3, 3), torch.ones(1, 16384, 3, 3), 1, 1)
