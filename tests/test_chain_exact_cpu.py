"""tests/_chain_exact.py checked against itself and against torch on the CPU: the designed operands are what they claim (exact
statistics, values exactly on every mask boundary, ``proves_exact`` accepts them and rejects an over-range case), ``rows_plan``
gives the slab regimes the GPU module names, ``detie`` empties the band, the window-local argmax follows torch on ties, NaN
and +-inf — and the fp32 restatement of the kernels' summation tree meets the GPU module's bars on the Gaussian operands
while a one-pass variance on the same data does not."""
import math

import pytest
import torch
import torch.nn.functional as F

import _chain_exact as X

F64, F32 = torch.float64, torch.float32


def _bn(C, gamma, beta, eps, momentum=0.25, two_d=True):
    bn = (torch.nn.BatchNorm2d if two_d else torch.nn.BatchNorm1d)(C, eps=eps, momentum=momentum, affine=gamma is not None)
    if gamma is not None:
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    return bn


@pytest.mark.parametrize("R,plan,last", [(48, (16, 3), 16), (8192, (16, 512), 16), (8448, (17, 497), 16),
                                         (186624, (365, 512), 109), (262144, (512, 512), 512),
                                         (43264, (85, 509), 84), (9216, (18, 512), 18), (256, (16, 16), 16),
                                         (65536, (128, 512), 128), (16384, (32, 512), 32), (4096, (16, 256), 16)])
def test_rows_plan_gives_the_slab_regimes_the_gpu_module_names(R, plan, last):
    rpb, nblk = X.rows_plan(R)
    assert (rpb, nblk) == plan
    assert R - (nblk - 1) * rpb == last and (nblk - 1) * rpb < R <= nblk * rpb


def test_channel_classes():
    assert X.channel_class(4) == (1, False, False) and X.channel_class(68) == (1, False, False)
    assert X.channel_class(256) == (1, True, True) and X.channel_class(260) == (2, False, False)
    assert X.channel_class(192) == (1, False, True) and X.channel_class(768) == (3, True, True)


@pytest.mark.parametrize("R,C", [(48, 8), (8448, 68), (186624, 8)])
def test_designed_rows_have_exact_statistics_and_sit_on_every_boundary(R, C):
    D = X.designed_rows(R, C, seed=R + C)
    ga, be = X.designed_affine(C)
    g = X.designed_grad((R, C), 3)
    ref = X.sign_chain64(D["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False), ht=(-1.0, 1.0))
    assert torch.equal(ref["mean"], D["m"])                                       # bit for bit, in float64
    assert torch.equal(ref["invstd"], torch.pow(2.0, -(D["e"] + 1.0)))
    assert torch.equal(ref["xhat"], D["d"] / 2.0)
    assert set(ref["xhat"].unique().tolist()) == {-1.5, -0.5, 0.5, 1.5}
    y = ref["y"]
    for c, want in ((0, {-3.0, -1.0, 1.0, 3.0}), (1, {-2.0, 0.0, 2.0, 4.0}), (2, {-2.0, -1.0, 0.0, 1.0}), (3, {-0.5, 0.0, 0.5, 1.0})):
        assert set(y[:, c].unique().tolist()) == want
    # y == 0 -> +1; y == +-1: Hardtanh's mask is strict, the gradient stops
    assert bool((ref["out"][y == 0] == 1.0).all()) and bool((ref["out"][y < 0] == -1.0).all())
    assert not bool(ref["mask"][y.abs() >= 1.0].any()) and bool(ref["mask"][y.abs() < 1.0].all())
    assert torch.equal(ref["g_y"], torch.where(ref["mask"], g.double(), 0.0))      # autograd agrees with the stated mask
    assert torch.equal(ref["dgamma"], ref["bn"].weight.grad) and torch.equal(ref["dbeta"], ref["bn"].bias.grad)
    assert torch.equal(ref["running_mean"], 0.25 * D["m"])
    ok, why = X.proves_exact(ref, D["unit"], ga, be, dev_unit=D["dev_unit"])
    assert ok, why
    # without Hardtanh the STE alone masks: |y| <= 1.001 passes, so y == +-1 now carries gradient
    ref2 = X.sign_chain64(D["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False))
    assert bool(ref2["mask"][y.abs() <= 1.0].all()) and not bool(ref2["mask"][y.abs() > 1.0].any())
    # Hardtanh(-0.5, 2): y == -0.5 and y == 2 sit on its (strict) ends
    ref3 = X.sign_chain64(D["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False), ht=(-0.5, 2.0))
    assert bool((y == -0.5).any()) and bool((y == 2.0).any())
    assert not bool(ref3["mask"][(y == -0.5) | (y == 2.0)].any()) and bool(ref3["mask"][(y > -0.5) & (y <= 1.0)].all())


def test_proves_exact_rejects_sums_beyond_fp32():
    R, C = 262144, 4
    ga, be = X.designed_affine(C)
    g = X.designed_grad((R, C), 1)
    D = X.designed_rows(R, C, seed=2)
    assert X.proves_exact(X.sign_chain64(D["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False)), D["unit"], ga, be, dev_unit=D["dev_unit"])[0]
    big = X.designed_rows(R, C, seed=2, m_max=100)
    big["p"][:, 0] += 100.0 - big["m"][0].float()                                 # channel 0: mean exactly 100
    ok, why = X.proves_exact(X.sign_chain64(big["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False)), big["unit"], ga, be, dev_unit=big["dev_unit"])
    assert not ok and "2^24" in why
    off = D["p"].clone()
    off[5, 1] += 2.0 ** -9                                                        # one element off the grid
    ok, why = X.proves_exact(X.sign_chain64(off, g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False)), D["unit"], ga, be, dev_unit=D["dev_unit"])
    assert not ok


def test_cancelling_rows_are_exact_per_slab_and_break_an_fp32_fold():
    R, C = 262144, 8
    D = X.designed_cancelling_rows(R, C, seed=4)
    p = D["p"]
    assert torch.equal(p.double().mean(0), D["m"])
    ref = dict(p=p.double(), mean=D["m"])
    rpb, nblk = X.rows_plan(R)
    ok, why = X.proves_exact(ref, D["unit"], slab_rows=rpb, variance=False)
    assert ok, why
    assert not X.proves_exact(ref, D["unit"], variance=False)[0]                  # the whole-launch bound does NOT hold: by design
    # the tree with its double fold gives the mean exactly; the same partials folded in fp32 (32 per lane, then the lanes) do not
    mean, _ = X.tree_stats(p, 0.0)
    assert torch.equal(mean.double(), D["m"])
    part = p.reshape(nblk, rpb, C).double().sum(1).float()                        # the slabs' partials: exact fp32 values
    assert torch.equal(part.double(), p.reshape(nblk, rpb, C).double().sum(1))
    lane = torch.zeros((16, C), dtype=F32)
    for b in range(nblk // 16):
        lane = lane + part[16 * b:16 * b + 16]
    s = lane[0]
    for y_ in range(1, 16):
        s = s + lane[y_]
    assert not torch.equal((s.double() / R).float().double(), D["m"])


def test_designed_pool_input_pools_to_the_prescribed_values_with_ties():
    N, C, H, W, k = 4, 12, 9, 11, 2
    x, D = X.designed_pool_input(N, C, H, W, k, seed=7)
    xn = x.permute(0, 3, 1, 2)
    p, flat = F.max_pool2d(xn.double(), k, k, return_indices=True)
    assert torch.equal(p.permute(0, 2, 3, 1).reshape(-1, C), D["p"].double())
    win = F.unfold(xn.double().reshape(N * C, 1, H, W), k, stride=k)              # [N C, k k, L]
    ties = (win == win.amax(1, keepdim=True)).sum(1)
    assert int((ties > 1).sum()) > 0.2 * ties.numel()                             # equal maxima are common
    idx = X.window_argmax(flat, W, k, k)
    assert int(idx.min()) == 0 and int(idx.max()) == k * k - 1
    is_max = win == win.amax(1, keepdim=True)
    first = (is_max & (is_max.cumsum(1) == 1)).int().argmax(1)                    # the one position that is the FIRST maximum
    assert torch.equal(idx.reshape(N * C, -1), first)
    assert bool((xn[:, :, 8, :] > p.amax()).all()) and bool((xn[:, :, :, 10] > p.amax()).all())   # leftovers would win if pooled


def test_designed_residual_puts_t_exactly_on_zero():
    R, C = 8448, 8
    D = X.designed_rows(R, C, seed=9)
    ga, be = X.designed_affine(C)
    res = X.designed_residual(D, ga, be, seed=10, share=0.125)
    g = X.designed_grad((R, C), 11)
    ref = X.act_chain64(D["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False), res=res, relu=True, bits=4)
    share = float((ref["t"] == 0).double().mean())
    assert 0.125 - 0.01 <= share <= 0.35, share
    assert not bool(ref["mask"][ref["t"] == 0].any())                              # ReLU's mask is strict
    assert torch.equal(ref["g_res"], torch.where(ref["t"] > 0, g.double(), 0.0))
    assert float(ref["codes"].abs().max()) <= 127
    half = (ref["t"].clamp(min=0) * 15.0 % 1.0) == 0.5
    assert bool(half.any())                                                        # codes on rounding ties: round-half-even both sides
    ok, why = X.proves_exact(ref, D["unit"], ga, be, res=res, dev_unit=D["dev_unit"])
    assert ok, why


def test_argmax_convention_on_ties_nan_and_inf():
    """The first maximum in scan order wins; a NaN wins over everything and a later NaN over an earlier one; a window of -inf
    keeps its first position: F.max_pool2d(return_indices=True), which the kernels follow."""
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 1, 1] = 2.0
    x[0, 0, 1, 2] = 2.0                       # tie inside window (0, 0) of a 3 / 2 pooling: (1, 1) comes first
    x[0, 0, 2, 4] = math.nan
    x[0, 0, 4, 4] = math.nan                  # window (1, 1) sees both: the later one is reported
    x[0, 0, 2:5, 0:3] = -math.inf             # window (1, 0) is all -inf
    x[0, 0, 2, 2] = 2.0                       # ... but for this one, also in (0, 0): third equal maximum
    p, flat = F.max_pool2d(x, 3, 2, return_indices=True)
    idx = X.window_argmax(flat, 5, 3, 2)
    assert idx.tolist() == [[[[4, 8], [2, 8]]]]
    assert float(p[0, 0, 0, 0]) == 2.0 and math.isnan(float(p[0, 0, 0, 1])) and math.isnan(float(p[0, 0, 1, 1]))
    x[0, 0, 2, 2] = -math.inf
    p, flat = F.max_pool2d(x, 3, 2, return_indices=True)
    assert float(p[0, 0, 1, 0]) == -math.inf and int(X.window_argmax(flat, 5, 3, 2)[0, 0, 1, 0]) == 0
    cov = X.covered_pixels(8, 11, 2, 3)
    assert cov.sum() == 3 * 4 * 4 and not bool(cov[2].any()) and not bool(cov[:, 2].any()) and bool(cov[7, 10])


@pytest.mark.parametrize("pool", [None, (3, 2)])
def test_detie_empties_the_band_for_the_sign_chain(pool):
    N, C, H = 6, 12, 13
    x, sigma = X.gaussian_rows(N * H * H, C, seed=21)
    x = x.reshape(N, H, H, C).permute(0, 3, 1, 2).contiguous()
    ga, be = X.gaussian_affine(C, 22)
    bounds = (0.0, -1.0, 1.0)
    x0 = x.clone()
    x, moved = X.detie(x, sigma, ga, be, 1e-4, boundaries=bounds, pool=pool)
    g = torch.randn((N, C) + ((H, H) if pool is None else (6, 6)), generator=X._gen(23))
    ref = X.sign_chain64(x, g, _bn(C, ga, be, 1e-4), pool=pool, ht=(-1.0, 1.0))
    assert float(X.boundary_distance(ref["y"], bounds).abs().min()) >= X.BAND
    changed = x != x0
    assert int(changed.sum()) <= 3 * max(moved, 1)
    if moved:
        rel = ((x - x0).abs() / sigma.float().reshape(1, -1, 1, 1))[changed]
        assert float(rel.max()) <= 3.5 * X.NUDGE
    if pool is not None:      # the maxima moved upward: nothing else did
        assert bool((x >= x0).all())


def test_detie_empties_the_band_for_the_quantiser_chain():
    R, C = 4096, 16
    x, sigma = X.gaussian_rows(R, C, seed=31)
    ga, be = X.gaussian_affine(C, 32)
    res = (torch.randn((R, C), generator=X._gen(33)) * 0.5)
    x, moved = X.detie(x, sigma, ga, be, 1e-4, boundaries=(0.0,), levels=15.0, res=res)
    assert moved > 0
    ref = X.act_chain64(x, torch.ones(R, C), _bn(C, ga, be, 1e-4, two_d=False), res=res, relu=True, bits=4)
    assert float(X.boundary_distance(ref["t"], (0.0,), 15.0).abs().min()) >= X.BAND


@pytest.mark.parametrize("R", [262144, 186624, 8432])
def test_fp32_tree_meets_the_bars_and_a_one_pass_variance_does_not(R):
    """Bars of tests/test_gpu_train_chain_b256.py on the Gaussian operands (six decades, every fourth channel at 32 sigma):
    running statistics within 1e-6 per channel.  The two-pass tree in fp32 meets them with room (invstd to ~1e-7, the mean to
    half an ulp of the offset, 32 sigma 2^-24 ~ 2e-6 sigma); float(E[x^2]) - mean^2 from the same tree rounds 1025 sigma^2 to
    fp32 before it subtracts 1024 sigma^2 — up to 6e-5 of the variance — and misses on the offset channels."""
    C, eps = 32, 1e-4
    x, sigma = X.gaussian_rows(R, C, seed=R)
    x64 = x.double()
    mean64, var64 = x64.mean(0), x64.var(0, unbiased=False)
    invstd64 = 1.0 / torch.sqrt(var64 + eps)
    off = torch.arange(C) % 4 == 1
    big = sigma >= 1.0                        # below, eps = 1e-4 dominates var + eps and hides the variance's error
    mean, invstd = X.tree_stats(x, eps)
    e_mean = (mean.double() - mean64).abs() / sigma
    e_inv = (invstd.double() - invstd64).abs() / invstd64
    print(f"R={R}: two-pass mean err {float(e_mean.max()):.2e} sigma, invstd rel err {float(e_inv.max()):.2e}")
    assert float(e_mean.max()) <= 4e-6 and float(e_inv.max()) <= 1e-6
    # the bars as the GPU module states them: |running_mean err| <= 1e-6 mean|x|, |running_var err| <= 1e-6 running_var
    assert bool(((mean.double() - mean64).abs() <= 1e-6 * x64.abs().mean(0)).all())
    var32 = 1.0 / invstd.double() ** 2 - eps
    assert bool(((var32 - var64).abs()[big] <= 1e-6 * var64[big]).all())
    _, inv1 = X.tree_stats(x, eps, one_pass=True)
    e1 = (inv1.double() - invstd64).abs() / invstd64
    print(f"R={R}: one-pass invstd rel err on the offset channels {e1[off & big].tolist()}")
    assert float(e1[off & big].max()) > 1e-5 and float(e1[~off].max()) <= 1e-6
    # almost no element of y is small enough for its RELATIVE error to matter at 1e-5 of the channel's scale
    y = (x64 - mean64) * invstd64
    assert float((y.abs() < 1e-5 * y.abs().mean()).double().mean()) <= 1e-4


def test_grad_x_f32_restates_batchnorm_backward():
    R, C = 8448, 8
    D = X.designed_rows(R, C, seed=41)
    ga, be = X.designed_affine(C)
    g = X.designed_grad((R, C), 42)
    ref = X.sign_chain64(D["p"], g, _bn(C, ga, be, X.DESIGNED_EPS, two_d=False), ht=(-1.0, 1.0))
    gx = X.grad_x_f32(ref["p"], ref["g_y"], ref["mean"], ref["invstd"], ga, be, ref["dgamma"], ref["dbeta"], R)
    assert gx.dtype == F32
    assert float(X.channel_err(gx, ref["g_x"]).max()) <= 1e-6
    assert not bool(ref["g_x"][:, 0].any())       # gamma 2, beta 0 under Hardtanh: y in {+-1, +-3}, every element masked
    # where the mask is 0 the gradient is NOT 0: the batch terms remain (and only they)
    dead = ~ref["mask"]
    assert bool(dead.any()) and bool((ref["g_x"][dead] != 0).any())


def test_balanced_grad_cancels_the_batch_terms_exactly():
    R, C = 8448, 8
    D = X.designed_rows(R, C, seed=51)
    ga, be = X.designed_affine(C)
    bn = _bn(C, ga, be, X.DESIGNED_EPS, two_d=False)
    mask = X.sign_chain64(D["p"], torch.ones(R, C), bn, ht=(-1.0, 1.0))["mask"]
    g = X.balanced_grad(mask, D["d"], seed=52)
    assert float(g.abs().max()) <= 8 and bool((g == torch.round(g)).all()) and bool((g[~mask] != 0).all())
    ref = X.sign_chain64(D["p"], g, bn, ht=(-1.0, 1.0))
    assert not bool(ref["dgamma"].any()) and not bool(ref["dbeta"].any()) and float(ref["abs_dgamma"].max()) > 0
    assert not bool(ref["g_x"][~mask].any()) and bool(ref["g_x"][mask].any())
    assert torch.equal(ref["g_x"], ref["g_y"] * ga.double() * ref["invstd"])
    x4 = D["p"].reshape(33, 16, 16, C).permute(0, 3, 1, 2)                         # the same through a 4-D layout
    bn4 = _bn(C, ga, be, X.DESIGNED_EPS)
    m4 = X.sign_chain64(x4, torch.ones(33, C, 16, 16), bn4)["mask"]
    g4 = X.balanced_grad(m4, D["d"].reshape(33, 16, 16, C).permute(0, 3, 1, 2), seed=53)
    r4 = X.sign_chain64(x4, g4, bn4)
    assert g4.shape == x4.shape and not bool(r4["dgamma"].any()) and not bool(r4["dbeta"].any())
