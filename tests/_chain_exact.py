"""Float64 references, designed operands and an fp32 restatement of the summation tree for the two training chains of
csrc/train_chain.hip, shared by the tests (a plain module, not a conftest; plain torch on the CPU):

    FusedTrainPoolBnSign   [MaxPool2d(k, s)] -> BatchNorm (batch statistics) -> [Hardtanh] -> BinaryConnect
    FusedTrainBnActQuant   BatchNorm (batch statistics) [+ shortcut] -> ReLU -> nnDorefaQuant (identity STE)

References: the module chain itself in float64 (``sign_chain64`` / ``act_chain64``), as tests/test_gpu_r3.py evaluates it.

Designed operands (``designed_rows`` ...): per channel an integer mean m and deviations d 2^e with d = +-1 on 5R/8 of the rows and
+-3 on 3R/8, the signs in equal halves.  Then sum d = 0 and mean d^2 = 4: mean = m, var = 4^(e+1), and with an eps the sum absorbs
(DESIGNED_EPS) invstd = 2^-(e+1), xhat = d / 2 in {+-0.5, +-1.5}.  With dyadic gamma / beta, y = xhat gamma + beta lands EXACTLY on 0, on +-1
and beyond: the strictness of every mask is visible.  Every sum the kernels form is then a sum of integers on one grid below
2^24 of its units — exact in fp32 whatever the order — which ``proves_exact`` checks for the actual tensors before a test asks
for bit equality.

Gaussian operands (``gaussian_rows``): per-channel scales over six decades, every fourth channel offset by 32 sigma (a one-pass
variance E[x^2] - mean^2 loses (32)^2 = 2^10 of its 2^24 there), ``detie`` moves every element whose float64 value lies
within BAND of a decision boundary away from it, so signs, masks and codes are compared with nothing excluded.

``tree_stats``: the kernels' summation tree (16 lanes walking a slab sequentially, a 16-way fold, the per-slab partials folded
in double, float(s / R)) restated in fp32 torch — what correctly written fp32 arithmetic gives on an input, GPU or not."""
import copy
import math

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
STE_THRESHOLD = 1.001          # ops.STE_THRESHOLD (functions/binary_connect.py:37), restated
BAND = 5e-5                    # half-width of the band around a decision boundary that ``detie`` empties
NUDGE = 1e-3                   # ... by steps of NUDGE * sigma_c
# eps of the designed cases: torch's batch_norm refuses eps = 0; 2^-60 is absorbed by the addition in fp32 AND in float64
# (var >= 2^-2, half an ulp of it >= 2^-55), so var + eps == var and invstd = 2^-(e+1) exactly, as with eps = 0
DESIGNED_EPS = 2.0 ** -60
TC_TY = 16                     # rows in flight per workgroup (train_chain.hip), restated
TARGET_BLOCKS = 512

# (gamma, beta) of the designed channels, cycled over c % 4 (so the four lanes of a channel quad all differ):
#   (2, 0): y in {+-1, +-3}; (-2, 1): y in {0, 2, -2, 4}; (1, -0.5): y in {0, -1, 1, -2}; (0.5, 0.25): y in {0.5, 0, 1, -0.5}
DESIGNED_AFFINE = ((2.0, 0.0), (-2.0, 1.0), (1.0, -0.5), (0.5, 0.25))


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rows_plan(R: int):
    """(rows per workgroup, workgroups) of a chain launch over R rows: rows_per_block_for of train_chain.hip, restated."""
    R = int(R)
    rpb = max(TC_TY, -(-R // TARGET_BLOCKS))
    return rpb, -(-R // rpb)


def channel_class(C: int):
    """(256-channel chunks a workgroup walks, last chunk full, last 64-channel fold group full)."""
    return -(-int(C) // 256), C % 256 == 0, C % 64 == 0


def _dims(t):
    return (0, 2, 3) if t.dim() == 4 else (0,)


def _bc(v, t):
    """per-channel vector -> broadcastable against t (channel dimension 1)."""
    return v.reshape((1, -1) + (1,) * (t.dim() - 2))


def window_argmax(flat: torch.Tensor, W: int, k: int, s: int) -> torch.Tensor:
    """F.max_pool2d's flat indices (h W + w of the input plane) -> the kernels' window-local (h - ho s) k + (w - wo s)."""
    Ho, Wo = int(flat.shape[-2]), int(flat.shape[-1])
    h, w = torch.div(flat, W, rounding_mode="floor"), flat % W
    ho = torch.arange(Ho).reshape(-1, 1)
    wo = torch.arange(Wo).reshape(1, -1)
    return (h - ho * s) * k + (w - wo * s)


def covered_pixels(H: int, W: int, k: int, s: int) -> torch.Tensor:
    """bool [H, W]: the pixel lies in at least one pooling window (s > k, or a leftover row / column: some do not)."""
    Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
    m = torch.zeros((H, W), dtype=torch.bool)
    for ho in range(Ho):
        for wo in range(Wo):
            m[ho * s:ho * s + k, wo * s:wo * s + k] = True
    return m


# ---- float64 references: the module chain itself ----------------------------------------------------------------------------------

def _bn64(bn):
    return copy.deepcopy(bn).cpu().double().train()


def _stats(p, eps):
    d = _dims(p)
    mean = p.detach().mean(d)
    var = ((p.detach() - _bc(mean, p)) ** 2).mean(d)          # two passes: exact on the designed operands
    return mean, 1.0 / torch.sqrt(var + eps)


def sign_chain64(x, g, bn, pool=None, ht=None):
    """[MaxPool2d(*pool)] -> bn -> [Hardtanh(*ht)] -> BinaryConnect in float64 with autograd, on fp32 CPU tensors x (NCHW or
    [N, C]) and g (the upstream gradient, shaped like the output).  ``bn``: the BatchNorm module in the state BEFORE the step
    (copied; the copy — updated — is returned as "bn": pass it on for a second step).  Everything is float64, NCHW."""
    from pytorch_quantize_impls_amd.functions import BinaryConnect
    ref = _bn64(bn)
    lo, hi = ht if ht is not None else (-math.inf, math.inf)
    xr = x.detach().double().requires_grad_(True)
    out = {}
    if pool is not None:
        k, s = pool
        p, flat = F.max_pool2d(xr, k, s, return_indices=True)
        out["idx"] = window_argmax(flat, int(x.shape[3]), k, s)
    else:
        p = xr
    y = ref(p)
    y.retain_grad()
    h = torch.nn.Hardtanh(lo, hi)(y) if ht is not None else y
    sgn = BinaryConnect()(h)
    sgn.backward(g.detach().double())
    mean, invstd = _stats(p, ref.eps)
    xhat = (p.detach() - _bc(mean, p)) * _bc(invstd, p)
    yd, hd = y.detach(), h.detach()
    mask = (hd.abs() <= STE_THRESHOLD) & (yd > lo) & (yd < hi)
    g_y = y.grad
    out.update(p=p.detach(), mean=mean, invstd=invstd, xhat=xhat, y=yd, out=sgn.detach(), mask=mask, g_y=g_y, g_x=xr.grad,
               dgamma=(g_y * xhat).sum(_dims(p)), dbeta=g_y.sum(_dims(p)),
               abs_dgamma=(g_y * xhat).abs().sum(_dims(p)), abs_dbeta=g_y.abs().sum(_dims(p)),
               running_mean=ref.running_mean.clone(), running_var=ref.running_var.clone(), bn=ref)
    return out


def act_chain64(x, g, bn, res=None, relu=True, bits=4):
    """bn [+ res] [-> ReLU] [-> round(h n) / n, identity STE] in float64 with autograd (x, res, g: fp32 CPU tensors)."""
    ref = _bn64(bn)
    xr = x.detach().double().requires_grad_(True)
    rr = res.detach().double().requires_grad_(True) if res is not None else None
    y = ref(xr)
    t = y + rr if rr is not None else y
    t.retain_grad()
    a = torch.relu(t) if relu else t
    n = float((1 << bits) - 1) if bits else 0.0
    q = (torch.round(a * n) / n).detach() + (a - a.detach()) if bits else a
    q.backward(g.detach().double())
    mean, invstd = _stats(xr, ref.eps)
    xhat = (xr.detach() - _bc(mean, xr)) * _bc(invstd, xr)
    td = t.detach()
    g_t = t.grad
    return dict(p=xr.detach(), mean=mean, invstd=invstd, xhat=xhat, y=y.detach(), t=td, out=q.detach(),
                codes=torch.round(a.detach() * n) if bits else None, mask=(td > 0) if relu else torch.ones_like(td, dtype=torch.bool),
                g_y=g_t, g_x=xr.grad, g_res=rr.grad if rr is not None else None,
                dgamma=(g_t * xhat).sum(_dims(xr)), dbeta=g_t.sum(_dims(xr)),
                abs_dgamma=(g_t * xhat).abs().sum(_dims(xr)), abs_dbeta=g_t.abs().sum(_dims(xr)),
                running_mean=ref.running_mean.clone(), running_var=ref.running_var.clone(), bn=ref)


def grad_x_f32(p, g_y, mean, invstd, gamma, beta, dgamma, dbeta, R):
    """The kernels' last backward pass restated in fp32 torch, operation by operation (no contraction):
    ga is ((g_y - db invR) - (((p - mu) is) dg) invR), invR = float(1 / double(R)).  Arguments: float64 / fp32 tensors holding
    fp32 values (channel dimension 1; gamma None: 1).  Where g_y, dgamma and dbeta are the exact ones this is bit for bit what
    a correct kernel writes — in particular at the elements whose mask is 0 (g_y = 0), where BatchNorm's backward still leaves
    the batch terms."""
    f = lambda v: _bc(v.to(F32), p)
    pf, gy = p.to(F32), g_y.to(F32)
    invR = torch.tensor(1.0 / float(R), dtype=F64).to(F32)
    hx = (pf - f(mean)) * f(invstd)
    ga = f(gamma) if gamma is not None else torch.ones((), dtype=F32)
    return (ga * f(invstd)) * ((gy - f(dbeta) * invR) - (hx * f(dgamma)) * invR)


def channel_err(got, want, dim: int = 1):
    """per slice along ``dim``: max|got - want| / max|want| (a slice that is zero throughout: the absolute error)."""
    d = (got.detach().cpu().double() - want).abs().movedim(dim, 0).reshape(want.shape[dim], -1).amax(1)
    m = want.abs().movedim(dim, 0).reshape(want.shape[dim], -1).amax(1)
    return d / torch.where(m > 0, m, torch.ones_like(m))


# ---- designed operands --------------------------------------------------------------------------------------------------------

def designed_affine(C: int):
    """(gamma, beta) fp32 [C]: DESIGNED_AFFINE cycled over the channels."""
    ga = torch.tensor([DESIGNED_AFFINE[c % 4][0] for c in range(C)], dtype=F32)
    be = torch.tensor([DESIGNED_AFFINE[c % 4][1] for c in range(C)], dtype=F32)
    return ga, be


def designed_rows(R: int, C: int, seed: int, m_max: int = 6, e_range=(-2, 2)):
    """dict(p = fp32 [R, C] with p[r, c] = m_c + d[r, c] 2^(e_c), d, m, e, unit = 2^min(e, 0)): see the module docstring."""
    assert R % 16 == 0, "the deviation pattern needs R % 16 == 0"
    gen = _gen(seed)
    base = torch.cat([torch.full((5 * R // 16,), v) for v in (1.0, -1.0)] + [torch.full((3 * R // 16,), v) for v in (3.0, -3.0)])
    perm = torch.argsort(torch.rand((R, C), generator=gen), dim=0)
    d = base.to(F64)[perm]
    m = torch.randint(-m_max, m_max + 1, (C,), generator=gen).to(F64)
    e = torch.randint(e_range[0], e_range[1] + 1, (C,), generator=gen).to(F64)
    p = m + d * torch.pow(2.0, e)
    return dict(p=p.to(F32), d=d, m=m, e=e, unit=torch.pow(2.0, torch.clamp(e, max=0.0)), dev_unit=torch.pow(2.0, e))


def designed_cancelling_rows(R: int, C: int, seed: int, big: float = 4096.0):
    """designed_rows plus +big on the first half of the rows and -big on the second: the per-slab partial sums are +-2^23
    units with low bits set and cancel in the total — exact in double, not in an fp32 fold (32 partials per lane: 2^27).  The
    mean is still exactly m; the variance is not designed (compare it with a bar)."""
    D = designed_rows(R, C, seed, e_range=(-2, 0))
    half = torch.cat([torch.ones(R // 2), -torch.ones(R - R // 2)]).to(F64).reshape(-1, 1)
    D["p"] = (D["p"].to(F64) + big * half).to(F32)
    D["big"] = big
    return D


def designed_pool_input(N, C, H, W, k, seed):
    """(x fp32 [N, H, W, C], D): every k x k window of the stride-k pooling holds its prescribed value D["p"] (designed_rows over
    the N Ho Wo windows) at a seeded position and values smaller by 0, 1 or 2 grid steps elsewhere — ties included, the first
    in scan order is the argmax.  Pixels outside every window hold m + 64: they must not be pooled."""
    Ho, Wo = H // k, W // k
    D = designed_rows(N * Ho * Wo, C, seed)
    gen = _gen(seed + 1)
    step = torch.pow(2.0, D["e"])
    P = D["p"].to(F64).reshape(N, Ho, 1, Wo, 1, C)
    J = torch.randint(0, 3, (N, Ho, k, Wo, k, C), generator=gen).to(F64)
    pos = torch.randint(0, k * k, (N, Ho, 1, Wo, 1, C), generator=gen)
    at = (torch.arange(k).reshape(1, 1, k, 1, 1, 1) == pos // k) & (torch.arange(k).reshape(1, 1, 1, 1, k, 1) == pos % k)
    J[at] = 0.0
    x = (D["m"] + 64.0).expand(N, H, W, C).clone()
    x[:, :Ho * k, :Wo * k] = (P - J * step).reshape(N, Ho * k, Wo * k, C)
    return x.to(F32), D


def designed_residual(D, gamma, beta, seed, share: float = 0.125):
    """fp32 [R, C] dyadic shortcut: -y (so t = y + res is exactly 0) on ``share`` of the elements, a dyadic value elsewhere."""
    gen = _gen(seed)
    y = (D["d"] / 2.0) * gamma.to(F64) + beta.to(F64)
    zero = torch.rand(y.shape, generator=gen) < share
    other = torch.tensor([-1.0, -0.5, 0.5, 1.0, 1.5], dtype=F64)[torch.randint(0, 5, y.shape, generator=gen)]
    return torch.where(zero, -y, other).to(F32)


def designed_grad(shape, seed):
    """non-zero integers in [-8, 8], fp32: a wrong mask at any element changes g_y there by at least 1."""
    gen = _gen(seed)
    mag = torch.randint(1, 9, tuple(shape), generator=gen).to(F32)
    return torch.where(torch.rand(tuple(shape), generator=gen) < 0.5, -mag, mag)


def balanced_grad(mask, d, seed):
    """Integers in [-8, 8] (fp32, shaped like ``mask``; channel dimension 1) whose sum over the un-masked elements of every
    (channel, deviation value) group is 0: then dbeta = sum g_y = 0 and dgamma = sum g_y xhat = 0 exactly, BatchNorm's backward
    has no batch terms left, g_x = gamma invstd g_y — exactly 0 wherever the mask is 0.  Un-masked elements are paired inside
    their group (+a, -a; an odd one out gets 0); masked elements get non-zero values, which must not show anywhere."""
    gen = _gen(seed)
    C = mask.shape[1]
    m = mask.movedim(1, -1).reshape(-1, C)
    dv = d.movedim(1, -1).reshape(-1, C) if d.dim() == mask.dim() else d
    mag = torch.randint(1, 9, m.shape, generator=gen).to(F32)
    g = torch.where(torch.rand(m.shape, generator=gen) < 0.5, -mag, mag)          # the masked elements keep these
    key = (torch.arange(C).reshape(1, -1) * 8 + (dv.to(torch.int64) + 3)).masked_fill(~m, -1).reshape(-1)
    order = torch.argsort(key, stable=True)
    ks = key[order]
    first = torch.searchsorted(ks, ks, right=False)
    last = torch.searchsorted(ks, ks, right=True) - 1
    pos = torch.arange(ks.numel())
    rank = pos - first
    ms = mag.reshape(-1)[order]
    lead = (rank % 2 == 0)
    val = torch.where(lead, torch.where(pos < last, ms, torch.zeros(())), -ms[(pos - 1).clamp(min=0)])
    flat = g.reshape(-1).clone()
    live = ks >= 0
    flat[order[live]] = val[live]
    out = flat.reshape(m.shape)
    return out.reshape(mask.movedim(1, -1).shape).movedim(-1, 1) if mask.dim() > 2 else out


def _is_f32(v):
    return bool(torch.equal(v.to(F32).to(F64), v.to(F64)))


def proves_exact(ref, unit, gamma=None, beta=None, res=None, slab_rows=None, variance=True, dev_unit=None):
    """(ok, why): every quantity the kernels form on these operands is exact in fp32, whatever the summation order.  ``ref``: the
    float64 reference dict (p, mean, invstd, xhat, y, g_y; channel dimension 1), ``unit`` [C]: the grid of p per channel,
    ``dev_unit`` [C]: that of p - mean (2^e: a common power of two scales a sum without touching its exactness).
    Checked: p on the grid and sum|p| below 2^24 units (it bounds every partial sum; with ``slab_rows`` the bound is asked of each
    slab of that many rows only — the slabs' partials are folded in double), mean an fp32 value, (p - mean)^2 on the grid of
    unit^2 with a sum below 2^24, invstd / xhat / y / t fp32 values, g_y integers with sum|g_y| < 2^24, g_y xhat on the grid of
    1/2 with sum below 2^24 of them."""
    lim = float(1 << 24)
    p, C = ref["p"], int(ref["p"].shape[1])
    rows = p.movedim(1, -1).reshape(-1, C)
    u = unit.to(F64)

    def total(v):            # [R, C] non-negative -> the largest sum any workgroup (or the whole launch) can see
        if slab_rows is None:
            return v.sum(0)
        pad = (-v.shape[0]) % slab_rows
        return F.pad(v, (0, 0, 0, pad)).reshape(-1, slab_rows, C).sum(1).amax(0)

    q = rows / u
    if not torch.equal(q, torch.round(q)):
        return False, "p is not on its grid"
    if float(total(q.abs()).max()) >= lim:
        return False, f"sum|p| reaches {float(total(q.abs()).max()):.3g} units (>= 2^24)"
    if not _is_f32(ref["mean"]):
        return False, "the mean is not an fp32 value"
    if variance:
        dev2 = ((rows - ref["mean"]) / (dev_unit.to(F64) if dev_unit is not None else u)) ** 2
        if not torch.equal(dev2, torch.round(dev2)) or float(total(dev2).max()) >= lim:
            return False, "sum (p - mean)^2 is off its grid or reaches 2^24 units"
        for name in ("invstd", "xhat", "y"):
            if not _is_f32(ref[name]):
                return False, f"{name} is not an fp32 value"
        if gamma is not None and not _is_f32(ref["xhat"] * _bc(gamma.to(F64), ref["xhat"])):
            return False, "xhat gamma is not an fp32 value"
        if res is not None and not _is_f32(ref["t"]):
            return False, "t = y + res is not an fp32 value"
        gy = ref["g_y"].movedim(1, -1).reshape(-1, C)
        if not torch.equal(gy, torch.round(gy)) or float(total(gy.abs()).max()) >= lim:
            return False, "g_y is not integer or sum|g_y| reaches 2^24"
        gx = gy * ref["xhat"].movedim(1, -1).reshape(-1, C) * 2.0
        if not torch.equal(gx, torch.round(gx)) or float(total(gx.abs()).max()) >= lim:
            return False, "g_y xhat is off the grid of 1/2 or its sum reaches 2^24 halves"
    return True, ""


# ---- Gaussian operands --------------------------------------------------------------------------------------------------------

OFFSET_SIGMAS = 32.0


def gaussian_rows(R: int, C: int, seed: int, offset: float = OFFSET_SIGMAS):
    """(x fp32 [R, C], sigma [C] float64): sigma_c log-spaced over 1e-3 .. 1e3 (shuffled), channels c % 4 == 1 offset by
    ``offset`` sigma."""
    gen = _gen(seed)
    sigma = torch.pow(10.0, torch.linspace(-3.0, 3.0, C, dtype=F64))[torch.randperm(C, generator=gen)] if C > 1 else torch.ones(1, dtype=F64)
    z = torch.randn((R, C), generator=gen, dtype=F64)
    off = torch.where(torch.arange(C) % 4 == 1, offset, 0.0).to(F64)
    return ((z + off) * sigma).to(F32), sigma


def gaussian_affine(C: int, seed: int):
    """(gamma, beta) fp32 [C]: |gamma| in [0.5, 1], every third negative; beta ~ 0.3 N(0, 1)."""
    gen = _gen(seed)
    ga = torch.rand((C,), generator=gen) * 0.5 + 0.5
    ga[::3] *= -1.0
    return ga.to(F32), (torch.randn((C,), generator=gen) * 0.3).to(F32)


def boundary_distance(t, boundaries=(), levels: float = 0.0):
    """signed distance (float64, in units of t) of every element to its nearest decision boundary: the scalars ``boundaries``
    and, with ``levels`` = n, the half-integers of n t (the quantiser's rounding boundaries; distance measured in t)."""
    best = torch.full_like(t, math.inf)
    for b in boundaries:
        if math.isfinite(b):
            d = t - b
            best = torch.where(d.abs() < best.abs(), d, best)
    if levels:
        u = t * levels
        d = (u - torch.floor(u) - 0.5) / levels
        best = torch.where(d.abs() < best.abs(), d, best)
    return best


def detie(x, sigma, gamma, beta, eps, boundaries=(), levels=0.0, pool=None, res=None, rounds: int = 3):
    """x (fp32 CPU, NCHW or [N, C]) with every element whose float64 chain value t = BatchNorm(pool(x)) [+ res] lies within BAND
    of a decision boundary moved away from it by NUDGE sigma_c (pooled inputs: the window's maximum is moved UPWARD, so the
    argmax stays); the statistics move with the data, so the pass is repeated, ``rounds`` times at most.  Asserts that
    afterwards no element is inside the band.  Returns (x, elements moved)."""
    x = x.clone()
    ga = gamma.to(F64) if gamma is not None else torch.ones(x.shape[1], dtype=F64)
    be = beta.to(F64) if beta is not None else torch.zeros(x.shape[1], dtype=F64)
    moved = 0
    for it in range(rounds + 1):
        x64 = x.to(F64)
        if pool is not None:
            p, flat = F.max_pool2d(x64, pool[0], pool[1], return_indices=True)
        else:
            p = x64
        mean, invstd = _stats(p, eps)
        t = (p - _bc(mean, p)) * _bc(invstd, p) * _bc(ga, p) + _bc(be, p)
        if res is not None:
            t = t + res.to(F64)
        d = boundary_distance(t, boundaries, levels)
        inside = d.abs() < BAND
        n_in = int(inside.sum())
        if n_in == 0:
            return x, moved
        assert it < rounds, f"detie: {n_in} elements are still within {BAND} of a boundary after {rounds} rounds"
        moved += n_in
        step = _bc(sigma.to(F64) * NUDGE, p)
        if pool is not None:
            N, C, H, W = x.shape
            upd = torch.zeros((N, C, H * W), dtype=F64)
            upd.scatter_reduce_(2, flat.reshape(N, C, -1), (inside.to(F64) * step).reshape(N, C, -1), "amax")
            x = (x64 + upd.reshape(N, C, H, W)).to(F32)
        else:
            direction = torch.where(d >= 0, 1.0, -1.0) * _bc(torch.where(ga >= 0, 1.0, -1.0), p)
            x = (x64 + inside.to(F64) * direction * step).to(F32)
    raise AssertionError("unreachable")


# ---- the kernels' summation tree in fp32 ------------------------------------------------------------------------------------------

def tree_sum(v: torch.Tensor) -> torch.Tensor:
    """float64 [C]: sum over the rows of fp32 v [R, C] as a chain launch forms it — per slab (rows_plan) 16 lanes each adding
    its rows r0 + y, r0 + y + 16, ... sequentially in fp32, the 16 lane sums added in lane order, the slabs' partials in double."""
    R, C = v.shape
    rpb, nblk = rows_plan(R)
    steps = -(-rpb // TC_TY)
    pad = torch.zeros((nblk * rpb, C), dtype=F32)
    pad[:R] = v
    lanes = F.pad(pad.reshape(nblk, rpb, C), (0, 0, 0, steps * TC_TY - rpb)).reshape(nblk, steps, TC_TY, C)
    acc = torch.zeros((nblk, TC_TY, C), dtype=F32)
    for st in range(steps):
        acc = acc + lanes[:, st]
    part = acc[:, 0]
    for y in range(1, TC_TY):
        part = part + acc[:, y]
    # fold_partials: lane y adds the partials y, y + 16, ... in double, then the 16 lane sums in lane order
    rounds = -(-nblk // TC_TY)
    pd = F.pad(part.to(F64), (0, 0, 0, rounds * TC_TY - nblk)).reshape(rounds, TC_TY, C)
    lane = torch.zeros((TC_TY, C), dtype=F64)
    for b in range(rounds):
        lane = lane + pd[b]
    s = torch.zeros((C,), dtype=F64)
    for y in range(TC_TY):
        s = s + lane[y]
    return s


def tree_stats(p: torch.Tensor, eps: float, one_pass: bool = False):
    """(mean, invstd) fp32 [C] of fp32 p [R, C] as the statistics launches form them, operation by operation — the mean is
    the device's bit for bit, so a test that compares them pins the slab plan, the lane stride and the fold order:
    mean = float(tree_sum(p) * (1 / R)), then
    var = float(tree_sum((p - mean)^2) / R) (two passes), invstd = 1 / sqrtf(var + eps).  ``one_pass``: the variance as
    E[x^2] - mean^2 from the same tree instead — what the two passes are there to avoid."""
    R = p.shape[0]
    s1 = tree_sum(p)
    mean = (s1 * (1.0 / R)).to(F32)           # fold_kernel: float(s * scale), scale = 1.0 / double(R)
    if one_pass:
        var = (tree_sum(p * p) / R).to(F32) - mean * mean
    else:
        dx = p - mean
        var = (tree_sum(dx * dx) / R).to(F32)
    return mean, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
