"""Independent reference for the depthwise convs on int8 code planes (include/qt_hip.h "Depthwise convolution on int8 code
planes"), shared by tests/test_dw_codes_cpu.py and tests/test_gpu_dw_codes.py.  Nothing of the package's packers or kernels is used:

* codes come from ``_codes_exact.random_codes`` (or are written by hand),
* the image is ``float32(inv_n) * q`` in numpy float32 (one rounding: what the kernel's decode forms),
* the conv value comes from ``_dw_exact.forward`` in float32, which reproduces qt_dwconv2d_f32 bit for bit,
* the epilogue is ``_codes_exact.epilogue`` with an ``Epi`` without a residual,
* planes are encoded / decoded with ``_codes_exact.encode_plane`` / ``decode_plane`` / ``check_plane_zeros``.

``CASES`` is the list the GPU file walks; ``build(i)`` its operands and reference (computed once per process).  The seeds are part
of the list: for each of them the reference's own count of sensitive elements (``_codes_exact.sensitive``) is zero, which the CPU
file asserts, so the GPU comparison waives nothing."""
import functools

import numpy as np
import torch

import _codes_exact as C
import _dw_exact as D

#            kernel  stride  padding dilation      (the seven geometries of tests/test_gpu_dwconv_chain.py)
GEOMS = (((3, 3), (1, 1), (1, 1), (1, 1)),
         ((3, 3), (2, 2), (1, 1), (1, 1)),
         ((5, 5), (1, 1), (2, 2), (1, 1)),
         ((1, 1), (1, 1), (0, 0), (1, 1)),
         ((7, 7), (1, 1), (3, 3), (1, 1)),        # 49 taps
         ((2, 3), (1, 1), (0, 0), (1, 1)),        # the generic tap form
         ((3, 1), (2, 1), (1, 0), (2, 1)))
CM = ((3, 1), (4, 1), (16, 1), (36, 1), (20, 2), (132, 1))       # partial dword, exact 16-byte rows, ld padding, m > 1, > 128 channels
MAPS = ((7, 7), (9, 8), (14, 14), (5, 17))
BATCHES = (1, 3)
HALOS = ((0, 0), (1, 1), (2, 1))
BITS = (2, 4, 8)
TAPS = ("pm_e", "grid3", "gauss")
FORMS = ("device", "folded")


class Case(dict):
    __getattr__ = dict.__getitem__


def _case(i):
    (Cc, m), (H, W) = CM[i % len(CM)], MAPS[i % len(MAPS)]
    k, s, p, d = GEOMS[i % len(GEOMS)]
    N = BATCHES[(i // 2) % 2]
    c = Case(i=i, C=Cc, m=m, H=H, W=W, N=N, kernel=k, stride=s, padding=p, dilation=d,
             in_halo=HALOS[i % 3], out_halo=HALOS[(i // 3 + i) % 3], in_bits=BITS[i % 3], out_bits=BITS[(i // 2) % 3],
             relu=(i % 4) < 2, form=FORMS[i % 2], bias=(i % 3) != 1, taps=TAPS[(i // 2) % 3], seed=4000 + 17 * i)
    c["id"] = (f"C{Cc}m{m}N{N}-k{k[0]}x{k[1]}-s{s[0]}{s[1]}-p{p[0]}{p[1]}-d{d[0]}-{H}x{W}-ih{c.in_halo[0]}{c.in_halo[1]}"
               f"-oh{c.out_halo[0]}{c.out_halo[1]}-a{c.in_bits}to{c.out_bits}-{c.form}-{c.taps}")
    return c


# every geometry twice, with another (C, m), map, batch, halo pair, bit widths, BatchNorm form and tap family
CASES = [_case(i) for i in range(2 * len(GEOMS))]


def geom(c):
    return c.kernel, c.stride, c.padding, c.dilation


def inv_levels(bits: int) -> np.float32:
    """fl32(1 / (2^k - 1)): a float32 division, as the quantiser forms it."""
    return np.float32(1.0) / np.float32((1 << int(bits)) - 1)


def code_range(bits: int):
    """Codes a k-bit activation holds in int8: 0 .. 2^k - 1 behind a ReLU; the unclamped 8-bit quantiser also gives negatives."""
    return (0, (1 << bits) - 1) if bits < 8 else (-100, 127)


def image(q: np.ndarray, inv_n) -> np.ndarray:
    """float32(inv_n) * q in numpy float32: the decode of the kernels, one rounding."""
    x = np.float32(inv_n) * q.astype(np.float32)
    assert x.dtype == np.float32
    return x


def taps(kind: str, seed: int, shape) -> np.ndarray:
    """[C m, kh, kw] float32 taps: +-E of a 1-bit DoReFa weight, the level image (2 q - 7) / 7 of a 3-bit one, or Gaussian."""
    r = np.random.RandomState(seed)
    if kind == "pm_e":
        return (np.where(r.rand(*shape) < 0.5, -1.0, 1.0) * np.float32(0.3712)).astype(np.float32)
    if kind == "grid3":
        return ((2.0 * r.randint(0, 8, size=shape) - 7.0).astype(np.float32) / np.float32(7.0)).astype(np.float32)
    return (r.randn(*shape) * 0.5).astype(np.float32)


def bn_params(Cout: int, kk: int, levels: float, seed: int, form: str):
    """BatchNorm statistics sized for the conv's spread, every third weight negative, scaled so that levels * t stays inside int8
    for all but far outliers.  Device form: (weight, bias, (mean, rs)); folded: (alpha, beta, None), each rounded once."""
    g = torch.Generator().manual_seed(seed)
    spread = 0.35 * kk ** 0.5 + 0.05
    mean = torch.randn(Cout, generator=g) * 0.5 * spread
    var = (torch.rand(Cout, generator=g) * 1.5 + 0.5) * spread * spread
    w = (torch.rand(Cout, generator=g) + 0.5) * min(1.0, 30.0 / levels)
    w[::3] *= -1
    b = torch.randn(Cout, generator=g) * 0.3 * min(1.0, 30.0 / levels)
    rs = (1.0 / torch.sqrt(var.double() + 1e-5)).float()
    if form == "device":
        return w, b, (mean, rs)
    alpha = w * rs
    return alpha, b - mean * alpha, None


def reference(q: np.ndarray, inv_n, w: np.ndarray, bias, geometry, epi: C.Epi) -> dict:
    """``_codes_exact.epilogue`` of the depthwise conv of the image of ``q`` [N, C, H, W]; every tensor of the result is
    [N, Ho, Wo, C m] (channels last).  ``y`` (float32, NCHW) is added."""
    y = D.forward(image(q, inv_n), w, bias, *geometry)
    assert y.dtype == np.float32
    ref = C.epilogue(torch.from_numpy(np.ascontiguousarray(y.transpose(0, 2, 3, 1))), epi)
    ref["y"] = y
    return ref


def out_plane(ref: dict, halo) -> torch.Tensor:
    """The int8 output plane the kernel must write: the reference's codes with a zero border and zero pad bytes."""
    return C.encode_plane(ref["codes"].permute(0, 3, 1, 2), halo)


@functools.lru_cache(maxsize=None)
def build(i: int) -> Case:
    c = CASES[i]
    Cout = c.C * c.m
    lo, hi = code_range(c.in_bits)
    q = C.random_codes((c.N, c.C, c.H, c.W), lo, hi, c.seed, "cpu").numpy()
    w = taps(c.taps, c.seed + 1, (Cout,) + c.kernel)
    b = (np.random.RandomState(c.seed + 2).randn(Cout) * 0.2).astype(np.float32) if c.bias else None
    levels = float((1 << c.out_bits) - 1)
    alpha, beta, stats = bn_params(Cout, c.kernel[0] * c.kernel[1], levels, c.seed + 3, c.form)
    epi = C.Epi(alpha=alpha, beta=beta, levels=levels, stats=stats, relu=1 if c.relu else 0)
    ref = reference(q, inv_levels(c.in_bits), w, b, geom(c), epi)
    return Case(q=q, w=w, b=b, alpha=alpha, beta=beta, stats=stats, epi=epi, ref=ref, inv_n=inv_levels(c.in_bits))


@functools.lru_cache(maxsize=None)
def designed() -> Case:
    """Operands for which every step is exact, so that codes sit EXACTLY on rint ties and on the ReLU boundary: inv_n = 1/4 (an
    entry-level argument: any float), codes 0 .. 15, taps k / 4 with |k| <= 2, bias j / 4 — y is a multiple of 1 / 16 below 32;
    device BatchNorm with mean k / 4, rs = 1 / 2, weight +-2, bias j / 4 — t = +-(y - mean) + bias, a multiple of 1 / 16; 15 t is
    exact in float32 and a tie wherever 16 t = 8 mod 16."""
    N, Cc, m, H, W = 2, 20, 2, 9, 8
    Cout = Cc * m
    r = np.random.RandomState(77)
    q = C.random_codes((N, Cc, H, W), 0, 15, 78, "cpu").numpy()
    w = (r.randint(-2, 3, size=(Cout, 3, 3)) / 4.0).astype(np.float32)
    b = (r.randint(-4, 5, size=(Cout,)) / 4.0).astype(np.float32)
    g = torch.Generator().manual_seed(79)
    weight = (torch.randint(0, 2, (Cout,), generator=g) * 4 - 2).float()
    mean = torch.randint(-8, 9, (Cout,), generator=g).float() / 4
    bias = torch.randint(-4, 5, (Cout,), generator=g).float() / 4
    rs = torch.full((Cout,), 0.5)
    geometry = ((3, 3), (1, 1), (1, 1), (1, 1))
    epi = C.Epi(alpha=weight, beta=bias, levels=15.0, stats=(mean, rs), relu=1)
    ref = reference(q, np.float32(0.25), w, b, geometry, epi)
    y64 = D.forward(image(q, 0.25), w, b, *geometry, dtype=np.float64)
    assert np.array_equal(ref["y"], y64)                       # the conv is exact
    t64 = (torch.from_numpy(y64.transpose(0, 2, 3, 1)) - mean.double()) * 0.5 * weight.double() + bias.double()
    lt = 15.0 * torch.relu(t64)
    ties = int(((lt - torch.floor(lt)) == 0.5).sum())
    on_relu = int((t64 == 0).sum())
    assert torch.equal(ref["t"].double(), torch.relu(t64))      # ... and so is the epilogue
    return Case(N=N, C=Cc, m=m, H=H, W=W, geometry=geometry, q=q, w=w, b=b, alpha=weight, beta=bias, stats=(mean, rs), epi=epi,
                ref=ref, inv_n=np.float32(0.25), ties=ties, on_relu=on_relu, below_relu=int((t64 < 0).sum()))
