"""Independent reference for the grouped convs on int8 code planes (include/qt_hip.h "Grouped convolution on int8 code planes"),
shared by tests/test_gconv_codes_cpu.py and tests/test_gpu_gconv_codes.py.  Nothing of the package's packers or kernels is used:

* codes come from ``_codes_exact.random_codes`` (or are written by hand),
* the image is ``float32(inv_n) * q`` in numpy float32 (one rounding: what the kernel's decode forms),
* the conv value comes from ``_gconv_exact.forward`` in float32, which restates the pinned order of qt_gconv2d_f32,
* the epilogue is ``_codes_exact.epilogue`` with an ``Epi`` without a residual,
* planes are encoded / decoded with ``_codes_exact.encode_plane`` / ``decode_plane`` / ``check_plane_zeros``.

``CASES`` is the list the GPU file walks; ``build(i)`` its operands and reference (computed once per process).  The seeds are part
of the list: for each of them the reference's own count of sensitive elements (``_codes_exact.sensitive``) is zero (and, for case
0, no code leaves int8), which the CPU file asserts, so the GPU comparison waives nothing."""
import functools

import numpy as np
import torch

import _codes_exact as C
import _gconv_exact as G
from _dw_codes import GEOMS, MAPS, BATCHES, HALOS, BITS, TAPS, FORMS, Case, inv_levels, code_range, image, taps, bn_params  # noqa: F401

#        (G, cin_g, cout_g)
SHAPES = ((4, 2, 2),       # 8-byte rows inside a 16-byte ld
          (4, 4, 4),       # an exact 16-byte row
          (5, 8, 4),       # ld padding
          (4, 3, 3),       # odd cin_g; a dword straddling groups
          (33, 4, 1),      # four groups per dword; a partial last dword; more than 128 input channels
          (4, 8, 17),      # cout_g = 17
          (6, 1, 2),       # must equal qt_dwconv2d_codes byte for byte
          (4, 16, 8))      # inside the entry's limits, beyond the layers' route
# every compile-time form of the kernel (1 x 1 and 3 x 3 at cin_g 2 / 4 / 8 with cout_g % 4 == 0) that the walk below does not
# reach: (shape, index into GEOMS or a geometry of its own).  The last two are 1 x 1 kernels WITH padding (and a stride): the only 1 x 1
# of GEOMS has none, so without them the clamp / select of the compile-time 1 x 1 forms would never meet a tap outside the image
EXTRA = (((4, 2, 4), 0), ((4, 2, 4), 3), ((4, 4, 4), 3), ((5, 8, 4), 0), ((4, 4, 4), 0), ((5, 8, 8), 1), ((20, 2, 4), 3),
         ((9, 4, 8), 0), ((4, 4, 4), ((1, 1), (1, 1), (1, 1), (1, 1))), ((5, 8, 4), ((1, 1), (2, 1), (1, 2), (1, 1))))
MAC_BUDGET = 3_000_000


def _case(i):
    n = 2 * len(SHAPES)
    if i < n:
        shape, k = SHAPES[i % len(SHAPES)], GEOMS[i % len(GEOMS)]
    else:
        shape, k = EXTRA[i - n]
        k = GEOMS[k] if isinstance(k, int) else k
    Gg, ci, co = shape
    (H, W) = MAPS[i % len(MAPS)]
    k, s, p, d = k
    N = BATCHES[(i // 2) % 2]
    c = Case(i=i, G=Gg, cin_g=ci, cout_g=co, H=H, W=W, N=N, kernel=k, stride=s, padding=p, dilation=d,
             in_halo=HALOS[i % 3], out_halo=HALOS[(i // 3 + i) % 3], in_bits=BITS[i % 3], out_bits=BITS[(i // 2) % 3],
             relu=(i % 4) < 2, form=FORMS[i % 2], bias=(i % 3) != 1, taps=TAPS[(i // 2) % 3], seed=5000 + 17 * i)
    c["id"] = (f"g{Gg}i{ci}o{co}N{N}-k{k[0]}x{k[1]}-s{s[0]}{s[1]}-p{p[0]}{p[1]}-d{d[0]}-{H}x{W}-ih{c.in_halo[0]}{c.in_halo[1]}"
               f"-oh{c.out_halo[0]}{c.out_halo[1]}-a{c.in_bits}to{c.out_bits}-{c.form}-{c.taps}")
    return c


# the eight shapes twice each over the seven geometries (each at least twice), then the compile-time forms
CASES = [_case(i) for i in range(2 * len(SHAPES) + len(EXTRA))]


def geom(c):
    return c.kernel, c.stride, c.padding, c.dilation


def macs(c) -> int:
    Ho, Wo = G.out_hw(c.H, c.W, *geom(c))
    return c.N * c.G * c.cout_g * Ho * Wo * c.cin_g * c.kernel[0] * c.kernel[1]


def reference(q: np.ndarray, inv_n, w: np.ndarray, bias, groups: int, geometry, epi: C.Epi) -> dict:
    """``_codes_exact.epilogue`` of the grouped conv of the image of ``q`` [N, G cin_g, H, W] with ``w`` [G cout_g, cin_g, kh, kw];
    every tensor of the result is [N, Ho, Wo, G cout_g] (channels last).  ``y`` (float32, NCHW) is added."""
    y = G.forward(image(q, inv_n), w, bias, groups, *geometry)
    assert y.dtype == np.float32
    ref = C.epilogue(torch.from_numpy(np.ascontiguousarray(y.transpose(0, 2, 3, 1))), epi)
    ref["y"] = y
    return ref


def out_plane(ref: dict, halo) -> torch.Tensor:
    """The int8 output plane the kernel must write: the reference's codes with a zero border and zero pad bytes."""
    return C.encode_plane(ref["codes"].permute(0, 3, 1, 2), halo)


def operands(c, seed: int) -> Case:
    Cin, Cout = c.G * c.cin_g, c.G * c.cout_g
    lo, hi = code_range(c.in_bits)
    q = C.random_codes((c.N, Cin, c.H, c.W), lo, hi, seed, "cpu").numpy()
    w = taps(c.taps, seed + 1, (Cout, c.cin_g) + c.kernel)
    b = (np.random.RandomState(seed + 2).randn(Cout) * 0.2).astype(np.float32) if c.bias else None
    levels = float((1 << c.out_bits) - 1)
    alpha, beta, stats = bn_params(Cout, c.cin_g * c.kernel[0] * c.kernel[1], levels, seed + 3, c.form)
    epi = C.Epi(alpha=alpha, beta=beta, levels=levels, stats=stats, relu=1 if c.relu else 0)
    ref = reference(q, inv_levels(c.in_bits), w, b, c.G, geom(c), epi)
    return Case(q=q, w=w, b=b, alpha=alpha, beta=beta, stats=stats, epi=epi, ref=ref, inv_n=inv_levels(c.in_bits))


@functools.lru_cache(maxsize=None)
def build(i: int) -> Case:
    return operands(CASES[i], CASES[i].seed)


@functools.lru_cache(maxsize=None)
def designed() -> Case:
    """Operands for which every step is exact at cin_g = 4, so that codes sit EXACTLY on rint ties and on the ReLU boundary:
    inv_n = 1/4, codes 0 .. 15, taps k / 4 with |k| <= 2, bias j / 4 — y is a sum of 36 multiples of 1 / 16, below 128; device
    BatchNorm with mean k / 4, rs = 1 / 8, weight +-2, bias j / 4 — t = +-(y - mean) / 4 + bias, a multiple of 1 / 64; 15 t is exact
    in float32 and a tie wherever 64 t = 32 mod 64."""
    N, Gg, ci, co, H, W = 2, 5, 4, 4, 9, 8
    Cout = Gg * co
    r = np.random.RandomState(177)
    q = C.random_codes((N, Gg * ci, H, W), 0, 15, 178, "cpu").numpy()
    w = (r.randint(-2, 3, size=(Cout, ci, 3, 3)) / 4.0).astype(np.float32)
    b = (r.randint(-4, 5, size=(Cout,)) / 4.0).astype(np.float32)
    g = torch.Generator().manual_seed(179)
    weight = (torch.randint(0, 2, (Cout,), generator=g) * 4 - 2).float()
    mean = torch.randint(-8, 9, (Cout,), generator=g).float() / 4
    bias = torch.randint(-4, 5, (Cout,), generator=g).float() / 4
    rs = torch.full((Cout,), 0.125)
    geometry = ((3, 3), (1, 1), (1, 1), (1, 1))
    epi = C.Epi(alpha=weight, beta=bias, levels=15.0, stats=(mean, rs), relu=1)
    ref = reference(q, np.float32(0.25), w, b, Gg, geometry, epi)
    y64 = G.forward(image(q, 0.25), w, b, Gg, *geometry, dtype=np.float64)
    assert np.array_equal(ref["y"], y64)                       # the conv is exact
    t64 = (torch.from_numpy(y64.transpose(0, 2, 3, 1)) - mean.double()) * 0.125 * weight.double() + bias.double()
    lt = 15.0 * torch.relu(t64)
    ties = int(((lt - torch.floor(lt)) == 0.5).sum())
    on_relu = int((t64 == 0).sum())
    assert torch.equal(ref["t"].double(), torch.relu(t64))      # ... and so is the epilogue
    return Case(N=N, G=Gg, cin_g=ci, cout_g=co, H=H, W=W, geometry=geometry, q=q, w=w, b=b, alpha=weight, beta=bias,
                stats=(mean, rs), epi=epi, ref=ref, inv_n=np.float32(0.25), ties=ties, on_relu=on_relu,
                below_relu=int((t64 < 0).sum()))
