"""Independent reference for the depthwise convs on bit planes (include/qt_hip.h "Depthwise convolution on bit planes"): numpy
only, nothing of the package is imported.  The value comes from ``_dw_exact.forward`` in float32 (the pinned order); this file adds
the threshold bit — a float32 multiply, a float32 add, ``< 0`` — and the two plane layouts, packed with numpy.

* sign plane  : int32 [N H W, ld], ld = max(4, ceil(C / 32) rounded up to 4); bit (k & 31) of word (k >> 5) of pixel row
                (n H + h) W + w is channel k, 1 <=> negative; all other bits zero.
* nibble plane: int32 [N (H + 2 hy) (W + 2 hx), ldn], ldn = max(4, ceil(C / 8) rounded up to 4); element k in nibble (k & 7) of
                word (k >> 3), +1 = 0x2, -1 = 0xA; channels >= C and the hy x hx border pixels are zero words.

tests/test_dwconv_chain_cpu.py pins both packers on hand-written words."""
import numpy as np


def packed_ld(K):
    return max(4, ((int(K) + 31) // 32 + 3) // 4 * 4)


def pixel_ld_nib(K):
    return max(4, ((int(K) + 7) // 8 + 3) // 4 * 4)


def threshold_bits(y, alpha, beta):
    """[fl(fl(y alpha) + beta) < 0] per element of y [N, C, H, W]: numpy rounds the float32 product and the float32 sum once each."""
    y = np.asarray(y, dtype=np.float32)
    a = np.asarray(alpha, dtype=np.float32)[None, :, None, None]
    b = np.asarray(beta, dtype=np.float32)[None, :, None, None]
    t = y * a
    assert t.dtype == np.float32
    return (t + b) < 0


def pack_sign(neg, ld=None):
    """Sign plane of a boolean [N, C, H, W] array (True = negative)."""
    neg = np.asarray(neg, dtype=bool)
    N, C, H, W = neg.shape
    ld = packed_ld(C) if ld is None else int(ld)
    rows = neg.transpose(0, 2, 3, 1).reshape(N * H * W, C)
    out = np.zeros((N * H * W, ld), dtype=np.uint32)
    for k in range(C):
        out[:, k >> 5] |= rows[:, k].astype(np.uint32) << np.uint32(k & 31)
    return out.view(np.int32)


def pack_nib(neg, halo=(0, 0), ld=None):
    """Nibble pixel plane of the +-1 image whose negative elements ``neg`` marks, with a zero border of ``halo`` pixels."""
    neg = np.asarray(neg, dtype=bool)
    N, C, H, W = neg.shape
    hy, hx = int(halo[0]), int(halo[1])
    ld = pixel_ld_nib(C) if ld is None else int(ld)
    img = np.zeros((N, H + 2 * hy, W + 2 * hx, ld), dtype=np.uint32)
    inner = img[:, hy:hy + H, hx:hx + W]
    px = neg.transpose(0, 2, 3, 1)
    for k in range(C):
        code = np.where(px[..., k], np.uint32(0xA), np.uint32(0x2))
        inner[..., k >> 3] |= code << np.uint32(4 * (k & 7))
    return img.reshape(N * (H + 2 * hy) * (W + 2 * hx), ld).view(np.int32)
