#!/usr/bin/env python
"""c2_tail_f16x2_256x256x512.npy: the fp16 two-term linear at 256 x 256 x 512 on the 256x256 ping-pong tile, as the kernel computed
it BEFORE its store tail changed (tests/test_gpu_c2_gemm_tail.py::test_f16_two_term_bits_unchanged compares bit for bit).

Provenance: written on an MI355X by the commit before the row-wide stores (6d40b59), with one addition and nothing else: the entry
point qt_f16_gemm_variant (include/qt_hip.h, csrc/mfma_gemm.hip) and the ``variant`` argument of ops.bf16_gemm, which that commit
did not have and without which no call reaches PP256<ElemF16> at this shape.  The kernel, its header and the build flags were that
commit's.  Inputs: the counter PRNG of synth.py (f16_two_term in the test module), so nothing but the result is stored.

Running it on a later commit only restates that commit's own output; regenerate it from the commit named above.

    python tests/golden/make_golden_c2_tail.py     # needs the GPU; rewrites tests/golden/c2_tail_f16x2_256x256x512.npy
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_c2_gemm_tail as T  # noqa: E402

if __name__ == "__main__":
    y = T.f16_two_term(torch.device("cuda:0"), profile=True)
    assert y.shape == (256, 256) and y.dtype == np.float32
    np.save(T.GOLDEN, y)
    print("wrote", T.GOLDEN, float(np.abs(y).max()))
