// The planes half of qt_gmconv2d_describe (include/qt_hip.h): the entry lives in gconv_mfma.hip, the walk it reports for
// QT_GM_OP_PLANES in gconv_planes_mfma.hip, next to the launch that runs the same functions.  Host code only.
#pragma once
#include <cstdint>

// The status qt_gmconv2d_sign (no output halo) returns for these numbers up to its pointer checks, and — where it would launch —
// the walk of that launch as text in out[cap].  An empty problem: QT_OK and an empty text.
__attribute__((visibility("hidden"))) int gp_describe(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                int pw, int dh, int dw, char* out, int cap);
