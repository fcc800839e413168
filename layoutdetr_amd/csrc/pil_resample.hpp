// Pillow's 8-bit resampling rule (src/libImaging/Resample.c, Pillow==9.3.0), the ONLY place that knows it: per output coordinate a window
// [xmin, xmin + cnt) of weights -- built in double, normalised, 22-bit fixed point rounded half away from zero -- and
//     out = clip8((2^21 + sum px * k) >> 22)
// in integer arithmetic, so a device pass is bit-identical to Pillow's.  Users: resample.hip (Lanczos page resize), layout_raster.hip (bilinear
// snapshot cells).  The host builder has no HIP type in it: a plain host compiler can build it on its own.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/ldetr_hip.h"   // LDETR_FILTER_*

#ifdef __HIPCC__
#define PIL_DEVICE __device__ __forceinline__
#else
#define PIL_DEVICE inline
#endif

namespace ldetr {

constexpr int PIL_PRECISION_BITS = 32 - 8 - 2;
constexpr int PIL_HALF = 1 << (PIL_PRECISION_BITS - 1);   // what an accumulator starts from: the shift in pil_clip8 then rounds

PIL_DEVICE int pil_clip8(int acc) {
    const int v = acc >> PIL_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One output pixel of a pass, three interleaved channels: a0..a2 (each started from PIL_HALF, each finished by pil_clip8) gather the taps
// px[t * stride + c] (bytes) times the weights k[t * k_stride + col] (column `col` of a tap-major table), t < cnt.  STEP > 0 (horizontal pass: 3):
// the taps are STEP bytes apart, indexed from px; STEP == 0 (vertical pass): they are `pitch` bytes apart and px is advanced.  The two address forms
// are a measured choice, not taste: with them the raster's and the page resize's loops compile as they did when each pass was written out (the
// indexed loop unrolled twice, the advancing one not); one form for both passes cost layout_raster_kernel<true> 1 to 2 % at a 1024 canvas,
// whose windows are 3 or 4 taps.  k_stride keeps the caller's integer type:
// tables inside LDS-sized pools are indexed in 32 bits, whole-image tables in 64.
template <int STEP, typename KStride>
PIL_DEVICE void pil_taps3(const unsigned char* px, int pitch, const int* k, KStride k_stride, int col, int cnt, int& a0, int& a1, int& a2) {
    for (int t = 0; t < cnt; t++) {
        const int w = k[t * k_stride + col];
        a0 += px[STEP * t] * w; a1 += px[STEP * t + 1] * w; a2 += px[STEP * t + 2] * w;
        if (!STEP) px += pitch;
    }
}

// Resample.c's windows and precompute_coeffs + normalize_coeffs_8bpc.  No fused multiply-add, whatever the host compiler's flags: the tables are
// pinned bit for bit.
inline double pil_window(int filter, double x) {
#pragma STDC FP_CONTRACT OFF
    if (filter == LDETR_FILTER_BILINEAR) {
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
    auto sinc = [](double v) { return v == 0.0 ? 1.0 : sin(v * M_PI) / (v * M_PI); };
    return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3.0) : 0.0;
}
inline double pil_support(int filter) { return filter == LDETR_FILTER_BILINEAR ? 1.0 : 3.0; }

inline int pil_ksize(int filter, int in_size, int out_size) {
#pragma STDC FP_CONTRACT OFF
    const double scale = (double)in_size / out_size;
    return (int)ceil(pil_support(filter) * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
// bounds [out_size][2] = (first input index, tap count); kk [pil_ksize][out_size], tap-major, zero beyond a window's tap count
inline void pil_coeffs(int filter, int in_size, int out_size, int32_t* bounds, int32_t* kk) {
#pragma STDC FP_CONTRACT OFF
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = pil_support(filter) * filterscale;
    const int ksize = pil_ksize(filter, in_size, out_size);
    const double ss = 1.0 / filterscale;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; xx++) {
        const double center = 0.0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5); if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) { w[x] = pil_window(filter, (x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < ksize; x++) {
            int q = 0;
            if (x < xmax) {
                const double v = ww != 0.0 ? w[x] / ww : w[x];
                q = v < 0 ? (int)(-0.5 + v * (1 << PIL_PRECISION_BITS)) : (int)(0.5 + v * (1 << PIL_PRECISION_BITS));
            }
            kk[(int64_t)x * out_size + xx] = q;
        }
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
    }
}

}  // namespace ldetr
