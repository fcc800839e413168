// Batched anti-aliased resize of uint8 images of different sizes: what the reference's image snapshots do per element with
//     skimage.transform.resize(im, (h', w'), anti_aliasing=True)      util.py:171, 240, 262
// on float arrays fetched from the device one at a time, as ONE launch per grid: every element crop and every page background is a job.
//
// Rule (rule 10), per spatial axis of a job n -> n': f = n / n', sigma = max(0, (f - 1) / 2), radius r = int(4 sigma + 0.5);
// a Gaussian of 2r + 1 normalised weights with the `mirror` boundary (period 2 (n - 1), reflected; n == 1 -> index 0), axis 0 before axis 1; then
// linear interpolation at c = (o + 0.5) f - 0.5 between the mirror-mapped floor(c) and floor(c) + 1, axis 0 before axis 1.  Weights and indices
// come from the host (built in double, passed as fp32: no device expf).  Arithmetic: v = u8 / 255 in fp32; every Gaussian sum starts at 0 and adds
// weight * value for k = -r .. r in that order; an interpolation is (w0 * a) + (w1 * b); one IEEE operation each (no fma contraction); the result
// is clamped to [0, 1] and written as floor(v * 255 + 2^-10).  A pass with r == 0 has the single weight 1.0: 0 + 1 * v == v, so it is a copy.
//
// Work layout: grid (tiles, jobs); a workgroup owns a Ty x Tx tile of one job's output (sized per job on the host, rows of up to 64 pixels so
// that a wave reads and writes contiguous bytes) and returns at once when its tile index lies beyond the job's extent.  It stages the source
// window the tile needs (tile extent x zoom + 2 radius per axis) in LDS as fp32, then runs both Gaussian passes and both interpolation passes
// between two LDS buffers (40 KiB + 20 KiB); uint8 is written once, and no float image or intermediate reaches HBM.
// What bounds it: LDS traffic of the Gaussian taps ((2 ry + 1) + (2 rx + 1) reads per window pixel and channel) when a job shrinks, the source
// bytes otherwise.  Limits the entry enforces: sizes in [1, 16384] per axis, radius <= 4096, and per job the window of a 1 x 1 tile must fit
// the two buffers: about (2 + 2 ry) * (2 + 2 rx) <= 3413 pixels, e.g. zoom 14 on both axes or zoom 200 on one axis with the other kept.
#include <limits.h>
#include <math.h>

#include <vector>

#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"

#pragma clang fp contract(off)

namespace ldetr {

constexpr int PR_THREADS = 256;
constexpr int PR_JOB_INTS = 16;           // per-job descriptor, see the host entry
constexpr int PR_A_FLOATS = 10240;        // source window / axis-1 Gaussian output
constexpr int PR_B_FLOATS = 5120;         // axis-0 Gaussian output / axis-0 interpolation output
constexpr int PR_MAX_SIZE = 16384;
constexpr int PR_MAX_RADIUS = 4096;
constexpr int PR_TILE_Y = 16, PR_TILE_X = 64;

struct PatchResizeParams {
    const unsigned char* src0; const unsigned char* src1; unsigned char* dst; const int* tables; const int* jobs;
};

__device__ __forceinline__ int pr_mirror(int i, int n) {
    if (i >= 0 && i < n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - m : m;
}

// one axis table in the pool: [r][2r + 1 Gaussian weights][i0 x out][i1 x out][w0 x out][w1 x out], floats stored as their bits
struct PrAxis {
    int r; const float* g; const int* i0; const int* i1; const float* w0; const float* w1;
};
__device__ __forceinline__ PrAxis pr_axis(const int* t, int out) {
    PrAxis a;
    a.r = t[0]; a.g = (const float*)(t + 1); a.i0 = t + 2 + 2 * a.r; a.i1 = a.i0 + out;
    a.w0 = (const float*)(a.i1 + out); a.w1 = a.w0 + out;
    return a;
}

// grid (tiles, jobs)
__global__ __launch_bounds__(PR_THREADS) void patch_resize_kernel(PatchResizeParams p) {
    __shared__ float A[PR_A_FLOATS];
    __shared__ float Bf[PR_B_FLOATS];
    const int* j = p.jobs + (long)blockIdx.y * PR_JOB_INTS;
    const int h = j[2], w = j[3], ho = j[6], wo = j[7], Ty = j[10], Tx = j[11], ntx = j[12], nty = j[13];
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (tile >= ntx * nty) return;
    const int oy0 = (tile / ntx) * Ty, oy1 = min(oy0 + Ty, ho), ox0 = (tile % ntx) * Tx, ox1 = min(ox0 + Tx, wo);
    const PrAxis ay = pr_axis(p.tables + j[8], ho), ax = pr_axis(p.tables + j[9], wo);
    // rows / columns of the filtered image this tile interpolates between, and the source window they need
    int gy0 = INT_MAX, gy1 = -1, gx0 = INT_MAX, gx1 = -1;
    for (int o = oy0; o < oy1; o++) { const int a = ay.i0[o], b = ay.i1[o]; gy0 = min(gy0, min(a, b)); gy1 = max(gy1, max(a, b)); }
    for (int o = ox0; o < ox1; o++) { const int a = ax.i0[o], b = ax.i1[o]; gx0 = min(gx0, min(a, b)); gx1 = max(gx1, max(a, b)); }
    const int sy0 = max(0, gy0 - ay.r), sy1 = min(h - 1, gy1 + ay.r), sx0 = max(0, gx0 - ax.r), sx1 = min(w - 1, gx1 + ax.r);
    const int Rs = sy1 - sy0 + 1, Cs = sx1 - sx0 + 1, Rg = gy1 - gy0 + 1, Cg = gx1 - gx0 + 1, nTy = oy1 - oy0, nTx = ox1 - ox0;
    const int rows = Cs * 3, rowg = Cg * 3, rowo = nTx * 3;
    if (gy0 < 0 || gx0 < 0 || gy1 >= h || gx1 >= w || (long)Rs * rows > PR_A_FLOATS || (long)Rg * rows > PR_B_FLOATS || (long)nTy * rowg > PR_B_FLOATS)
        return;                                                      // (never: the host sized the tile for it and checked the indices)
    const unsigned char* src = (j[14] ? p.src1 : p.src0) + get_i64(j);
    unsigned char* dst = p.dst + get_i64(j + 4);
    // 0. the source window, u8 / 255
    for (int i = tid; i < Rs * rows; i += PR_THREADS) {
        const int r = i / rows, c = i - r * rows;
        A[i] = (float)src[((long)(sy0 + r) * w + sx0) * 3 + c] / 255.f;
    }
    __syncthreads();
    // 1. Gaussian along axis 0: A [Rs][Cs] -> Bf [Rg][Cs]
    for (int i = tid; i < Rg * rows; i += PR_THREADS) {
        const int g = i / rows, c = i - g * rows;
        float acc;
        if (ay.r == 0) acc = A[(gy0 + g - sy0) * rows + c];
        else {
            acc = 0.f;
            for (int k = -ay.r; k <= ay.r; k++) acc = acc + ay.g[k + ay.r] * A[(pr_mirror(gy0 + g + k, h) - sy0) * rows + c];
        }
        Bf[i] = acc;
    }
    __syncthreads();
    // 2. Gaussian along axis 1: Bf [Rg][Cs] -> A [Rg][Cg]
    for (int i = tid; i < Rg * rowg; i += PR_THREADS) {
        const int g = i / rowg, c3 = i - g * rowg, cx = c3 / 3, ch = c3 - cx * 3;
        float acc;
        if (ax.r == 0) acc = Bf[g * rows + (gx0 + cx - sx0) * 3 + ch];
        else {
            acc = 0.f;
            for (int k = -ax.r; k <= ax.r; k++) acc = acc + ax.g[k + ax.r] * Bf[g * rows + (pr_mirror(gx0 + cx + k, w) - sx0) * 3 + ch];
        }
        A[i] = acc;
    }
    __syncthreads();
    // 3. interpolation along axis 0: A [Rg][Cg] -> Bf [nTy][Cg]
    for (int i = tid; i < nTy * rowg; i += PR_THREADS) {
        const int t = i / rowg, c = i - t * rowg, o = oy0 + t;
        const float m0 = ay.w0[o] * A[(ay.i0[o] - gy0) * rowg + c], m1 = ay.w1[o] * A[(ay.i1[o] - gy0) * rowg + c];
        Bf[i] = m0 + m1;
    }
    __syncthreads();
    // 4. interpolation along axis 1, clamp, quantise: Bf [nTy][Cg] -> uint8
    for (int i = tid; i < nTy * rowo; i += PR_THREADS) {
        const int t = i / rowo, c3 = i - t * rowo, x = c3 / 3, ch = c3 - x * 3, o = ox0 + x;
        const float m0 = ax.w0[o] * Bf[t * rowg + (ax.i0[o] - gx0) * 3 + ch], m1 = ax.w1[o] * Bf[t * rowg + (ax.i1[o] - gx0) * 3 + ch];
        float v = m0 + m1;
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        const float q = v * 255.f;
        dst[((long)(oy0 + t) * wo + ox0) * 3 + c3] = (unsigned char)(int)floorf(q + 0.0009765625f);
    }
}

// the largest extent, over the tiles of T outputs, of the filtered rows a tile touches (g) and of the source window behind them (s)
static void pr_extents(const int32_t* i0, const int32_t* i1, int out, int T, int r, int n, long* g_ext, long* s_ext) {
    long ge = 0, se = 0;
    for (int o0 = 0; o0 < out; o0 += T) {
        int lo = INT_MAX, hi = -1;
        for (int o = o0; o < out && o < o0 + T; o++) {
            lo = std::min(lo, std::min(i0[o], i1[o]));
            hi = std::max(hi, std::max(i0[o], i1[o]));
        }
        ge = std::max(ge, (long)hi - lo + 1);
        se = std::max(se, (long)std::min(n - 1, hi + r) - std::max(0, lo - r) + 1);
    }
    *g_ext = ge; *s_ext = se;
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_patch_resize_u8(const ldetr_patch_resize_args* a, void* stream) {
    LDETR_CHECK_BLOCK(a, ldetr_patch_resize_args, "patch_resize");
    const int J = a->n_jobs;
    LDETR_CHECK(J >= 0 && J <= 65535, "patch_resize: 0 <= jobs <= 65535 (got %d)", J);
    if (J == 0) return LDETR_OK;
    LDETR_CHECK(a->jobs && a->tables && a->tables_host && a->jobs_dev && a->dst, "patch_resize: null pointer");
    LDETR_CHECK(a->tables_len >= 0 && a->dst_bytes >= 0 && a->src0_bytes >= 0 && a->src1_bytes >= 0, "patch_resize: negative buffer size");
    static thread_local std::vector<int32_t> jobs;                     // outlives the call: the upload below reads it
    jobs.assign((size_t)J * PR_JOB_INTS, 0);
    long tiles = 1;
    for (int k = 0; k < J; k++) {
        const int64_t* q = a->jobs + 9 * (long)k;                      // (source buffer, src offset, h, w, dst offset, h', w', axis-0 table, axis-1 table)
        LDETR_CHECK(q[0] == 0 || q[0] == 1, "patch_resize: job %d: source buffer %ld (0 or 1)", k, (long)q[0]);
        const uint8_t* sb = q[0] ? a->src1 : a->src0;
        const int64_t sbytes = q[0] ? a->src1_bytes : a->src0_bytes;
        LDETR_CHECK(sb, "patch_resize: job %d: source buffer %ld is null", k, (long)q[0]);
        LDETR_CHECK(q[2] >= 1 && q[3] >= 1 && q[2] <= PR_MAX_SIZE && q[3] <= PR_MAX_SIZE, "patch_resize: job %d: source %ld x %ld outside [1, %d]", k, (long)q[3],
                    (long)q[2], PR_MAX_SIZE);
        LDETR_CHECK(q[5] >= 1 && q[6] >= 1 && q[5] <= PR_MAX_SIZE && q[6] <= PR_MAX_SIZE, "patch_resize: job %d: target %ld x %ld outside [1, %d]", k, (long)q[6],
                    (long)q[5], PR_MAX_SIZE);
        const int h = (int)q[2], w = (int)q[3], ho = (int)q[5], wo = (int)q[6];
        LDETR_CHECK(q[1] >= 0 && q[1] + (int64_t)h * w * 3 <= sbytes, "patch_resize: job %d: source reaches past its buffer", k);
        LDETR_CHECK(q[4] >= 0 && q[4] + (int64_t)ho * wo * 3 <= a->dst_bytes, "patch_resize: job %d: target reaches past the output buffer", k);
        const int32_t* tab[2];
        int rad[2];
        for (int ax = 0; ax < 2; ax++) {
            const int64_t off = q[7 + ax];
            const int n = ax ? w : h, out = ax ? wo : ho;
            LDETR_CHECK(off >= 0 && off < a->tables_len, "patch_resize: job %d: axis %d table offset outside the pool", k, ax);
            const int r = a->tables_host[off];
            LDETR_CHECK(r >= 0 && r <= PR_MAX_RADIUS, "patch_resize: job %d: axis %d radius %d outside [0, %d]", k, ax, r, PR_MAX_RADIUS);
            LDETR_CHECK(off + 2 + 2 * (int64_t)r + 4 * (int64_t)out <= a->tables_len, "patch_resize: job %d: axis %d table reaches past the pool", k, ax);
            const int32_t* i0 = a->tables_host + off + 2 + 2 * r;
            for (int o = 0; o < 2 * out; o++)
                LDETR_CHECK(i0[o] >= 0 && i0[o] < n, "patch_resize: job %d: axis %d table names source index %d of %d", k, ax, i0[o], n);
            tab[ax] = i0; rad[ax] = r;
        }
        // tile: the source window and the intermediates of a tile must fit the two LDS buffers
        int Ty = std::min(ho, PR_TILE_Y), Tx = std::min(wo, PR_TILE_X);
        for (;;) {
            long gy, sy, gx, sx;
            pr_extents(tab[0], tab[0] + ho, ho, Ty, rad[0], h, &gy, &sy);
            pr_extents(tab[1], tab[1] + wo, wo, Tx, rad[1], w, &gx, &sx);
            if (sy * sx * 3 <= PR_A_FLOATS && gy * sx * 3 <= PR_B_FLOATS && (long)Ty * gx * 3 <= PR_B_FLOATS) break;
            LDETR_CHECK(Ty > 1 || Tx > 1, "patch_resize: job %d: %d x %d -> %d x %d needs a %ld x %ld source window per output pixel, more than the %d floats of LDS", k,
                        w, h, wo, ho, sx, sy, PR_A_FLOATS);
            if (Tx > 1 && (Tx >= 4 * Ty || Ty == 1)) Tx = (Tx + 1) / 2;
            else Ty = (Ty + 1) / 2;
        }
        int32_t* c = jobs.data() + (size_t)k * PR_JOB_INTS;
        put_i64(c, q[1]); c[2] = h; c[3] = w;
        put_i64(c + 4, q[4]); c[6] = ho; c[7] = wo;
        c[8] = (int32_t)q[7]; c[9] = (int32_t)q[8]; c[10] = Ty; c[11] = Tx;
        c[12] = (wo + Tx - 1) / Tx; c[13] = (ho + Ty - 1) / Ty; c[14] = (int32_t)q[0];
        tiles = std::max(tiles, (long)c[12] * c[13]);
    }
    LDETR_CHECK(a->tables_len < (1L << 31), "patch_resize: table pool too large");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_descriptors("patch_resize", a->jobs_dev, jobs.data(), jobs.size(), st)) return rc;
    PatchResizeParams p;
    p.src0 = a->src0; p.src1 = a->src1; p.dst = a->dst; p.tables = a->tables; p.jobs = a->jobs_dev;
    hipLaunchKernelGGL(patch_resize_kernel, dim3((unsigned)tiles, (unsigned)J), PR_THREADS, 0, st, p);
    return check_launch("patch_resize");
}
