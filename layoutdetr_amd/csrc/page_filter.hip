// The two page filters of the reference's generation tool, on decoded uint8 pages in GPU memory:
//     background = background_orig.filter(ImageFilter.GaussianBlur(radius=3))                         generate.py:267-269
//     background = background_orig.convert('L').filter(ImageFilter.FIND_EDGES).convert('RGB')         generate.py:280-282
// Both are 8-bit integer arithmetic in Pillow, so the device result is bit-identical to Pillow's (as csrc/resample.hip's resize is).
//
// Blur (src/libImaging/BoxBlur.c): the Gaussian radius becomes ONE fractional box radius fr (r = its integer part; weight ww for the 2r + 1 inner
// pixels, fw for the two outermost, 24-bit fixed point); the box runs three times along x, then three times along y, each pass rounded to 8 bits:
//     out[x] = (ww * sum_{d = -r..r} in[clamp(x + d)] + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24        (32-bit unsigned)
// Pillow's _gaussian_blur_radius keeps its intermediates in C floats; box_params() below does the same (in double, ww differs by one at a few radii).
// Edge: g = (19595 R + 38470 G + 7471 B + 32768) >> 16; first / last row and column keep g, the rest clip(9 g - sum of the 3x3 neighbourhood, 0, 255),
// written to all three channels.  The grey image exists in LDS only.
//
// Shape.  Byte work: a 1024 x 1024 page is 3 MB in and 3 MB out, microseconds of HBM time, while the blur is six passes of ~15 integer instructions
// and three LDS byte accesses per byte -- bound by instruction issue and LDS traffic, like resample.hip.  So: ONE launch per call, a block per
// PF_TILE x PF_TILE output tile of one image, nothing between global load and global store but LDS.
//  * PF_TILE = 64.  The blur needs a halo of h = 3 (r + 1) pixels on every side (each pass eats r + 1; h = 9 at radius 3, at most 15 at radius 5),
//    two LDS buffers of (64 + 2h) rows, rows padded to an odd number of dwords (threads that own neighbouring rows then sit on different banks):
//    2 x 82 x 252 B = 41 KB at radius 3 (three blocks per CU's 160 KiB), 2 x 94 x 284 B = 53 KB at radius 5 (two blocks, the floor asked for).
//    A 32-tile would read (32 + 18)^2 / 32^2 = 2.4 x its output at radius 3, the 64-tile 1.64 x; a 128-tile (1.3 x) is 128 KB: one block per CU.
//  * Staging: the tile plus halo, with 4-byte global loads (two aligned dwords funnel-shifted into one LDS dword: page rows are 3 W bytes and start
//    at any alignment).  Positions outside the page are filled with the clamped pixel, so the staged buffer holds in[clamp(y)][clamp(x)].
//  * A pass: a thread owns one line of one channel (x passes: (row, channel), 3 (64 + 2h) lines; y passes: (column, channel), 192 lines) and slides
//    the box along it: two byte reads and one byte write per output.  It computes the positions inside the page, from a source that already holds
//    the replicated values beyond the page border, and then writes ITS border value to the positions beyond the border: every pass sees the
//    replication Pillow's clamped indices give, never a value computed from a shrinking halo.  The valid window shrinks by r + 1 per pass and ends
//    as the tile.
//  * The tile leaves through LDS as aligned dword stores (two LDS dwords funnel-shifted), bytes only at the ends of a row.
// Edge: the same staging with a 1-pixel halo, a grey plane in LDS, one thread per pixel, the same store path.  18 KB of LDS.
// PF_TILE is mirrored by PAGE_FILTER_TILE in training/dataset_layoutganpp.py (the tests aim at tile seams through it).
#include <math.h>

#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"

namespace ldetr {

constexpr int PF_TILE = 64;
constexpr int PF_THREADS = 256;
constexpr int PF_MAX_HALO = 15;                             // 3 * (r + 1), r <= 4 for radius <= 5
constexpr int PF_OUT_WORDS = PF_TILE * 3 / 4 + 1;           // aligned dwords a tile row of 192 bytes can touch

struct PageFilterParams {
    const unsigned char* src; unsigned char* dst; long bytes;      // bytes = images * H * W * 3
    int H, W;
    int r, halo, pitch;                                     // box radius, staged halo, LDS row pitch in bytes (a multiple of 4)
    unsigned int ww, fw;
};

__host__ __device__ inline int pf_pitch(int halo) { return ((((PF_TILE + 2 * halo) * 3 + 3) >> 2) | 1) * 4; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Stage rows [0, rows) x columns [0, cols) of the tile's neighbourhood into buf: local (ly, lx) = page pixel (clamp(gy0 + ly), clamp(gx0 + lx)).
__device__ __forceinline__ void pf_stage(const PageFilterParams& p, unsigned char* buf, long img, int gy0, int gx0, int rows, int cols) {
    const int words = (cols * 3 + 3) >> 2;                  // <= pitch / 4; bytes past cols * 3 are padding (filled with a clamped pixel)
    const int c_lo = max(0, gx0), c_hi = min(p.W, gx0 + cols);          // page columns read as they are: local bytes [b_lo, b_hi)
    const int b_lo = (c_lo - gx0) * 3, b_hi = (c_hi - gx0) * 3;
    for (int i = threadIdx.x; i < rows * words; i += PF_THREADS) {
        const int ly = i / words, j = i - ly * words;
        const int gy = clampi(gy0 + ly, 0, p.H - 1);
        const long row = (img * p.H + gy) * (long)p.W * 3;             // byte offset of the page row
        unsigned int w = 0;
        bool done = false;
        if (4 * j >= b_lo && 4 * j + 4 <= b_hi) {
            const long g = row + (long)gx0 * 3 + 4 * j;                // >= row, since 4 j >= b_lo
            const int a = (int)(g & 3);
            const long base = g - a;
            if (base + (a ? 8 : 4) <= p.bytes) {
                const unsigned int w0 = *reinterpret_cast<const unsigned int*>(p.src + base);
                if (a) {
                    const unsigned int w1 = *reinterpret_cast<const unsigned int*>(p.src + base + 4);
                    w = (w0 >> (8 * a)) | (w1 << (32 - 8 * a));
                } else {
                    w = w0;
                }
                done = true;
            }
        }
        if (!done) {                                                   // page border, row ends, the last bytes of the buffer: byte by byte
            for (int k = 0; k < 4; k++) {
                const int b = 4 * j + k, col = b / 3, c = b - col * 3;
                const int gx = clampi(gx0 + col, 0, p.W - 1);
                w |= (unsigned int)p.src[row + (long)gx * 3 + c] << (8 * k);
            }
        }
        *reinterpret_cast<unsigned int*>(buf + ly * p.pitch + 4 * j) = w;
    }
}

// Write LDS rows [0, th) (row ry at buf + off0 + ry * pitch, tw * 3 bytes each; buf dword aligned, off0 any) to the tile at page pixel (y0, x0):
// aligned dwords, bytes at the row ends.
__device__ __forceinline__ void pf_store(const PageFilterParams& p, const unsigned char* buf, int off0, long img, int y0, int x0, int th, int tw) {
    const int nb = tw * 3;
    for (int i = threadIdx.x; i < th * PF_OUT_WORDS; i += PF_THREADS) {
        const int ry = i / PF_OUT_WORDS, j = i - ry * PF_OUT_WORDS;
        const long g0 = ((img * p.H + y0 + ry) * (long)p.W + x0) * 3;  // first byte of the tile row
        const long A = (g0 & ~3L) + 4L * j;                            // this thread's aligned dword
        const int k = (int)(A - g0);                                   // tile-row byte of the dword's first byte (-3 .. nb + 2)
        if (k >= nb) continue;
        const unsigned char* rowp = buf + off0 + ry * p.pitch;
        if (k >= 0 && k + 4 <= nb) {
            const int lds = off0 + ry * p.pitch + k, s = lds & 3;
            const unsigned int* lw = reinterpret_cast<const unsigned int*>(buf + (lds - s));
            unsigned int w = lw[0];
            if (s) w = (w >> (8 * s)) | (lw[1] << (32 - 8 * s));       // lw[1] holds byte k + 3 of the row: inside the buffer
            *reinterpret_cast<unsigned int*>(p.dst + A) = w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (k + t >= 0 && k + t < nb) p.dst[g0 + k + t] = rowp[k + t];
        }
    }
}

// One box pass along one line.  s / d: the line's position 0 in the source / destination buffer, `step` bytes between positions.  Computes
// positions [cs, ce) (inside the page), then copies the value at cs to [lo, cs) and the value at ce - 1 to [ce, hi) (beyond the page border).
// Reads positions [cs - r - 1, ce + r + 1) of the source.
__device__ __forceinline__ void pf_box_line(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, int step, int lo, int hi, int cs, int ce,
                                            int r, unsigned int ww, unsigned int fw) {
    unsigned int sum = 0;
#pragma clang loop vectorize(disable)
    for (int t = -r; t <= r; t++) sum += s[(cs + t) * step];
    unsigned int e_lo = s[(cs - r - 1) * step];
    unsigned int first = 0, out = 0;
    const unsigned char* sl = s + (cs - r) * step;                     // leaves the sum when the box moves on
    const unsigned char* sh = s + (cs + r + 1) * step;                 // upper outermost pixel; enters the sum when the box moves on
    unsigned char* dp = d + cs * step;
#pragma unroll 4
    for (int x = cs; x < ce; x++) {
        const unsigned int e_hi = *sh, n_lo = *sl;
        out = (__umul24(ww, sum) + __umul24(fw, e_lo + e_hi) + (1u << 23)) >> 24;  // 24-bit operands: the full-rate multiply
        *dp = (unsigned char)out;
        if (x == cs) first = out;
        sum += e_hi - n_lo;
        e_lo = n_lo;
        sl += step; sh += step; dp += step;
    }
#pragma clang loop vectorize(disable)
    for (int x = lo; x < cs; x++) d[x * step] = (unsigned char)first;
#pragma clang loop vectorize(disable)
    for (int x = ce; x < hi; x++) d[x * step] = (unsigned char)out;
}

// grid (ceil(W / PF_TILE), ceil(H / PF_TILE), images); dynamic LDS 2 * (PF_TILE + 2 halo) * pitch
__global__ __launch_bounds__(PF_THREADS) void page_blur_kernel(PageFilterParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pf_lds[];
    const int x0 = blockIdx.x * PF_TILE, y0 = blockIdx.y * PF_TILE;
    const long img = blockIdx.z;
    const int tw = min(PF_TILE, p.W - x0), th = min(PF_TILE, p.H - y0);
    const int h = p.halo, r = p.r, q = r + 1;
    const int rows = th + 2 * h, cols = tw + 2 * h;
    const int gx0 = x0 - h, gy0 = y0 - h;                              // page coordinates of local (0, 0)
    unsigned char* A = pf_lds;
    unsigned char* B = pf_lds + (PF_TILE + 2 * h) * p.pitch;
    pf_stage(p, A, img, gy0, gx0, rows, cols);
    __syncthreads();
    // local positions inside the page: columns [cx0, cx1), rows [cy0, cy1)
    const int cx0 = max(0, -gx0), cx1 = min(cols, p.W - gx0);
    const int cy0 = max(0, -gy0), cy1 = min(rows, p.H - gy0);
    unsigned char* s = A;
    unsigned char* d = B;
    for (int k = 1; k <= 3; k++) {                                     // x passes over every staged row; window [k q, cols - k q)
        const int lo = k * q, hi = cols - k * q;
        for (int i = threadIdx.x; i < rows * 3; i += PF_THREADS) {
            const int row = i / 3, c = i - row * 3;
            const int off = row * p.pitch + c;
            pf_box_line(s + off, d + off, 3, lo, hi, max(lo, cx0), min(hi, cx1), r, p.ww, p.fw);
        }
        __syncthreads();
        unsigned char* t = s; s = d; d = t;
    }
    for (int k = 1; k <= 3; k++) {                                     // y passes over the tile's columns; window [k q, rows - k q)
        const int lo = k * q, hi = rows - k * q;
        for (int i = threadIdx.x; i < tw * 3; i += PF_THREADS) {
            const int off = h * 3 + i;
            pf_box_line(s + off, d + off, p.pitch, lo, hi, max(lo, cy0), min(hi, cy1), r, p.ww, p.fw);
        }
        __syncthreads();
        unsigned char* t = s; s = d; d = t;
    }
    pf_store(p, s, h * p.pitch + h * 3, img, y0, x0, th, tw);          // s: the sixth pass's output; its window is the tile
}

// grid as above; static LDS: staged tile + 1-pixel halo (re-used for the output), grey plane
__global__ __launch_bounds__(PF_THREADS) void page_edge_kernel(PageFilterParams p) {
    constexpr int L = PF_TILE + 2, GP = PF_TILE + 4;                   // grey plane pitch
    __shared__ __attribute__((aligned(16))) unsigned char buf[L * (((L * 3 + 3) >> 2 | 1) * 4)];
    __shared__ unsigned char grey[L * GP];
    const int x0 = blockIdx.x * PF_TILE, y0 = blockIdx.y * PF_TILE;
    const long img = blockIdx.z;
    const int tw = min(PF_TILE, p.W - x0), th = min(PF_TILE, p.H - y0);
    const int rows = th + 2, cols = tw + 2;
    pf_stage(p, buf, img, y0 - 1, x0 - 1, rows, cols);
    __syncthreads();
    for (int i = threadIdx.x; i < rows * cols; i += PF_THREADS) {
        const int ly = i / cols, lx = i - ly * cols;
        const unsigned char* px = buf + ly * p.pitch + lx * 3;
        grey[ly * GP + lx] = (unsigned char)((19595u * px[0] + 38470u * px[1] + 7471u * px[2] + 32768u) >> 16);
    }
    __syncthreads();                                                   // every grey is computed: buf may now take the output (tile row ty at buf row ty)
    for (int i = threadIdx.x; i < th * tw; i += PF_THREADS) {
        const int ty = i / tw, tx = i - ty * tw;
        const int gy = y0 + ty, gx = x0 + tx;
        const unsigned char* g = grey + (ty + 1) * GP + tx + 1;
        int v = g[0];
        if (gy > 0 && gy < p.H - 1 && gx > 0 && gx < p.W - 1) {
            const int sum = g[-GP - 1] + g[-GP] + g[-GP + 1] + g[-1] + g[0] + g[1] + g[GP - 1] + g[GP] + g[GP + 1];
            v = clampi(9 * v - sum, 0, 255);
        }
        unsigned char* o = buf + ty * p.pitch + tx * 3;
        o[0] = o[1] = o[2] = (unsigned char)v;
    }
    __syncthreads();
    pf_store(p, buf, 0, img, y0, x0, th, tw);
}

// Pillow's _gaussian_blur_radius(radius, 3) and ImagingLineBoxBlur's weights.  sigma2, L, l, a are C floats there: sqrt and floor are taken in double
// and rounded on assignment, the rest is float arithmetic (volatile: no contraction, no wider intermediates).
static void box_params(float radius, int* r_out, unsigned int* ww_out, unsigned int* fw_out) {
    volatile float sigma2 = radius * radius / 3;
    volatile float L = (float)sqrt(12.0 * sigma2 + 1.0);
    volatile float l = (float)floor((L - 1.0) / 2.0);
    volatile float t0 = 2 * l + 1, t1 = l * (l + 1), t2 = 3 * sigma2, t3 = t1 - t2;
    volatile float a = t0 * t3;
    volatile float t4 = (l + 1) * (l + 1), t5 = sigma2 - t4, t6 = 6 * t5;
    a = a / t6;
    volatile float fr = l + a;
    const int r = (int)fr;
    volatile float den = fr * 2 + 1;
    volatile float quot = (float)(1 << 24) / den;
    const unsigned int ww = (unsigned int)quot;
    *r_out = r; *ww_out = ww; *fw_out = ((1u << 24) - (2u * r + 1u) * ww) / 2;
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_page_filter_u8(const uint8_t* src, uint8_t* dst, int64_t images, int H, int W, int kind, float radius, void* stream) {
    LDETR_CHECK(src && dst, "page_filter: null pointer");
    LDETR_CHECK(images >= 0 && H > 0 && W > 0, "page_filter: bad shape");
    LDETR_CHECK(kind == LDETR_PAGE_FILTER_BLUR || kind == LDETR_PAGE_FILTER_EDGE, "page_filter: kind must be 1 (blur) or 2 (edge)");
    LDETR_CHECK(images <= 65535 && cdiv(H, PF_TILE) <= 65535, "page_filter: grid limit (images, rows / %d <= 65535)", PF_TILE);
    LDETR_CHECK((((uintptr_t)src) & 3) == 0 && (((uintptr_t)dst) & 3) == 0, "page_filter: src and dst must be 4-byte aligned");
    if (kind == LDETR_PAGE_FILTER_BLUR) LDETR_CHECK(radius > 0.f && radius <= 5.f, "page_filter: blur radius must be in (0, 5]");
    const int64_t bytes = images * (int64_t)H * W * 3;
    LDETR_CHECK((uintptr_t)src + (uintptr_t)bytes <= (uintptr_t)dst || (uintptr_t)dst + (uintptr_t)bytes <= (uintptr_t)src,
                "page_filter: src and dst overlap");
    if (images == 0) return LDETR_OK;
    PageFilterParams p; memset(&p, 0, sizeof(p));
    p.src = src; p.dst = dst; p.bytes = bytes; p.H = H; p.W = W;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(W, PF_TILE), cdiv(H, PF_TILE), (unsigned)images);
    if (kind == LDETR_PAGE_FILTER_EDGE) {
        p.halo = 1; p.pitch = pf_pitch(1);
        hipLaunchKernelGGL(page_edge_kernel, grid, PF_THREADS, 0, st, p);
        return check_launch("page_edge");
    }
    box_params(radius, &p.r, &p.ww, &p.fw);
    if (p.ww >= (1u << 24))                                             // radius so small that the box is one pixel of weight 1: every pass is the identity
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess ? LDETR_OK : check_launch("page_blur copy");
    LDETR_CHECK(p.r >= 0 && 3 * (p.r + 1) <= PF_MAX_HALO, "page_filter: box radius %d out of range", p.r);
    p.halo = 3 * (p.r + 1); p.pitch = pf_pitch(p.halo);
    const int lds = 2 * (PF_TILE + 2 * p.halo) * p.pitch;
    hipLaunchKernelGGL(page_blur_kernel, grid, PF_THREADS, lds, st, p);
    return check_launch("page_blur");
}
