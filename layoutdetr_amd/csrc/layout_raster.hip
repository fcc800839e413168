// Snapshot grids of layouts, rendered on the device: what the reference's save_image does per sample on the host (util.py:85-141)
//     convert_layout_to_image: boxes sorted by area, one ImageDraw.rectangle(outline, fill with alpha 100) each on a page-sized canvas   util.py:85-103
//     PIL resize to the canvas size (BILINEAR), expand2square                                                                            util.py:105-112, 71-82
//     ToTensor, torch.stack, torchvision make_grid(padding=2) + save_image                                                               util.py:123-141
// (and, as ldetr_image_raster_u8, the compositing half of save_real_image / save_real_image_with_background, util.py:144-325: see the kernel's comment)
// as ONE launch per grid: every cell, the letterbox bars and the grid padding are written here (no memset before the launch), and the
// page-resolution image never exists in HBM.  Integer arithmetic end to end, so the grid is bit-identical to the reference's PNG pixels.
//
// Rule: boxes in stable descending order of a = w * h (fp32); corners (xc -+ w / 2) * W, (yc -+ h / 2) * H in fp32, one IEEE
// operation each (no fma contraction), truncated toward zero after clamping to the int32 range, swapped where reversed; the rectangle covers
// X1 <= x <= X2, Y1 <= y <= Y2: its border pixels take the label's colour, its interior blends with alpha 100 as Pillow's 8-bit blend does
// (t = c * 100 + d * 155 + 128; d = ((t >> 8) + t) >> 8).  Invalid slots and boxes whose area or any corner is NaN are skipped.  The page is
// resized with Pillow's two-pass 8-bit resampling (triangle window; the tables are ldetr_resample_coeffs_filter's), a pass whose sizes agree
// is skipped, and the result is letterboxed into an S x S cell of the grid.
//
// Work layout: a workgroup owns one cell and a band of R output rows (and the padding above / left of them; the last column / row of cells
// also owns the right / bottom padding).  It sorts the cell's boxes into LDS (at most 16 entries, read as broadcasts: no dynamically indexed
// registers), then forms the source rows its band needs -- procedural for a white page (the rule above per source pixel), or read from the
// uint8 page and drawn over -- a few at a time in a 16 KiB LDS row buffer, runs the horizontal pass over them into a uint8 LDS intermediate
// (44 KiB), and finally the vertical pass straight into the grid.
// What bounds it: R is sized on the host so that the intermediate rows of a band (about R * H / Hn + 2 * support, Wn * 3 bytes each) fit the
// 44 KiB; with the row buffer and the box list a workgroup holds just under 61 KiB of the CU's 160 KiB of LDS, so two workgroups stay resident.
// The work is byte and integer arithmetic (per source pixel up to 16 box tests, per output pixel ~2 * scale multiply-adds per pass): bound by
// instruction issue, like resample.hip, not by memory -- the only HBM traffic is the page bytes (if any) and the grid itself.
#include <limits.h>
#include <math.h>

#include <vector>

#include "ldetr_common.hpp"
#include "pil_resample.hpp"

#pragma clang fp contract(off)

namespace ldetr {

constexpr int LR_THREADS = 256;
constexpr int LR_MAX_N = 16;
constexpr int LR_CELL_INTS = 32;          // per-cell descriptor, see the host entry
constexpr int LR_IMAGE_CELL_INTS = 128;   // the image kinds' descriptor: the same head, then (x1, y1, x2, y2, offset low, offset high) per slot from int 32
constexpr int LR_HBUF_BYTES = 44 * 1024;  // horizontal-pass rows of a band
constexpr int LR_SRC_BYTES = 16 * 1024;   // source rows in flight
constexpr int LR_MAX_BAND = 32;

struct LayoutRasterParams {
    const float* bbox; const unsigned char* pages; const int* coeffs; const int* cells; unsigned char* out;
    int B, N, S, xmaps, ymaps, pad, Hg, Wg;
};

__device__ __forceinline__ int lr_trunc(float f) {
    if (f >= 2147483648.f) return INT_MAX;
    if (f <= -2147483648.f) return INT_MIN;
    return f == f ? (int)f : 0;                                      // (a NaN corner: the box is skipped, the value is never used)
}
__device__ __forceinline__ unsigned lr_blend(unsigned c, unsigned d) {
    const unsigned t = c * 100u + d * 155u + 128u;
    return ((t >> 8) + t) >> 8;
}

// grid (bands, xmaps * ymaps).  IMAGE (ldetr_image_raster_u8, util.py:144-325): the page is not drawn with rectangles but pasted with resized text
// patches -- per source pixel the LAST element in draw order whose clipped paste rectangle [x1, x2) x [y1, y2) covers it gives the pixel, read from
// its resized patch in `pages` (here the output buffer of ldetr_patch_resize_u8); otherwise the resized background or white.  The sort, the two
// 8-bit passes, the letterbox and the grid tail are the same code.
template <bool IMAGE>
__global__ __launch_bounds__(LR_THREADS) void layout_raster_kernel(LayoutRasterParams p) {
    __shared__ unsigned char hbuf[LR_HBUF_BYTES];
    __shared__ unsigned char sbuf[LR_SRC_BYTES];
    __shared__ int bx[LR_MAX_N][4];
    __shared__ unsigned bcol[LR_MAX_N];
    __shared__ float barea[LR_MAX_N];
    __shared__ int bok[LR_MAX_N];
    __shared__ long boff[IMAGE ? LR_MAX_N : 1];
    constexpr int CI = IMAGE ? LR_IMAGE_CELL_INTS : LR_CELL_INTS;
    const int slot = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const int S = p.S, P = p.pad;
    const bool live = slot < p.B;                                   // the last grid row may have empty slots: written as zeros
    const int* cell = p.cells + (long)(live ? slot : 0) * CI;
    const int R = live ? cell[13] : S;
    if (band * R >= S) return;
    const int cy = slot / p.xmaps, cx = slot % p.xmaps;
    const int y0 = band * R, y1 = min(y0 + R, S);
    const int W = cell[0], H = cell[1], Wn = cell[2], Hn = cell[3], ox = cell[4], oy = cell[5];
    const long page_off = get_i64(cell + 6);                          // < 0: white page
    const int hoff = cell[8], voff = cell[10];                        // < 0: the pass is skipped
    const int ys = live ? max(y0 - oy, 0) : 0, ye = live ? min(y1 - oy, Hn) : 0;   // rows of the resized page in this band
    int rlo = 0;
    if (ys < ye) {
        // 1. the cell's boxes, sorted, into LDS
        int X1 = 0, Y1 = 0, X2 = 0, Y2 = 0, ok = 0;
        float a = 0.f;
        if (tid < LR_MAX_N) {
            if (tid < p.N && ((cell[12] >> tid) & 1)) {
                const float* b = p.bbox + ((long)slot * p.N + tid) * 4;
                const float xc = b[0], yc = b[1], w = b[2], h = b[3];
                a = w * h;
                if constexpr (IMAGE) {
                    const int* e = cell + 32 + 6 * tid;
                    ok = !(a != a);
                    X1 = e[0]; Y1 = e[1]; X2 = e[2]; Y2 = e[3];
                } else {
                    const float fx1 = (xc - w / 2.f) * (float)W, fx2 = (xc + w / 2.f) * (float)W;
                    const float fy1 = (yc - h / 2.f) * (float)H, fy2 = (yc + h / 2.f) * (float)H;
                    ok = !(a != a || fx1 != fx1 || fx2 != fx2 || fy1 != fy1 || fy2 != fy2);
                    X1 = lr_trunc(fx1); X2 = lr_trunc(fx2); Y1 = lr_trunc(fy1); Y2 = lr_trunc(fy2);
                    if (X1 > X2) { const int t = X1; X1 = X2; X2 = t; }
                    if (Y1 > Y2) { const int t = Y1; Y1 = Y2; Y2 = t; }
                }
            }
            bok[tid] = ok; barea[tid] = a;
        }
        __syncthreads();
        if (tid < LR_MAX_N) {
            if (ok) {
                int rank = 0;
                for (int j = 0; j < LR_MAX_N; j++) rank += (bok[j] && (barea[j] > a || (barea[j] == a && j < tid))) ? 1 : 0;
                bx[rank][0] = X1; bx[rank][1] = Y1; bx[rank][2] = X2; bx[rank][3] = Y2;
                if constexpr (IMAGE) boff[rank] = get_i64(cell + 32 + 6 * tid + 4);
                else bcol[rank] = (unsigned)cell[16 + tid];
            }
        }
        __syncthreads();
        int nb = 0;
        for (int j = 0; j < LR_MAX_N; j++) nb += bok[j];
        // 2. source rows [rlo, rhi) -> horizontal pass -> hbuf
        const int* vb = p.coeffs + (voff < 0 ? 0 : voff);
        rlo = voff < 0 ? ys : vb[2 * ys];
        int rhi = voff < 0 ? ye : vb[2 * (ye - 1)] + vb[2 * (ye - 1) + 1];
        rhi = min(min(rhi, H), rlo + LR_HBUF_BYTES / (Wn * 3));       // (never binds: the host sized R for it)
        const int chunk = hoff < 0 ? rhi - rlo : max(1, min(LR_SRC_BYTES / (W * 3), rhi - rlo));
        unsigned char* dst = hoff < 0 ? hbuf : sbuf;
        const int* hb = p.coeffs + (hoff < 0 ? 0 : hoff);
        const int* hk = hb + 2 * Wn;
        for (int r0 = rlo; r0 < rhi; r0 += chunk) {
            const int nr = min(chunk, rhi - r0);
            if (hoff >= 0 && r0 > rlo) __syncthreads();                // the previous chunk's horizontal pass has read sbuf
            for (int i = tid; i < nr * W; i += LR_THREADS) {
                const int y = r0 + i / W, x = i % W;
                unsigned d0 = 255u, d1 = 255u, d2 = 255u;
                if (page_off >= 0) {
                    const unsigned char* px = p.pages + page_off + ((long)y * W + x) * 3;
                    d0 = px[0]; d1 = px[1]; d2 = px[2];
                }
                if constexpr (IMAGE) {
                    for (int k = nb - 1; k >= 0; k--) {
                        const int bX1 = bx[k][0], bY1 = bx[k][1], bX2 = bx[k][2], bY2 = bx[k][3];
                        if (x < bX1 || x >= bX2 || y < bY1 || y >= bY2) continue;
                        const unsigned char* px = p.pages + boff[k] + ((long)(y - bY1) * (bX2 - bX1) + (x - bX1)) * 3;
                        d0 = px[0]; d1 = px[1]; d2 = px[2];
                        break;
                    }
                } else {
                    for (int k = 0; k < nb; k++) {
                        const int bX1 = bx[k][0], bY1 = bx[k][1], bX2 = bx[k][2], bY2 = bx[k][3];
                        if (x < bX1 || x > bX2 || y < bY1 || y > bY2) continue;
                        const unsigned c = bcol[k], c0 = c & 255u, c1 = (c >> 8) & 255u, c2 = (c >> 16) & 255u;
                        if (x == bX1 || x == bX2 || y == bY1 || y == bY2) { d0 = c0; d1 = c1; d2 = c2; }
                        else { d0 = lr_blend(c0, d0); d1 = lr_blend(c1, d1); d2 = lr_blend(c2, d2); }
                    }
                }
                unsigned char* o = dst + i * 3;
                o[0] = (unsigned char)d0; o[1] = (unsigned char)d1; o[2] = (unsigned char)d2;
            }
            if (hoff >= 0) {
                __syncthreads();
                for (int i = tid; i < nr * Wn; i += LR_THREADS) {
                    const int row = i / Wn, xx = i % Wn;
                    const int xmin = hb[2 * xx], cnt = hb[2 * xx + 1];
                    int a0 = PIL_HALF, a1 = a0, a2 = a0;
                    pil_taps3<3>(sbuf + (row * W + xmin) * 3, 0, hk, Wn, xx, cnt, a0, a1, a2);
                    unsigned char* o = hbuf + ((r0 - rlo + row) * Wn + xx) * 3;
                    o[0] = (unsigned char)pil_clip8(a0); o[1] = (unsigned char)pil_clip8(a1); o[2] = (unsigned char)pil_clip8(a2);
                }
            }
        }
        __syncthreads();
    }
    // 3. vertical pass + letterbox + padding: every pixel this workgroup owns
    const int ylo = band == 0 ? -P : y0, yhi = y1 + ((y1 == S && cy == p.ymaps - 1) ? P : 0);
    const int xlo = -P, xhi = S + (cx == p.xmaps - 1 ? P : 0);
    const int nc = xhi - xlo;
    const int* vb = p.coeffs + (voff < 0 ? 0 : voff);
    const int* vk = vb + 2 * Hn;
    for (int i = tid; i < (yhi - ylo) * nc; i += LR_THREADS) {
        const int y = ylo + i / nc, x = xlo + i % nc;
        const int gy = P + cy * (S + P) + y, gx = P + cx * (S + P) + x;
        if (gy < 0 || gy >= p.Hg || gx < 0 || gx >= p.Wg) continue;
        const int yy = y - oy, xx = x - ox;
        int v0 = 0, v1 = 0, v2 = 0;
        if (yy >= ys && yy < ye && xx >= 0 && xx < Wn) {
            if (voff < 0) {
                const unsigned char* px = hbuf + ((yy - rlo) * Wn + xx) * 3;
                v0 = px[0]; v1 = px[1]; v2 = px[2];
            } else {
                const int ymin = vb[2 * yy], cnt = vb[2 * yy + 1];
                int a0 = PIL_HALF, a1 = a0, a2 = a0;
                pil_taps3<0>(hbuf + ((ymin - rlo) * Wn + xx) * 3, Wn * 3, vk, Hn, yy, cnt, a0, a1, a2);
                v0 = pil_clip8(a0); v1 = pil_clip8(a1); v2 = pil_clip8(a2);
            }
        }
        unsigned char* o = p.out + ((long)gy * p.Wg + gx) * 3;
        o[0] = (unsigned char)v0; o[1] = (unsigned char)v1; o[2] = (unsigned char)v2;
    }
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_layout_raster_cell_size(int W, int H, int S, int* wn_out, int* hn_out) {
    LDETR_CHECK(wn_out && hn_out, "layout_raster_cell_size: null output");
    LDETR_CHECK(W >= 1 && H >= 1 && S >= 1, "layout_raster_cell_size: page and canvas sizes must be positive (got %d x %d -> %d)", W, H, S);
    if (W > H) { *wn_out = S; *hn_out = (int)((double)H / (double)W * (double)S) / 2 * 2; }
    else { *hn_out = S; *wn_out = (int)((double)W / (double)H * (double)S) / 2 * 2; }
    return LDETR_OK;
}

// the part of a cell's descriptor both entries share: resized size, letterbox offsets, coefficient tables, band height (c[0..5], c[8..11], c[13])
static int lr_cell_geometry(const char* who, int b, int W, int H, int S, const int64_t* cc, int64_t coeffs_len, int32_t* c, int* bands) {
    LDETR_CHECK(W >= 1 && H >= 1 && W < (1 << 24) && H < (1 << 24), "%s: cell %d: bad page size %d x %d", who, b, W, H);
    int Wn, Hn;
    ldetr_layout_raster_cell_size(W, H, S, &Wn, &Hn);
    LDETR_CHECK(Wn >= 1 && Hn >= 1, "%s: cell %d: page %d x %d leaves no pixel at canvas size %d", who, b, W, H, S);
    LDETR_CHECK((long)W * 3 <= LR_SRC_BYTES, "%s: cell %d: page wider than %d pixels", who, b, LR_SRC_BYTES / 3);
    const bool hskip = W == Wn, vskip = H == Hn;
    LDETR_CHECK(hskip ? cc[0] < 0 : (cc[0] >= 0 && cc[1] >= 1 && cc[0] + (2 + cc[1]) * Wn <= coeffs_len),
                "%s: cell %d: horizontal coefficient table outside the pool (or given for a skipped pass)", who, b);
    LDETR_CHECK(vskip ? cc[2] < 0 : (cc[2] >= 0 && cc[3] >= 1 && cc[2] + (2 + cc[3]) * Hn <= coeffs_len),
                "%s: cell %d: vertical coefficient table outside the pool (or given for a skipped pass)", who, b);
    // band height: the intermediate rows of a band must fit LR_HBUF_BYTES
    const long cap = LR_HBUF_BYTES / ((long)Wn * 3);
    const double scale = (double)H / Hn, support = scale < 1.0 ? 1.0 : scale;
    int R = LR_MAX_BAND;
    auto rows = [&](int r) { return vskip ? (long)r : (long)ceil(r * scale + 2.0 * support) + 2; };
    while (R > 1 && rows(R) > cap) R--;
    LDETR_CHECK(rows(R) <= cap, "%s: cell %d: page %d x %d too tall for one band of the canvas", who, b, W, H);
    c[0] = W; c[1] = H; c[2] = Wn; c[3] = Hn;
    c[4] = W > H ? 0 : (S - Wn) / 2; c[5] = W > H ? (S - Hn) / 2 : 0;
    c[8] = hskip ? -1 : (int32_t)cc[0]; c[9] = hskip ? 0 : (int32_t)cc[1];
    c[10] = vskip ? -1 : (int32_t)cc[2]; c[11] = vskip ? 0 : (int32_t)cc[3];
    c[13] = R;
    const int nb = (S + R - 1) / R;
    if (nb > *bands) *bands = nb;
    return LDETR_OK;
}

// Both raster entries: the shared checks, make_grid's layout (rule 7), one descriptor per cell, its upload and the launch.  `what` names a slot in
// the messages; `check()` holds an entry's own argument checks; `fill(b, W, H, c, off, mask)` writes a cell's kind-specific words into c and
// gives the byte offset of its page (-1: white) and the mask of the slots it draws.
template <bool IMAGE, typename Args, typename Check, typename Fill>
static int lr_raster(const char* who, const char* what, const Args* a, const uint8_t* pages, void* stream, Check check, Fill fill) {
    constexpr int CI = IMAGE ? LR_IMAGE_CELL_INTS : LR_CELL_INTS;
    const int B = a->B, N = a->N, S = a->S;
    LDETR_CHECK(B >= 0, "%s: negative B (got %d)", who, B);
    LDETR_CHECK(N >= 1 && N <= LR_MAX_N, "%s: needs 1 <= N <= 16 %s per layout (got %d)", who, what, N);
    LDETR_CHECK(S >= 2 && S % 2 == 0 && S <= 4096, "%s: the canvas size must be even and in [2, 4096] (got %d)", who, S);
    if (B == 0) return LDETR_OK;
    LDETR_CHECK(a->bbox && a->valid && a->page_wh && a->cell_coeffs && a->coeffs && a->cells_dev && a->out, "%s: null pointer", who);
    if (int rc = check()) return rc;
    int xmaps = 1, ymaps = 1, pad = 0;
    if (B > 1) {
        const int nrow = a->nrow > 0 ? a->nrow : (int)ceil(sqrt((double)B));
        xmaps = nrow < B ? nrow : B; ymaps = (B + xmaps - 1) / xmaps; pad = 2;
    }
    const long Hg = (long)ymaps * (S + pad) + pad, Wg = (long)xmaps * (S + pad) + pad;
    LDETR_CHECK(Hg * Wg * 3 < (1L << 31) && (long)xmaps * ymaps <= 65535, "%s: grid too large (%ld x %ld)", who, Hg, Wg);
    static thread_local std::vector<int32_t> cells;                    // outlives the call: the upload below reads it
    cells.assign((size_t)B * CI, 0);
    int bands = 1;
    for (int b = 0; b < B; b++) {
        int32_t* c = cells.data() + (size_t)b * CI;
        const int W = a->page_wh[2 * b], H = a->page_wh[2 * b + 1];
        if (int rc = lr_cell_geometry(who, b, W, H, S, a->cell_coeffs + 4 * (long)b, a->coeffs_len, c, &bands)) return rc;
        int64_t off = -1;
        unsigned mask = 0;
        if (int rc = fill(b, W, H, c, off, mask)) return rc;
        put_i64(c + 6, off);
        c[12] = (int32_t)mask;
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = upload_descriptors(who, a->cells_dev, cells.data(), cells.size(), st)) return rc;
    LayoutRasterParams p; memset(&p, 0, sizeof(p));
    p.bbox = a->bbox; p.pages = pages; p.coeffs = a->coeffs; p.cells = a->cells_dev; p.out = a->out;
    p.B = B; p.N = N; p.S = S; p.xmaps = xmaps; p.ymaps = ymaps; p.pad = pad; p.Hg = (int)Hg; p.Wg = (int)Wg;
    hipLaunchKernelGGL(layout_raster_kernel<IMAGE>, dim3((unsigned)bands, (unsigned)(xmaps * ymaps)), LR_THREADS, 0, st, p);
    return check_launch(who);
}

extern "C" int ldetr_layout_raster_u8(const ldetr_layout_raster_args* a, void* stream) {
    LDETR_CHECK_BLOCK(a, ldetr_layout_raster_args, "layout_raster");
    auto check = [&]() {
        LDETR_CHECK(a->labels && a->palette, "layout_raster: null pointer");
        LDETR_CHECK(a->n_colors >= 1, "layout_raster: empty palette");
        LDETR_CHECK(a->n_pages >= 0 && (a->n_pages == 0 || (a->pages && a->page_table && a->page_index)), "layout_raster: pages given without buffer, table or index");
        return LDETR_OK;
    };
    auto fill = [&](int b, int W, int H, int32_t* c, int64_t& off, unsigned& mask) {
        const int N = a->N, pi = a->n_pages > 0 ? a->page_index[b] : -1;
        LDETR_CHECK(pi >= -1 && pi < a->n_pages, "layout_raster: cell %d: page index %d outside the page table (%d pages)", b, pi, a->n_pages);
        if (pi >= 0) {
            const int64_t* t = a->page_table + 3 * (long)pi;
            LDETR_CHECK(t[1] == W && t[2] == H, "layout_raster: cell %d: page %d is %ld x %ld, the cell says %d x %d", b, pi, (long)t[1], (long)t[2], W, H);
            LDETR_CHECK(t[0] >= 0 && t[0] + (int64_t)W * H * 3 <= a->pages_bytes, "layout_raster: cell %d: page %d reaches past the page buffer", b, pi);
            off = t[0];
        }
        for (int i = 0; i < N; i++) {
            if (!a->valid[(long)b * N + i]) continue;
            const int lab = a->labels[(long)b * N + i];
            LDETR_CHECK(lab >= 0 && lab < a->n_colors, "layout_raster: cell %d: label %d outside the palette (%d colours)", b, lab, a->n_colors);
            mask |= 1u << i;
            c[16 + i] = a->palette[3 * lab] | (a->palette[3 * lab + 1] << 8) | (a->palette[3 * lab + 2] << 16);
        }
        return LDETR_OK;
    };
    return lr_raster<false>("layout_raster", "boxes", a, a->pages, stream, check, fill);
}

extern "C" int ldetr_image_raster_u8(const ldetr_image_raster_args* a, void* stream) {
    LDETR_CHECK_BLOCK(a, ldetr_image_raster_args, "image_raster");
    auto check = [&]() {
        LDETR_CHECK(a->rects && a->patch_off && a->page_off, "image_raster: null pointer");
        LDETR_CHECK(a->pixels_bytes >= 0 && (a->pixels || a->pixels_bytes == 0), "image_raster: pixel buffer size without buffer");
        return LDETR_OK;
    };
    auto fill = [&](int b, int W, int H, int32_t* c, int64_t& off, unsigned& mask) {
        const int N = a->N;
        off = a->page_off[b];
        LDETR_CHECK(off >= -1 && (off < 0 || off + (int64_t)W * H * 3 <= a->pixels_bytes), "image_raster: cell %d: resized background reaches past the pixel buffer", b);
        for (int i = 0; i < N; i++) {
            if (!a->valid[(long)b * N + i]) continue;
            const int32_t* r = a->rects + ((long)b * N + i) * 4;           // the UNCLIPPED paste rectangle: the patch is (y2 - y1) x (x2 - x1)
            if (r[2] <= r[0] || r[3] <= r[1] || r[2] <= 0 || r[3] <= 0 || r[0] >= W || r[1] >= H) continue;      // draws nothing
            const int64_t po = a->patch_off[(long)b * N + i];
            LDETR_CHECK(po >= 0 && po + ((int64_t)r[3] - r[1]) * ((int64_t)r[2] - r[0]) * 3 <= a->pixels_bytes,
                        "image_raster: cell %d: the resized patch of slot %d reaches past the pixel buffer", b, i);
            mask |= 1u << i;
            int32_t* e = c + 32 + 6 * i;
            e[0] = r[0]; e[1] = r[1]; e[2] = r[2]; e[3] = r[3];             // (the kernel only visits page pixels: that is the clip)
            put_i64(e + 4, po);
        }
        return LDETR_OK;
    };
    return lr_raster<true>("image_raster", "elements", a, a->pixels, stream, check, fill);
}
