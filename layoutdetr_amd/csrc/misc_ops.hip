// HBM-bound helper kernels around the contraction engine: fused elementwise + per-(sample, channel)
// reductions for the modulated-conv / bias_act backward, NHWC max-pool, toRGB backward.
// All tensors are row-major [rows][C] with C contiguous (NHWC pixels are rows).
#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"
#include <type_traits>

namespace ldetr {

enum { RR_COLSUM = 0, RR_ACTGRAD = 1, RR_MULRED = 2 };

struct RRParams {
    const float* a; const float* b; float* out;
    const float* colv;   // [C]
    const float* sampv;  // [B][C]
    float* red1; long red1_bs;
    float* red2; long red2_bs;
    float* part;         // [2][blocks][C] partial sums instead of atomics (finished by rr_finish_kernel), or NULL
    long P; int B, C, mode, act, rows_pb;
    float alpha, gain;
};

// Block = 256 threads = TQ channel-quads x RL row lanes.  grid = (row chunks, B, channel chunks).
template <int MODE>
__global__ __launch_bounds__(256) void rowreduce_kernel(RRParams p) {
    __shared__ float4 sh1[256];
    __shared__ float4 sh2[256];
    const int C4 = p.C >> 2;
    const int TQ = C4 < 256 ? C4 : 256;
    const int RL = 256 / TQ;
    const int tx = threadIdx.x % TQ, ty = threadIdx.x / TQ;
    const int cq = blockIdx.z * TQ + tx;
    const int b = blockIdx.y;
    const bool active = (ty < RL) && (cq < C4);
    float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = r1;
    if (active) {
        const int c = cq << 2;
        float4 cv = make_float4(0.f, 0.f, 0.f, 0.f), sv = make_float4(1.f, 1.f, 1.f, 1.f);
        if (p.colv) cv = *reinterpret_cast<const float4*>(p.colv + c);
        if (p.sampv) sv = *reinterpret_cast<const float4*>(p.sampv + (long)b * p.C + c);
        const long r0 = (long)blockIdx.x * p.rows_pb;
        const long r1e = min(p.P, r0 + p.rows_pb);
        auto process = [&](const float4& a, const float4& x2, long off) {
            if (MODE == RR_COLSUM) {
                r1.x += a.x; r1.y += a.y; r1.z += a.z; r1.w += a.w;
            } else if (MODE == RR_ACTGRAD) {
                // a = dy, x2 = y (saved output).  dv = dy * gain * (y > 0 ? 1 : alpha)   [act 2: lrelu, 1: relu, 0: linear]
                const float4& y = x2;
                float4 dv;
                float gp = p.gain, gn = (p.act == 2) ? p.gain * p.alpha : (p.act == 1 ? 0.f : p.gain);
                dv.x = a.x * (y.x > 0.f ? gp : gn); dv.y = a.y * (y.y > 0.f ? gp : gn);
                dv.z = a.z * (y.z > 0.f ? gp : gn); dv.w = a.w * (y.w > 0.f ? gp : gn);
                if (p.out) *reinterpret_cast<float4*>(p.out + off) = dv;
                r1.x += dv.x; r1.y += dv.y; r1.z += dv.z; r1.w += dv.w;
                if (p.red2) {
                    // pre-activation v = y/gain (y > 0) or y/(gain*alpha); u*d = v - bias; red2 += dv * (v - bias) / d
                    float ip = 1.f / gp, in = (gn != 0.f) ? 1.f / gn : 0.f;
                    float vx = y.x * (y.x > 0.f ? ip : in) - cv.x, vy = y.y * (y.y > 0.f ? ip : in) - cv.y;
                    float vz = y.z * (y.z > 0.f ? ip : in) - cv.z, vw = y.w * (y.w > 0.f ? ip : in) - cv.w;
                    r2.x += dv.x * vx / sv.x; r2.y += dv.y * vy / sv.y; r2.z += dv.z * vz / sv.z; r2.w += dv.w * vw / sv.w;
                }
            } else {  // RR_MULRED: out = a * sampv (optional), red1 += a * b
                if (p.out) {
                    float4 o = make_float4(a.x * sv.x, a.y * sv.y, a.z * sv.z, a.w * sv.w);
                    *reinterpret_cast<float4*>(p.out + off) = o;
                }
                r1.x += a.x * x2.x; r1.y += a.y * x2.y; r1.z += a.z * x2.z; r1.w += a.w * x2.w;
            }
        };
        // four rows per trip, all loads issued before the first store (the output may alias an input, so the compiler
        // cannot hoist them itself): 8 float4 loads in flight per lane
        constexpr int UN = 4;
        for (long r = r0 + ty; r < r1e; r += (long)RL * UN) {
            float4 av[UN], bv[UN];
#pragma unroll
            for (int u = 0; u < UN; u++) {
                const long rr = r + (long)u * RL;
                if (rr < r1e) {
                    const long off = ((long)b * p.P + rr) * p.C + c;
                    av[u] = *reinterpret_cast<const float4*>(p.a + off);
                    if (MODE != RR_COLSUM) bv[u] = *reinterpret_cast<const float4*>(p.b + off);
                }
            }
#pragma unroll
            for (int u = 0; u < UN; u++) {
                const long rr = r + (long)u * RL;
                if (rr < r1e) process(av[u], bv[u], ((long)b * p.P + rr) * p.C + c);
            }
        }
    }
    sh1[threadIdx.x] = r1; sh2[threadIdx.x] = r2;
    __syncthreads();
    if (active && ty == 0) {
        for (int j = 1; j < RL; j++) {
            float4 t = sh1[j * TQ + tx]; r1.x += t.x; r1.y += t.y; r1.z += t.z; r1.w += t.w;
            float4 u = sh2[j * TQ + tx]; r2.x += u.x; r2.y += u.y; r2.z += u.z; r2.w += u.w;
        }
        const int c = cq << 2;
        if (p.part) {
            const long nblk = (long)gridDim.x * gridDim.y, blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
            *reinterpret_cast<float4*>(p.part + blk * p.C + c) = r1;
            if (p.red2) *reinterpret_cast<float4*>(p.part + (nblk + blk) * p.C + c) = r2;
            return;
        }
        if (p.red1) {
            float* d = p.red1 + (long)b * p.red1_bs + c;
            atomicAdd(d, r1.x); atomicAdd(d + 1, r1.y); atomicAdd(d + 2, r1.z); atomicAdd(d + 3, r1.w);
        }
        if (p.red2) {
            float* d = p.red2 + (long)b * p.red2_bs + c;
            atomicAdd(d, r2.x); atomicAdd(d + 1, r2.y); atomicAdd(d + 2, r2.z); atomicAdd(d + 3, r2.w);
        }
    }
}

// Second stage of the row reductions: red[b][c] += sum over the row chunks' partial sums (all samples' chunks when the
// reduction is shared by the batch, bs == 0), for up to RR_MAX_PLANES partial planes [planes][blocks][C] of one first-stage launch.
// No long same-address atomic queues: with one atomic per block and channel the first stage's time was (#blocks x ~0.1 us)
// whatever the bandwidth; here at most `segs` (<= 16) atomics meet per address.
// grid (ceil(C / 64), B or 1, planes * segs): z / segs = plane; z % segs = slice of the partial rows.
// Block = 64 channels x 4 partial-row lanes.
enum { RR_MAX_PLANES = 6 };
struct RRFinish {
    float* red[RR_MAX_PLANES]; long bs[RR_MAX_PLANES];   // plane i -> red[i][b * bs[i] + c]; a NULL plane is skipped
    const float* part; int B, C;
};

__global__ __launch_bounds__(256) void rr_finish_kernel(RRFinish f, int chunks, int segs) {
    __shared__ float sh[256];
    const int which = blockIdx.z / segs, seg = blockIdx.z % segs;
    float* red = nullptr; long bs = 0;
#pragma unroll
    for (int i = 0; i < RR_MAX_PLANES; i++) if (which == i) { red = f.red[i]; bs = f.bs[i]; }
    if (!red) return;
    const bool shared_by_batch = bs == 0;
    if (shared_by_batch && blockIdx.y > 0) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), lane = threadIdx.x >> 6;
    const long nblk = (long)chunks * f.B;
    const float* part = f.part + (long)which * nblk * f.C;
    const long first = shared_by_batch ? 0 : (long)blockIdx.y * chunks, count = shared_by_batch ? nblk : chunks;
    const long per = (count + segs - 1) / segs, i0 = seg * per, i1 = min(count, i0 + per);
    float acc = 0.f;
    if (c < f.C) {
#pragma unroll 4
        for (long i = i0 + lane; i < i1; i += 4) acc += part[(first + i) * f.C + c];
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (lane == 0 && c < f.C && i0 < i1) {
        acc += sh[threadIdx.x + 64] + sh[threadIdx.x + 128] + sh[threadIdx.x + 192];
        float* d = red + (shared_by_batch ? 0 : (long)blockIdx.y * bs) + c;
        if (segs > 1) atomicAdd(d, acc); else *d += acc;
    }
}

// Row-chunk plan shared by the streaming reductions: a few blocks per CU in total, never straddling a sample.
static dim3 rr_grid(int B, long P, int C, int* rows_pb_out) {
    const int C4 = C / 4;
    const int TQ = C4 < 256 ? C4 : 256;
    const int RL = 256 / TQ;
    static const long target = 2048;
    const long groups = (long)B * cdiv(C4, TQ);
    long chunks = target / groups; if (chunks < 1) chunks = 1;
    long rows_pb = (P + chunks - 1) / chunks;
    const long min_rows = (long)RL * 4;
    if (rows_pb < min_rows) rows_pb = min_rows;
    rows_pb = (rows_pb + RL - 1) / RL * RL;
    *rows_pb_out = (int)rows_pb;
    return dim3((unsigned)((P + rows_pb - 1) / rows_pb), B, cdiv(C4, TQ));
}

static int launch_rr_finish(const RRFinish& f, int planes, int chunks, long sharers, hipStream_t st) {
    int segs = (int)(sharers / 32); if (segs < 1) segs = 1; if (segs > 16) segs = 16;
    hipLaunchKernelGGL(rr_finish_kernel, dim3(cdiv(f.C, 64), f.B, planes * segs), 256, 0, st, f, chunks, segs);
    return check_launch("rowreduce_finish");
}

static int launch_rr(RRParams& p, hipStream_t st) {
    // their partial sums go through the workspace to rr_finish_kernel
    const dim3 grid = rr_grid(p.B, p.P, p.C, &p.rows_pb);
    const long nblk = (long)grid.x * grid.y;
    // atomics queue up per output cache line: 32 per block and line at ~5 ns each, i.e. ~0.16 us per sharing block -- cheaper than
    // the ~4.5 us of a second launch up to ~30 sharers (measured: 48 us vs 10 us at 256 sharers); beyond that the partial sums go
    // through the workspace to rr_finish_kernel
    const long sharers = p.red1 && p.red1_bs == 0 ? nblk : (long)grid.x;     // blocks adding into one output element
    p.part = (p.red1 || p.red2) && sharers > 32 ? scratch_alloc((size_t)nblk * p.C * sizeof(float) * (p.red2 ? 2 : 1)) : nullptr;
    if (p.mode == RR_COLSUM) hipLaunchKernelGGL(rowreduce_kernel<RR_COLSUM>, grid, 256, 0, st, p);
    else if (p.mode == RR_ACTGRAD) hipLaunchKernelGGL(rowreduce_kernel<RR_ACTGRAD>, grid, 256, 0, st, p);
    else hipLaunchKernelGGL(rowreduce_kernel<RR_MULRED>, grid, 256, 0, st, p);
    int rc = check_launch("rowreduce"); if (rc || !p.part) return rc;
    RRFinish f; memset(&f, 0, sizeof(f));
    f.red[0] = p.red1; f.bs[0] = p.red1_bs; f.red[1] = p.red2; f.bs[1] = p.red2_bs; f.part = p.part; f.B = p.B; f.C = p.C;
    return launch_rr_finish(f, p.red2 ? 2 : 1, (int)grid.x, sharers, st);
}

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 2 / pad 1 max-pool on NHWC (torchvision ResNet stem; reference: detr_backbone.py:105).
struct PoolParams {
    const float* x; float* y; unsigned char* idx; const float* dy; float* dx;
    int N, H, W, C, OH, OW;
};

__global__ __launch_bounds__(256) void maxpool_fwd_kernel(PoolParams p) {
    const int C4 = p.C >> 2;
    const long total = (long)p.N * p.OH * p.OW * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) << 2; long t = i / C4;
        int ox = (int)(t % p.OW); t /= p.OW;
        int oy = (int)(t % p.OH); int n = (int)(t / p.OH);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        // the index starts at the window's first in-image tap (row 1 / column 1 of a border window), as F.max_pool2d's does: a window whose
        // in-image elements are all -inf then routes its gradient there and not to a tap outside the image
        const unsigned char k0 = (unsigned char)((oy == 0 ? 3 : 0) + (ox == 0 ? 1 : 0));
        uchar4 mi = make_uchar4(k0, k0, k0, k0);
#pragma unroll
        for (int kh = 0; kh < 3; kh++) {
            int y = oy * 2 - 1 + kh;
            if (y < 0 || y >= p.H) continue;
#pragma unroll
            for (int kw = 0; kw < 3; kw++) {
                int x = ox * 2 - 1 + kw;
                if (x < 0 || x >= p.W) continue;
                float4 v = *reinterpret_cast<const float4*>(p.x + (((long)n * p.H + y) * p.W + x) * p.C + c);
                unsigned char k = (unsigned char)(kh * 3 + kw);
                if (v.x > m.x || v.x != v.x) { m.x = v.x; mi.x = k; }
                if (v.y > m.y || v.y != v.y) { m.y = v.y; mi.y = k; }
                if (v.z > m.z || v.z != v.z) { m.z = v.z; mi.z = k; }
                if (v.w > m.w || v.w != v.w) { m.w = v.w; mi.w = k; }
            }
        }
        long o = (((long)n * p.OH + oy) * p.OW + ox) * p.C + c;
        *reinterpret_cast<float4*>(p.y + o) = m;
        if (p.idx) *reinterpret_cast<uchar4*>(p.idx + o) = mi;
    }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(PoolParams p) {
    const int C4 = p.C >> 2;
    const long total = (long)p.N * p.H * p.W * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int c = (int)(i % C4) << 2; long t = i / C4;
        int x = (int)(t % p.W); t /= p.W;
        int y = (int)(t % p.H); int n = (int)(t / p.H);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        int oy0 = y >> 1, oy1 = (y + 1) >> 1;  // windows with oy*2-1 <= y <= oy*2+1
        int ox0 = x >> 1, ox1 = (x + 1) >> 1;
        for (int oy = oy0; oy <= oy1; oy++) {
            if (oy >= p.OH) continue;
            for (int ox = ox0; ox <= ox1; ox++) {
                if (ox >= p.OW) continue;
                unsigned char k = (unsigned char)((y - (oy * 2 - 1)) * 3 + (x - (ox * 2 - 1)));
                long o = (((long)n * p.OH + oy) * p.OW + ox) * p.C + c;
                uchar4 mi = *reinterpret_cast<const uchar4*>(p.idx + o);
                float4 d = *reinterpret_cast<const float4*>(p.dy + o);
                if (mi.x == k) g.x += d.x;
                if (mi.y == k) g.y += d.y;
                if (mi.z == k) g.z += d.z;
                if (mi.w == k) g.w += d.w;
            }
        }
        *reinterpret_cast<float4*>(p.dx + (((long)n * p.H + y) * p.W + x) * p.C + c) = g;
    }
}

// ---------------------------------------------------------------------------------------------
// toRGB (1x1 modulated conv to 3 channels, no demodulation) backward:
//   dx[b,p,c]     = s[b,c] * sum_co dy[b,p,co] * w[co,c]
//   dws[b,co,c]  += sum_p dy[b,p,co] * x[b,p,c]          (per-sample; host folds in styles / weights)
//   dbias[co]    += sum_{b,p} dy[b,p,co]
struct RgbParams {
    const float* x; const float* dy; const float* w; const float* s;
    float* dx; float* dws; float* dbias;
    long P; int B, C, rows_pb;
};

__global__ __launch_bounds__(256) void torgb_bwd_kernel(RgbParams p) {
    __shared__ float4 sh[3][256];
    const int C4 = p.C >> 2;
    const int TQ = C4 < 256 ? C4 : 256;
    const int RL = 256 / TQ;
    const int tx = threadIdx.x % TQ, ty = threadIdx.x / TQ;
    const int cq = blockIdx.z * TQ + tx;
    const int b = blockIdx.y;
    const bool active = (ty < RL) && (cq < C4);
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0;
    float db0 = 0.f, db1 = 0.f, db2 = 0.f;
    if (active) {
        const int c = cq << 2;
        const float4 w0 = *reinterpret_cast<const float4*>(p.w + c);
        const float4 w1 = *reinterpret_cast<const float4*>(p.w + p.C + c);
        const float4 w2 = *reinterpret_cast<const float4*>(p.w + 2 * p.C + c);
        const float4 sv = *reinterpret_cast<const float4*>(p.s + (long)b * p.C + c);
        const long r0 = (long)blockIdx.x * p.rows_pb;
        const long r1e = min(p.P, r0 + p.rows_pb);
        for (long r = r0 + ty; r < r1e; r += RL) {
            const long row = (long)b * p.P + r;
            const float d0 = p.dy[row * 3], d1 = p.dy[row * 3 + 1], d2 = p.dy[row * 3 + 2];
            const float4 xv = *reinterpret_cast<const float4*>(p.x + row * p.C + c);
            float4 o;
            o.x = sv.x * (d0 * w0.x + d1 * w1.x + d2 * w2.x); o.y = sv.y * (d0 * w0.y + d1 * w1.y + d2 * w2.y);
            o.z = sv.z * (d0 * w0.z + d1 * w1.z + d2 * w2.z); o.w = sv.w * (d0 * w0.w + d1 * w1.w + d2 * w2.w);
            *reinterpret_cast<float4*>(p.dx + row * p.C + c) = o;
            a0.x += d0 * xv.x; a0.y += d0 * xv.y; a0.z += d0 * xv.z; a0.w += d0 * xv.w;
            a1.x += d1 * xv.x; a1.y += d1 * xv.y; a1.z += d1 * xv.z; a1.w += d1 * xv.w;
            a2.x += d2 * xv.x; a2.y += d2 * xv.y; a2.z += d2 * xv.z; a2.w += d2 * xv.w;
            if (cq == 0) { db0 += d0; db1 += d1; db2 += d2; }
        }
    }
    sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1; sh[2][threadIdx.x] = a2;
    __syncthreads();
    if (active && ty == 0) {
        for (int j = 1; j < RL; j++) {
            float4 t0 = sh[0][j * TQ + tx], t1 = sh[1][j * TQ + tx], t2 = sh[2][j * TQ + tx];
            a0.x += t0.x; a0.y += t0.y; a0.z += t0.z; a0.w += t0.w;
            a1.x += t1.x; a1.y += t1.y; a1.z += t1.z; a1.w += t1.w;
            a2.x += t2.x; a2.y += t2.y; a2.z += t2.z; a2.w += t2.w;
        }
        const int c = cq << 2;
        float* d = p.dws + (long)b * 3 * p.C + c;
        atomicAdd(d, a0.x); atomicAdd(d + 1, a0.y); atomicAdd(d + 2, a0.z); atomicAdd(d + 3, a0.w);
        d += p.C;
        atomicAdd(d, a1.x); atomicAdd(d + 1, a1.y); atomicAdd(d + 2, a1.z); atomicAdd(d + 3, a1.w);
        d += p.C;
        atomicAdd(d, a2.x); atomicAdd(d + 1, a2.y); atomicAdd(d + 2, a2.z); atomicAdd(d + 3, a2.w);
    }
    // bias gradient: the block's row lanes are summed through LDS first, so one block issues 3 atomics instead of 3 x RL onto the
    // same cache line (at 256^2 x 16 samples that queue of 65536 same-line atomics WAS the kernel: 340 us)
    if (p.dbias && blockIdx.z == 0) {
        __syncthreads();
        float* f = reinterpret_cast<float*>(&sh[0][0]);
        if (tx == 0 && ty < RL) { f[ty * 3] = db0; f[ty * 3 + 1] = db1; f[ty * 3 + 2] = db2; }
        __syncthreads();
        if (threadIdx.x < 3) {
            float t = 0.f;
            for (int j = 0; j < RL; j++) t += f[j * 3 + threadIdx.x];
            atomicAdd(p.dbias + threadIdx.x, t);
        }
    }
}

// Second stage of the toRGB backward: dws [B][3][C] = per-sample sums of dy x (x unmodulated) ->
//   dw[o][c] += sum_b dws[b][o][c] * s[b][c]   (accumulated: dw is the flat .grad view or a zero-filled temporary)
//   ds[b][c]  = sum_o dws[b][o][c] * w[o][c]
// (the reference's autograd forms both with broadcast multiplies and reductions: 4 launches + 2 accumulations per layer)
__global__ __launch_bounds__(256) void torgb_finish_kernel(const float* __restrict__ dws, const float* __restrict__ s, const float* __restrict__ w,
                                                           float* __restrict__ dw, float* __restrict__ ds, int B, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 3 * C) {
        const int c = i % C;
        float a = 0.f;
        for (int b = 0; b < B; b++) a += dws[(long)b * 3 * C + i] * s[(long)b * C + c];
        dw[i] += a;
    }
    if (i < B * C) {
        const int b = i / C, c = i - b * C;
        const float* d = dws + (long)b * 3 * C + c;
        ds[i] = d[0] * w[c] + d[C] * w[C + c] + d[2 * C] * w[2 * C + c];
    }
}

// ---------------------------------------------------------------------------------------------
// StyleGAN2 synthesis backward, the hand-off between two contraction launches (training/networks_stylegan2.py:307-326, :349-353): the
// producer layer's saved output x is at once the tensor the consumer conv's style gradient multiplies against, the toRGB's input and the
// carrier of the lrelu sign, so  dxs -> * s_conv -> (+ toRGB's dx) -> * gain * lrelu'(x)  is ONE pass over two tensors:
//   dv[b,p,c]       = (dxs * s_conv[b][c] + s_rgb[b][c] * sum_k dy[b,p,k] * w_rgb[k][c]) * (x > 0 ? gain : gain * alpha)
//   ds_conv[b][c]  += sum_p dxs * x                      (CONV)
//   dws[b][k][c]   += sum_p dy[b,p,k] * x                (RGB; finished by torgb_finish_kernel)
//   dbias_rgb[k]   += sum_{b,p} dy[b,p,k]                (RGB)
//   dbias[c]       += sum_{b,p} dv
//   ddemod[b][c]   += sum_p dv * (pre(x) - bias[c]) / demod[b][c]        (the formula of RR_ACTGRAD; only when ddemod != NULL)
// toRGB's dx (three FMAs per element from a 3-channel gradient) and the styled dx never exist in memory.  Thread layout and trip shape of
// rowreduce_kernel; partial planes in the order ds_conv, dws[0..2], dbias, ddemod (those present).
struct HandoffParams {
    const float* dxs; const float* x; const float* dy; float* dv;
    const float* s_conv; const float* s_rgb; const float* w_rgb; const float* bias; const float* demod;
    float* ds_conv; float* dws; float* dbias_rgb; float* dbias; float* ddemod;
    float* part;         // [planes][blocks][C] partial sums instead of atomics (finished by rr_finish_kernel), or NULL
    long P; int B, C, rows_pb;
    float gp, gn;        // slope for x > 0 and for x <= 0, activation gain included
};

static __device__ __forceinline__ void f4_fma(float4& acc, float s, const float4& v) {
    acc.x += s * v.x; acc.y += s * v.y; acc.z += s * v.z; acc.w += s * v.w;
}
static __device__ __forceinline__ void f4_add(float4& acc, const float4& v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }

template <bool CONV, bool RGB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CONV && RGB ? 4 : 5))) void sg2_handoff_kernel(HandoffParams p) {
    __shared__ float4 sh[3][256];
    __shared__ float4 shw[3][256];      // s_rgb[b][c] * w_rgb[k][c] of the block's channel quads: read per row, 12 registers less held per lane
    const int C4 = p.C >> 2;
    const int TQ = C4 < 256 ? C4 : 256;
    const int RL = 256 / TQ;
    const int tx = threadIdx.x % TQ, ty = threadIdx.x / TQ;
    const int cq = blockIdx.z * TQ + tx;
    const int b = blockIdx.y;
    const bool active = (ty < RL) && (cq < C4);
    const bool dd = p.ddemod != nullptr;
    if (RGB) {
        if (active && ty == 0) {
            const int c = cq << 2;
            const float4 sr = *reinterpret_cast<const float4*>(p.s_rgb + (long)b * p.C + c);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float4 w = *reinterpret_cast<const float4*>(p.w_rgb + (long)k * p.C + c);
                shw[k][tx] = make_float4(sr.x * w.x, sr.y * w.y, sr.z * w.z, sr.w * w.w);
            }
        }
        __syncthreads();
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rs = zero, rb = zero, rd = zero, a0 = zero, a1 = zero, a2 = zero;
    float db0 = 0.f, db1 = 0.f, db2 = 0.f;
    if (active) {
        const int c = cq << 2;
        float4 sc = zero;
        if (CONV) sc = *reinterpret_cast<const float4*>(p.s_conv + (long)b * p.C + c);
        const float gp = p.gp, gn = p.gn;
        const float ip = 1.f / gp, in = (gn != 0.f) ? 1.f / gn : 0.f;
        // the block's rows [r0, r0 + nrows) of sample b: one 64-bit base per tensor (uniform) + an unsigned 32-bit byte offset per lane (the
        // host checks that a chunk of rows_pb x C floats stays below 2^32 bytes): no 64-bit address arithmetic in registers
        const long r0 = (long)blockIdx.x * p.rows_pb;
        const int nrows = (int)(min(p.P, r0 + p.rows_pb) - r0);
        const long base = ((long)b * p.P + r0) * p.C;
        const char* xb = reinterpret_cast<const char*>(p.x + base);
        const char* ab = CONV ? reinterpret_cast<const char*>(p.dxs + base) : nullptr;
        const char* yb = RGB ? reinterpret_cast<const char*>(p.dy + ((long)b * p.P + r0) * 3) : nullptr;
        char* ob = reinterpret_cast<char*>(p.dv + base);
        const unsigned rowb = (unsigned)p.C * 4u, cb = (unsigned)c * 4u;
        // four rows per trip, all loads issued before the first store (dv may alias dxs); full trips carry no bounds test at all, the chunk's
        // last rows (fewer than 4 x RL) go one per trip
        auto trip = [&](int r, auto un) {
            constexpr int UN = decltype(un)::value;
            float4 av[UN], xv[UN];
            float d0[UN], d1[UN], d2[UN];
#pragma unroll
            for (int u = 0; u < UN; u++) {
                // row r + u * RL: the u * RL rows go into the (uniform) base, so the four rows share one offset register per tensor
                const unsigned off = (unsigned)r * rowb + cb, yo = (unsigned)r * 12u;
                const size_t ub = (size_t)(u * RL) * rowb, uy = (size_t)(u * RL) * 12u;
                if (CONV) av[u] = *reinterpret_cast<const float4*>(ab + ub + off);
                xv[u] = *reinterpret_cast<const float4*>(xb + ub + off);
                if (RGB) {
                    d0[u] = *reinterpret_cast<const float*>(yb + uy + yo); d1[u] = *reinterpret_cast<const float*>(yb + uy + 4 + yo);
                    d2[u] = *reinterpret_cast<const float*>(yb + uy + 8 + yo);
                }
            }
#pragma unroll
            for (int u = 0; u < UN; u++) {
                // rows are consumed one after the other: left to itself the scheduler interleaves the four rows (and their twelve LDS reads
                // each) for ILP this HBM-bound loop has no use for, at 30 registers and one wave per SIMD
                __builtin_amdgcn_sched_barrier(0);
                const float4& x = xv[u];
                float4 g = zero;
                if (RGB) {
                    // (the index passes through an empty asm so that the three reads stay here and are not hoisted back into registers)
                    int wi = tx;
                    asm volatile("" : "+v"(wi));
                    f4_fma(g, d0[u], shw[0][wi]); f4_fma(g, d1[u], shw[1][wi]); f4_fma(g, d2[u], shw[2][wi]);
                    f4_fma(a0, d0[u], x); f4_fma(a1, d1[u], x); f4_fma(a2, d2[u], x);
                    db0 += d0[u]; db1 += d1[u]; db2 += d2[u];        // (every lane sums them; the first channel quad's are used)
                }
                if (CONV) {
                    const float4& a = av[u];
                    g.x += a.x * sc.x; g.y += a.y * sc.y; g.z += a.z * sc.z; g.w += a.w * sc.w;
                    rs.x += a.x * x.x; rs.y += a.y * x.y; rs.z += a.z * x.z; rs.w += a.w * x.w;
                }
                float4 dv;
                // (both products, then the choice: the slopes stay scalar operands instead of four registers held for the selects)
                dv.x = x.x > 0.f ? g.x * gp : g.x * gn; dv.y = x.y > 0.f ? g.y * gp : g.y * gn;
                dv.z = x.z > 0.f ? g.z * gp : g.z * gn; dv.w = x.w > 0.f ? g.w * gp : g.w * gn;
                *reinterpret_cast<float4*>(ob + (size_t)(u * RL) * rowb + ((unsigned)r * rowb + cb)) = dv;
                f4_add(rb, dv);
                // pre-activation v = x / gain (x > 0) or x / (gain * alpha); u * d = v - bias.  rd sums dv * v here; "- bias * sum dv" and the
                // division by d follow once per block below (sum dv is rb).  Summed whether or not ddemod is wanted: a few VALU operations
                // under the loads, no branch in the loop.
                rd.x += dv.x * (x.x > 0.f ? x.x * ip : x.x * in); rd.y += dv.y * (x.y > 0.f ? x.y * ip : x.y * in);
                rd.z += dv.z * (x.z > 0.f ? x.z * ip : x.z * in); rd.w += dv.w * (x.w > 0.f ? x.w * ip : x.w * in);
            }
        };
        int r = ty;
#pragma nounroll
        for (; r + 3 * RL < nrows; r += 4 * RL) trip(r, std::integral_constant<int, 4>());
#pragma nounroll
        for (; r < nrows; r += RL) trip(r, std::integral_constant<int, 1>());
    }
    const bool lead = active && ty == 0;
    const int c = cq << 2;
    const long nblk = (long)gridDim.x * gridDim.y, blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    // one plane's block sum -> its partial plane, or atomics into red[b * bs + c]
    auto emit = [&](const float4& v, int plane, float* red, long bs) {
        if (p.part) { *reinterpret_cast<float4*>(p.part + ((long)plane * nblk + blk) * p.C + c) = v; return; }
        float* d = red + (long)b * bs + c;
        atomicAdd(d, v.x); atomicAdd(d + 1, v.y); atomicAdd(d + 2, v.z); atomicAdd(d + 3, v.w);
    };
    // the row lanes' sums meet through LDS, three planes at a time
    if (RGB) {
        sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1; sh[2][threadIdx.x] = a2;
        __syncthreads();
        if (lead) {
            for (int j = 1; j < RL; j++) { f4_add(a0, sh[0][j * TQ + tx]); f4_add(a1, sh[1][j * TQ + tx]); f4_add(a2, sh[2][j * TQ + tx]); }
            const int pl = CONV ? 1 : 0;
            emit(a0, pl, p.dws, 3L * p.C); emit(a1, pl + 1, p.dws + p.C, 3L * p.C); emit(a2, pl + 2, p.dws + 2 * p.C, 3L * p.C);
        }
        __syncthreads();
    }
    sh[0][threadIdx.x] = rs; sh[1][threadIdx.x] = rb; sh[2][threadIdx.x] = rd;
    __syncthreads();
    if (lead) {
        for (int j = 1; j < RL; j++) { f4_add(rs, sh[0][j * TQ + tx]); f4_add(rb, sh[1][j * TQ + tx]); f4_add(rd, sh[2][j * TQ + tx]); }
        const int pl = (CONV ? 1 : 0) + (RGB ? 3 : 0);
        if (CONV) emit(rs, 0, p.ds_conv, p.C);
        emit(rb, pl, p.dbias, 0);
        if (dd) {
            const float4 dmv = *reinterpret_cast<const float4*>(p.demod + (long)b * p.C + c);
            const float4 cv = p.bias ? *reinterpret_cast<const float4*>(p.bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            rd.x = (rd.x - cv.x * rb.x) / dmv.x; rd.y = (rd.y - cv.y * rb.y) / dmv.y;
            rd.z = (rd.z - cv.z * rb.z) / dmv.z; rd.w = (rd.w - cv.w * rb.w) / dmv.w;
            emit(rd, pl + 1, p.ddemod, p.C);
        }
    }
    // toRGB's bias gradient: the block's row lanes are summed through LDS first, one block issues 3 atomics (see torgb_bwd_kernel)
    if (RGB && blockIdx.z == 0) {
        __syncthreads();
        float* f = reinterpret_cast<float*>(&sh[0][0]);
        if (tx == 0 && ty < RL) { f[ty * 3] = db0; f[ty * 3 + 1] = db1; f[ty * 3 + 2] = db2; }
        __syncthreads();
        if (threadIdx.x < 3) {
            float t = 0.f;
            for (int j = 0; j < RL; j++) t += f[j * 3 + threadIdx.x];
            atomicAdd(p.dbias_rgb + threadIdx.x, t);
        }
    }
}

template <bool CONV, bool RGB>
static int launch_handoff(HandoffParams& p, hipStream_t st) {
    const dim3 grid = rr_grid(p.B, p.P, p.C, &p.rows_pb);
    LDETR_CHECK((long)p.rows_pb * p.C < (1L << 30), "sg2_handoff: a row chunk of %d x %d floats exceeds the kernel's 32-bit offsets", p.rows_pb, p.C);
    const long nblk = (long)grid.x * grid.y;            // dbias is shared by the batch: every block of a channel chunk adds into it
    const int planes = (CONV ? 1 : 0) + (RGB ? 3 : 0) + 1 + (p.ddemod ? 1 : 0);
    p.part = nblk > 32 ? scratch_alloc((size_t)planes * nblk * p.C * sizeof(float)) : nullptr;
    hipLaunchKernelGGL((sg2_handoff_kernel<CONV, RGB>), grid, 256, 0, st, p);
    int rc = check_launch("sg2_handoff"); if (rc || !p.part) return rc;
    RRFinish f; memset(&f, 0, sizeof(f));
    int i = 0;
    if (CONV) { f.red[i] = p.ds_conv; f.bs[i++] = p.C; }
    if (RGB) for (int k = 0; k < 3; k++) { f.red[i] = p.dws + (long)k * p.C; f.bs[i++] = 3L * p.C; }
    f.red[i] = p.dbias; f.bs[i++] = 0;
    if (p.ddemod) { f.red[i] = p.ddemod; f.bs[i++] = p.C; }
    f.part = p.part; f.B = p.B; f.C = p.C;
    return launch_rr_finish(f, planes, (int)grid.x, nblk, st);
}

}  // namespace ldetr

using namespace ldetr;

static int rr_common(RRParams& p, const char* what) {
    LDETR_CHECK(p.a, "%s: null pointer", what);
    LDETR_CHECK(p.C % 4 == 0 && p.C > 0, "%s: C must be a positive multiple of 4", what);
    LDETR_CHECK(p.B > 0 && p.P >= 0, "%s: bad shape", what);
    return LDETR_OK;
}

// red[b][c] += sum_p a[b,p,c]   (B = 1 gives a plain column sum).  red must be pre-zeroed by the caller.
extern "C" int ldetr_colsum_f32(const float* a, float* red, int B, int64_t P, int C, void* stream) {
    RRParams p; memset(&p, 0, sizeof(p));
    p.a = a; p.red1 = red; p.red1_bs = C; p.B = B; p.P = P; p.C = C; p.mode = RR_COLSUM;
    int rc = rr_common(p, "colsum"); if (rc) return rc;
    if (P == 0) return LDETR_OK;
    return launch_rr(p, (hipStream_t)stream);
}

// bias_act first-derivative fused with its reductions (reference: bias_act.py:166-171 does dx then dx.sum()):
//   dv = dy * gain * (y > 0 ? 1 : alpha)      act: 0 linear, 1 relu, 2 lrelu
//   dbias[c]     += sum_{b,p} dv
//   ddemod[b][c] += sum_p dv * (pre(y) - bias[c]) / demod[b][c]      (only when ddemod != NULL)
extern "C" int ldetr_act_bwd_reduce_f32(const float* dy, const float* y, float* dv, const float* bias, const float* demod,
                                        float* dbias, float* ddemod, int B, int64_t P, int C, int act, float alpha, float gain,
                                        void* stream) {
    RRParams p; memset(&p, 0, sizeof(p));
    p.a = dy; p.b = y; p.out = dv; p.colv = bias; p.sampv = demod; p.red1 = dbias; p.red1_bs = 0;
    p.red2 = ddemod; p.red2_bs = C; p.B = B; p.P = P; p.C = C; p.mode = RR_ACTGRAD; p.act = act; p.alpha = alpha; p.gain = gain;
    int rc = rr_common(p, "act_bwd_reduce"); if (rc) return rc;
    LDETR_CHECK(y, "act_bwd_reduce: y is required");
    LDETR_CHECK(!ddemod || demod, "act_bwd_reduce: ddemod needs demod");
    if (P == 0) return LDETR_OK;
    return launch_rr(p, (hipStream_t)stream);
}

//   out[b,p,c] = a[b,p,c] * scale[b][c]   (skipped when out == NULL)
//   red[b][c] += sum_p a[b,p,c] * x[b,p,c]
extern "C" int ldetr_mul_reduce_f32(const float* a, const float* x, const float* scale, float* out, float* red,
                                    int B, int64_t P, int C, void* stream) {
    RRParams p; memset(&p, 0, sizeof(p));
    p.a = a; p.b = x; p.out = out; p.sampv = scale; p.red1 = red; p.red1_bs = C; p.B = B; p.P = P; p.C = C; p.mode = RR_MULRED;
    int rc = rr_common(p, "mul_reduce"); if (rc) return rc;
    LDETR_CHECK(x, "mul_reduce: x is required");
    if (P == 0) return LDETR_OK;
    return launch_rr(p, (hipStream_t)stream);
}

extern "C" int ldetr_maxpool3x3s2_fwd_f32(const float* x, float* y, unsigned char* idx, int N, int H, int W, int C, void* stream) {
    LDETR_CHECK(x && y, "maxpool_fwd: null pointer");
    LDETR_CHECK(C % 4 == 0, "maxpool_fwd: C must be a multiple of 4");
    PoolParams p; memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.idx = idx; p.N = N; p.H = H; p.W = W; p.C = C; p.OH = (H + 2 - 3) / 2 + 1; p.OW = (W + 2 - 3) / 2 + 1;
    long total = (long)N * p.OH * p.OW * (C / 4);
    int grid = (int)((total + 255) / 256); if (grid > 8192) grid = 8192; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(maxpool_fwd_kernel, grid, 256, 0, (hipStream_t)stream, p);
    return check_launch("maxpool_fwd");
}

extern "C" int ldetr_maxpool3x3s2_bwd_f32(const float* dy, const unsigned char* idx, float* dx, int N, int H, int W, int C, void* stream) {
    LDETR_CHECK(dy && idx && dx, "maxpool_bwd: null pointer");
    LDETR_CHECK(C % 4 == 0, "maxpool_bwd: C must be a multiple of 4");
    PoolParams p; memset(&p, 0, sizeof(p));
    p.dy = dy; p.idx = const_cast<unsigned char*>(idx); p.dx = dx; p.N = N; p.H = H; p.W = W; p.C = C;
    p.OH = (H + 2 - 3) / 2 + 1; p.OW = (W + 2 - 3) / 2 + 1;
    long total = (long)N * H * W * (C / 4);
    int grid = (int)((total + 255) / 256); if (grid > 8192) grid = 8192; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(maxpool_bwd_kernel, grid, 256, 0, (hipStream_t)stream, p);
    return check_launch("maxpool_bwd");
}

namespace ldetr {
// ToRGBLayer forward (networks_stylegan2.py:349-353: modulated 1x1 convolution to 3 colour channels, no demodulation, + bias):
//   y[b][p][o] = bias[o] + sum_c x[b][p][c] * w[o][c] * s[b][c]
// One read of x, 12 bytes written per pixel: HBM-bound.  LPP = min(C / 4, 64) lanes share a pixel (a float4 of channels each, C / 4 / LPP
// trips), their three partial dot products meet through xor shuffles.  On the contraction engine this launch pads 3 output channels to a
// 64-wide tile: 144 us at 16 x 256 x 256 x 32 for 134 MB.
struct RgbFwdParams { const float* x; const float* w; const float* s; const float* bias; float* y; long P; int B, C; const float* add; };   // add [B][P][3] or NULL: y = add + (conv + bias), the skip connection

template <int LPP>
__global__ __launch_bounds__(256) void torgb_fwd_kernel(RgbFwdParams p) {
    const int lane_in = threadIdx.x % LPP;
    const long pix_per_block = 256 / LPP;
    const int C4 = p.C >> 2;
    const int b = blockIdx.y;
    const float* sb = p.s + (long)b * p.C;
    // the (sample-scaled) weights this lane needs, for up to two trips (C <= 512)
    float4 w0[2], w1[2], w2[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int cq = lane_in + t * LPP;
        if (cq < C4) {
            const float4 sv = *reinterpret_cast<const float4*>(sb + 4 * cq);
            float4 a = *reinterpret_cast<const float4*>(p.w + 4 * cq), bq = *reinterpret_cast<const float4*>(p.w + p.C + 4 * cq), c = *reinterpret_cast<const float4*>(p.w + 2 * p.C + 4 * cq);
            w0[t] = make_float4(a.x * sv.x, a.y * sv.y, a.z * sv.z, a.w * sv.w);
            w1[t] = make_float4(bq.x * sv.x, bq.y * sv.y, bq.z * sv.z, bq.w * sv.w);
            w2[t] = make_float4(c.x * sv.x, c.y * sv.y, c.z * sv.z, c.w * sv.w);
        } else { w0[t] = w1[t] = w2[t] = make_float4(0.f, 0.f, 0.f, 0.f); }
    }
    const float b0 = p.bias ? p.bias[0] : 0.f, b1 = p.bias ? p.bias[1] : 0.f, b2 = p.bias ? p.bias[2] : 0.f;
    const long stride = (long)gridDim.x * pix_per_block;
    for (long r = (long)blockIdx.x * pix_per_block + threadIdx.x / LPP; r < p.P; r += stride) {
        const float* xr = p.x + ((long)b * p.P + r) * p.C;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int cq = lane_in + t * LPP;
            if (cq < C4) {
                const float4 xv = *reinterpret_cast<const float4*>(xr + 4 * cq);
                d0 += xv.x * w0[t].x + xv.y * w0[t].y + xv.z * w0[t].z + xv.w * w0[t].w;
                d1 += xv.x * w1[t].x + xv.y * w1[t].y + xv.z * w1[t].z + xv.w * w1[t].w;
                d2 += xv.x * w2[t].x + xv.y * w2[t].y + xv.z * w2[t].z + xv.w * w2[t].w;
            }
        }
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) { d0 += __shfl_xor(d0, o, 64); d1 += __shfl_xor(d1, o, 64); d2 += __shfl_xor(d2, o, 64); }
        if (lane_in == 0) {
            float* yr = p.y + ((long)b * p.P + r) * 3;
            float y0 = d0 + b0, y1 = d1 + b1, y2 = d2 + b2;
            if (p.add) {   // one more rounded add per value: what `img + y` after this launch computes
                const float* ar = p.add + ((long)b * p.P + r) * 3;
                y0 = __fadd_rn(ar[0], y0); y1 = __fadd_rn(ar[1], y1); y2 = __fadd_rn(ar[2], y2);
            }
            yr[0] = y0; yr[1] = y1; yr[2] = y2;
        }
    }
}
}  // namespace ldetr

// x [B][P][C] (NHWC pixels), w [3][C], styles [B][C], bias [3] or NULL -> y [B][P][3].  C a multiple of 4 up to 512, a power of two in quads.
static int torgb_fwd(const float* x, const float* w, const float* styles, const float* bias, const float* addend, float* y,
                     int B, int64_t P, int C, void* stream) {
    LDETR_CHECK(x && w && styles && y, "torgb_fwd: null pointer");
    const int C4 = C / 4;
    LDETR_CHECK(C % 4 == 0 && C4 >= 1 && C <= 512 && (C4 & (C4 - 1)) == 0, "torgb_fwd: C must be 4 x a power of two, at most 512 (got %d)", C);
    LDETR_CHECK((((uintptr_t)x | (uintptr_t)w | (uintptr_t)styles) & 15) == 0, "torgb_fwd: buffers must be 16-byte aligned");
    if (B == 0 || P == 0) return LDETR_OK;
    RgbFwdParams p; p.x = x; p.w = w; p.s = styles; p.bias = bias; p.y = y; p.P = P; p.B = B; p.C = C; p.add = addend;
    const int lpp = C4 < 64 ? C4 : 64;
    const long ppb = 256 / lpp;
    long gx = (P + ppb - 1) / ppb; if (gx > 4096) gx = 4096;
    const dim3 grid((unsigned)gx, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    switch (lpp) {
        case 1: hipLaunchKernelGGL(torgb_fwd_kernel<1>, grid, 256, 0, st, p); break;
        case 2: hipLaunchKernelGGL(torgb_fwd_kernel<2>, grid, 256, 0, st, p); break;
        case 4: hipLaunchKernelGGL(torgb_fwd_kernel<4>, grid, 256, 0, st, p); break;
        case 8: hipLaunchKernelGGL(torgb_fwd_kernel<8>, grid, 256, 0, st, p); break;
        case 16: hipLaunchKernelGGL(torgb_fwd_kernel<16>, grid, 256, 0, st, p); break;
        case 32: hipLaunchKernelGGL(torgb_fwd_kernel<32>, grid, 256, 0, st, p); break;
        default: hipLaunchKernelGGL(torgb_fwd_kernel<64>, grid, 256, 0, st, p); break;
    }
    return check_launch("torgb_fwd");
}

extern "C" int ldetr_torgb_fwd_f32(const float* x, const float* w, const float* styles, const float* bias, float* y,
                                   int B, int64_t P, int C, void* stream) {
    return torgb_fwd(x, w, styles, bias, nullptr, y, B, P, C, stream);
}

// The same with the skip connection folded in: y = addend + (conv + bias), addend [B][P][3] (the upsampled image of the block below; may be y itself).
extern "C" int ldetr_torgb_fwd_add_f32(const float* x, const float* w, const float* styles, const float* bias, const float* addend, float* y,
                                       int B, int64_t P, int C, void* stream) {
    LDETR_CHECK(addend, "torgb_fwd_add: null addend");
    return torgb_fwd(x, w, styles, bias, addend, y, B, P, C, stream);
}

// dws [B][3][C] and dbias [3] must be zeroed by the caller.
extern "C" int ldetr_torgb_bwd_f32(const float* x, const float* dy, const float* w, const float* styles,
                                   float* dx, float* dws, float* dbias, int B, int64_t P, int C, void* stream) {
    LDETR_CHECK(x && dy && w && styles && dx && dws, "torgb_bwd: null pointer");
    LDETR_CHECK(C % 4 == 0, "torgb_bwd: C must be a multiple of 4");
    RgbParams p; memset(&p, 0, sizeof(p));
    p.x = x; p.dy = dy; p.w = w; p.s = styles; p.dx = dx; p.dws = dws; p.dbias = dbias; p.B = B; p.P = P; p.C = C;
    const int C4 = C / 4; const int TQ = C4 < 256 ? C4 : 256; const int RL = 256 / TQ;
    long rows_pb = (long)RL * 16;
    long nb = ((P + rows_pb - 1) / rows_pb) * B * cdiv(C4, TQ);
    while (nb > 2048) { rows_pb *= 2; nb = ((P + rows_pb - 1) / rows_pb) * B * cdiv(C4, TQ); }
    p.rows_pb = (int)rows_pb;
    dim3 grid((unsigned)((P + rows_pb - 1) / rows_pb), B, cdiv(C4, TQ));
    hipLaunchKernelGGL(torgb_bwd_kernel, grid, 256, 0, (hipStream_t)stream, p);
    return check_launch("torgb_bwd");
}

// dxs (with s_conv, ds_conv) and dy_rgb (with s_rgb, w_rgb, dws_rgb, dbias_rgb) are optional, at least one of them; ddemod (with demod; bias
// NULL = 0) is optional.  dv may alias dxs.  Every accumulation target must hold its starting value (zeros or a gradient to add to).
extern "C" int ldetr_sg2_handoff_f32(const float* dxs, const float* x, const float* dy_rgb, float* dv, const float* s_conv, const float* s_rgb,
                                     const float* w_rgb, const float* bias, const float* demod, float* ds_conv, float* dws_rgb,
                                     float* dbias_rgb, float* dbias, float* ddemod, int B, int64_t P, int C, float alpha, float gain,
                                     void* stream) {
    LDETR_CHECK(x && dv && dbias, "sg2_handoff: x, dv and dbias are required");
    LDETR_CHECK(dxs || dy_rgb, "sg2_handoff: neither a conv gradient nor an rgb gradient");
    LDETR_CHECK(!dxs || (s_conv && ds_conv), "sg2_handoff: dxs needs s_conv and ds_conv");
    LDETR_CHECK(!dy_rgb || (s_rgb && w_rgb && dws_rgb && dbias_rgb), "sg2_handoff: dy_rgb needs s_rgb, w_rgb, dws_rgb and dbias_rgb");
    LDETR_CHECK(!ddemod || demod, "sg2_handoff: ddemod needs demod");
    LDETR_CHECK(C % 4 == 0 && C > 0 && B > 0 && P >= 0, "sg2_handoff: C must be a positive multiple of 4, B > 0 (got B %d, C %d)", B, C);
    LDETR_CHECK((((uintptr_t)dxs | (uintptr_t)x | (uintptr_t)dv | (uintptr_t)s_conv | (uintptr_t)s_rgb | (uintptr_t)w_rgb | (uintptr_t)bias |
                  (uintptr_t)demod) & 15) == 0, "sg2_handoff: buffers must be 16-byte aligned");
    if (P == 0) return LDETR_OK;
    HandoffParams p; memset(&p, 0, sizeof(p));
    p.dxs = dxs; p.x = x; p.dy = dy_rgb; p.dv = dv; p.s_conv = s_conv; p.s_rgb = s_rgb; p.w_rgb = w_rgb; p.bias = bias; p.demod = demod;
    p.ds_conv = ds_conv; p.dws = dws_rgb; p.dbias_rgb = dbias_rgb; p.dbias = dbias; p.ddemod = ddemod;
    p.B = B; p.P = P; p.C = C; p.gp = gain; p.gn = gain * alpha;
    hipStream_t st = (hipStream_t)stream;
    if (dxs && dy_rgb) return launch_handoff<true, true>(p, st);
    if (dxs) return launch_handoff<true, false>(p, st);
    return launch_handoff<false, true>(p, st);
}

extern "C" int ldetr_torgb_bwd_finish_f32(const float* dws, const float* s, const float* w, int B, int C, float* dw, float* ds, void* stream) {
    LDETR_CHECK(dws && s && w && dw && ds && B > 0 && C > 0, "torgb_bwd_finish: bad arguments");
    const int n = (B > 3 ? B : 3) * C;
    hipLaunchKernelGGL(torgb_finish_kernel, dim3((unsigned)((n + 255) / 256)), 256, 0, (hipStream_t)stream, dws, s, w, dw, ds, B, C);
    return check_launch("torgb_bwd_finish");
}
