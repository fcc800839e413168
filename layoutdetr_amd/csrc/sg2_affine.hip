// Backward of the style affines of the StyleGAN2 synthesis network, all layers at once (training/networks_stylegan2.py: SynthesisLayer.affine,
// ToRGBLayer.affine; one latent w [B][D] feeds every layer).
//   s_l = post_l * (gain_l * w A_l^T + bias_l),   A_l [C_l][D],   scale_l = post_l * gain_l,   ds_l [B][C_l] given
//   dw[b][k]    = sum_l scale_l * sum_c ds_l[b][c] * A_l[c][k]
//   dA_l[c][k] += scale_l * sum_b ds_l[b][c] * w[b][k]
//   db_l[c]    += post_l * sum_b ds_l[b][c]
// As autograd nodes that is, per layer, one paired small-GEMM launch (data + weight gradient; 8 blocks for 1 MB of A_l) and one add of the
// layer's dw into the running sum: 40 launches for 98 MFLOP and 36 MB of traffic at the 256^2 network.  Here: ONE grid over (64-channel chunk of
// the concatenated channels, 64 latent columns).  A block stages its [64][64] tile of A_l, its chunk of ds_l and its columns of w in LDS and
// produces the chunk's partial dw (into scratch), the dA tile (+=) and, on the first column group, the db chunk (+=).  A second launch adds the
// partial dw in chunk order: one writer per element and a fixed order, so the result is deterministic.  Plain fp32 FMAs: the problem is
// bound by reading A once (12 MB) and updating dA once, not by arithmetic.
#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"

namespace ldetr {

constexpr int AFF_MAXB = 64;

struct AffineGroup { ldetr_affine_desc d[LDETR_AFFINE_GROUP_MAX]; int start[LDETR_AFFINE_GROUP_MAX + 1]; int n; };

// grid (chunks * ceil(D / 64)); dynamic LDS (64 + 2 B) * 64 floats
__global__ __launch_bounds__(256) void sg2_affine_bwd_kernel(AffineGroup g, const float* __restrict__ latent, float* __restrict__ part, int B, int D) {
    extern __shared__ float lds[];
    float* At = lds;                   // [64 c][64 col]
    float* dsL = lds + 64 * 64;        // [B][64 c]
    float* wL = dsL + B * 64;          // [B][64 col]
    const int gx = (D + 63) >> 6;
    const int ci = (int)blockIdx.x / gx, cgp = (int)blockIdx.x - ci * gx;
    int pi = 0;
    for (int i = 1; i < g.n; i++) pi += (ci >= g.start[i]) ? 1 : 0;
    const ldetr_affine_desc& d = g.d[pi];
    const int C = d.C, c0 = (ci - g.start[pi]) * 64, col0 = cgp * 64;
    const int tid = threadIdx.x, cc = tid & 63, grp = tid >> 6;
    const int col = col0 + cc;
    for (int idx = tid; idx < 64 * 64; idx += 256) {
        const int c = idx >> 6;
        At[idx] = (c0 + c < C && col < D) ? d.A[(long)(c0 + c) * D + col] : 0.f;      // (idx & 63 == cc: 256 is a multiple of 64)
    }
    for (int idx = tid; idx < B * 64; idx += 256) {
        const int b = idx >> 6;
        dsL[idx] = (c0 + cc < C) ? d.ds[(long)b * C + c0 + cc] : 0.f;
        wL[idx] = (col < D) ? latent[(long)b * D + col] : 0.f;
    }
    __syncthreads();
    // partial dw of this chunk: sample b = grp + 4 u, column col
    {
        float acc[16];
#pragma unroll
        for (int u = 0; u < 16; u++) acc[u] = 0.f;
        for (int c = 0; c < 64; c++) {
            const float av = At[c * 64 + cc];
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (grp + 4 * u < B) acc[u] += dsL[(grp + 4 * u) * 64 + c] * av;
        }
        if (col < D) {
#pragma unroll
            for (int u = 0; u < 16; u++)
                if (grp + 4 * u < B) part[((long)ci * B + grp + 4 * u) * D + col] = d.scale * acc[u];
        }
    }
    // dA tile: channels c0 + 16 grp .. + 15, column col
    if (d.dA && col < D) {
        for (int j = 0; j < 16; j++) {
            const int c = grp * 16 + j;
            if (c0 + c >= C) break;
            float v = 0.f;
            for (int b = 0; b < B; b++) v += dsL[b * 64 + c] * wL[b * 64 + cc];
            float* dst = d.dA + (long)(c0 + c) * D + col;
            *dst += d.scale * v;
        }
    }
    if (d.db && cgp == 0 && tid < 64 && c0 + tid < C) {
        float v = 0.f;
        for (int b = 0; b < B; b++) v += dsL[b * 64 + tid];
        d.db[c0 + tid] += d.post * v;
    }
}

// dw[b][k] (+)= sum over the chunks, in order
__global__ __launch_bounds__(256) void sg2_affine_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int accumulate, int chunks, long BD) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BD) return;
    float v = 0.f;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; u++) t[u] = part[(long)(c + u) * BD + i];
#pragma unroll
        for (int u = 0; u < 8; u++) v += t[u];
    }
    for (; c < chunks; c++) v += part[(long)c * BD + i];
    dw[i] = accumulate ? dw[i] + v : v;
}

static int affine_fill(AffineGroup& g, const ldetr_affine_desc* d, int n, const char* what) {
    LDETR_CHECK(d && n >= 1 && n <= LDETR_AFFINE_GROUP_MAX, "%s: 1..%d layers", what, LDETR_AFFINE_GROUP_MAX);
    memset(&g, 0, sizeof(g));
    g.n = n;
    long chunks = 0;
    for (int l = 0; l < n; l++) {
        LDETR_CHECK(d[l].ds && d[l].A && d[l].C > 0, "%s: bad layer %d", what, l);
        g.d[l] = d[l];
        g.start[l] = (int)chunks;
        chunks += cdiv(d[l].C, 64);
    }
    LDETR_CHECK(chunks < (1 << 20), "%s: too many channels", what);
    g.start[n] = (int)chunks;
    return LDETR_OK;
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_sg2_affine_bwd_f32(const ldetr_affine_desc* layers, int n, const float* latent, float* dlatent, int accumulate_dlatent,
                                        float* scratch, int64_t scratch_floats, int B, int D, void* stream) {
    AffineGroup g;
    int rc = affine_fill(g, layers, n, "sg2_affine_bwd"); if (rc) return rc;
    LDETR_CHECK(latent && dlatent && scratch, "sg2_affine_bwd: null pointer");
    LDETR_CHECK(B > 0 && B <= AFF_MAXB && D > 0, "sg2_affine_bwd: bad shape (batch <= %d)", AFF_MAXB);
    const int chunks = g.start[n], gx = cdiv(D, 64);
    LDETR_CHECK((long)chunks * gx < 0x7fffffffL, "sg2_affine_bwd: grid too large");
    LDETR_CHECK(scratch_floats >= (int64_t)chunks * B * D, "sg2_affine_bwd: scratch too small (%lld floats needed)", (long long)chunks * B * D);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(64 + 2 * B) * 64 * sizeof(float);
    hipLaunchKernelGGL(sg2_affine_bwd_kernel, dim3((unsigned)(chunks * gx)), 256, lds, st, g, latent, scratch, B, D);
    rc = check_launch("sg2_affine_bwd"); if (rc) return rc;
    const long BD = (long)B * D;
    hipLaunchKernelGGL(sg2_affine_bwd_reduce_kernel, dim3((unsigned)((BD + 255) / 256)), 256, 0, st, scratch, dlatent, accumulate_dlatent, chunks, BD);
    return check_launch("sg2_affine_bwd_reduce");
}
