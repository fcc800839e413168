// Layout FID on the device (include/ldetr_hip.h: ldetr_layoutnet_features_f32, ldetr_feature_stats_f64).
//
// (a) LayoutNet.extract_features (reference training/networks_layoutnet.py:48-66) as ONE launch.  A sample is the class token plus at most
//     15 elements = one 16-row MFMA tile; d_model 256, 4 heads of width 64, feed-forward width 128, four post-norm layers.  A block of 8 waves
//     owns NS samples and walks the whole network with the activations in LDS; every weight tile it loads (global -> registers in MFMA operand
//     order, 16 weight rows x 16 reduction columns as one float4 per lane) is multiplied into all NS samples before the next one is fetched.
//     The contraction is v_mfma_f32_16x16x4_f32 on fp32 operands: the project's fp32 value contract, no downcast.  The reduction index of a
//     float4 is spread as k = 4 (lane >> 4) + j over the four MFMAs j = 0..3 of a chunk -- A and B use the same permutation, so the sum is the
//     plain dot product in a fixed order.
//       wave w: head w >> 1; the two waves of a head split its 12 q|k|v column tiles, both compute the 16 x 16 score tile (64 MFMA-k), the softmax
//       over the valid keys, and half of P V each; out_proj / linear2: 2 column tiles per wave, linear1: 1; LayerNorm: 2 rows per wave and sample.
//     Padded rows are zero on entry and are never keys (their score columns are -inf before the softmax), so nothing they hold reaches row 0.
//     A valid element whose label is outside the embedding table makes that sample's features NaN (nothing is read out of bounds).
//     The input stage and the layer body live in layoutnet_layers.hpp: csrc/layoutnet_train.hip (LayoutNet.forward) walks the same code.
// (b) FeatureStats.append with capture_mean_cov (reference metrics/metric_utils_layout.py:97-112): raw_mean += sum_i x_i, raw_cov += sum_i x_i x_i^T
//     with every product and sum in float64, v_mfma_f64_16x16x4_f64.  One wave owns one 16 x 16 tile of raw_cov (and, in the first tile column,
//     16 entries of raw_mean): no atomics, one fixed summation order, the same input gives the same bits.
#include "layoutnet_layers.hpp"
#include "../../include/ldetr_hip.h"

using namespace ldetr;
using namespace ldetr::layoutnet;       // the layer body, shared with csrc/layoutnet_train.hip

namespace {

template <int NS>
__global__ __launch_bounds__(LN_THREADS) void layoutnet_features_kernel(LayoutNetParams p) {
    __shared__ __attribute__((aligned(16))) float xb[NS * 16 * XP];      // the residual stream
    __shared__ __attribute__((aligned(16))) float ob[NS * 16 * XP];      // attention output (first: the label embeddings)
    __shared__ __attribute__((aligned(16))) float st[STAGE];
    const int tid = threadIdx.x;
    const float* wh = p.w + (long)p.num_label * LN_D;
    unsigned valid[NS];
    bool bad[NS];
    encoder_input<NS>(p, xb, ob, valid, bad);
    for (int layer = 0; layer < LN_LAYERS; layer++) transformer_layer<NS>(wh + W_LAYERS + layer * L_SIZE, xb, ob, st, valid);
    for (int e = tid; e < NS * LN_D; e += LN_THREADS) {
        const int s = e / LN_D, c = e & (LN_D - 1), b = blockIdx.x * NS + s;
        if (b < p.B) p.out[(long)b * LN_D + c] = bad[s] ? __builtin_nanf("") : xb[s * 16 * XP + c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

// block = one wave = the tile (ti, tj) of raw_cov; v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D[row = (lane >> 4) + 4 reg][col = lane & 15] (NOT the f32 shapes' row map).
__global__ __launch_bounds__(64) void feature_stats_f64_kernel(const float* __restrict__ x, long n, int F, double* __restrict__ raw_mean, double* __restrict__ raw_cov) {
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int ti = blockIdx.y, tj = blockIdx.x;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;
    const float* pa = x + 16 * ti + r;
    const float* pb = x + 16 * tj + r;
    const long n4 = n & ~3L;
#pragma unroll 4
    for (long k0 = 0; k0 < n4; k0 += 4) {
        const double a = (double)pa[(k0 + g) * F], b = (double)pb[(k0 + g) * F];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        colsum += a;
    }
    if (n4 < n) {
        const bool in = n4 + g < n;
        const double a = in ? (double)pa[(n4 + g) * F] : 0.0, b = in ? (double)pb[(n4 + g) * F] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        colsum += a;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) raw_cov[(long)(16 * ti + g + 4 * q) * F + 16 * tj + r] += acc[q];
    if (tj == 0) {
        colsum += __shfl_xor(colsum, 16, 64);
        colsum += __shfl_xor(colsum, 32, 64);
        if (g == 0) raw_mean[16 * ti + r] += colsum;
    }
}

}  // namespace

extern "C" int ldetr_layoutnet_features_f32(const float* bbox, const int64_t* label, const uint8_t* padding_mask, const int* label_map, int map_len,
                                            const float* weights, int64_t weights_len, int num_label, int B, int N, float* out, void* stream) {
    LDETR_CHECK(bbox && label && padding_mask && weights && out, "layoutnet_features: pointers must be non-null");
    LDETR_CHECK(B >= 0 && N >= 1, "layoutnet_features: bad shape B=%d N=%d", B, N);
    LDETR_CHECK(N + 1 <= 16, "layoutnet_features: a sample is the class token plus at most 15 elements (got N=%d); longer layouts take the composed path", N);
    LDETR_CHECK(num_label >= 1 && weights_len == (int64_t)num_label * LN_D + W_TOTAL,
                "layoutnet_features: %lld packed weights do not match LayoutNet(%d) (%lld)", (long long)weights_len, num_label,
                (long long)((int64_t)num_label * LN_D + W_TOTAL));
    LDETR_CHECK(map_len >= 0 && map_len <= 16 && (map_len == 0 || label_map), "layoutnet_features: the label map has at most 16 entries (got %d)", map_len);
    LayoutNetParams p; memset(&p, 0, sizeof(p));
    for (int i = 0; i < map_len; i++) {
        LDETR_CHECK(label_map[i] >= 0 && label_map[i] < num_label, "layoutnet_features: label map entry %d -> %d is outside the embedding table (%d labels)", i,
                    label_map[i], num_label);
        p.map[i] = label_map[i];
    }
    if (B == 0) return LDETR_OK;
    p.bbox = bbox; p.label = label; p.pad = padding_mask; p.w = weights; p.out = out; p.B = B; p.N = N; p.num_label = num_label; p.map_len = map_len;
    // few samples: one per block (every block streams all weights either way, and the grid is far below the CU count); many: each weight tile serves three
    if (B <= 256) hipLaunchKernelGGL(layoutnet_features_kernel<1>, dim3((unsigned)B), LN_THREADS, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(layoutnet_features_kernel<3>, dim3((unsigned)cdiv(B, 3)), LN_THREADS, 0, (hipStream_t)stream, p);
    return check_launch("layoutnet_features");
}

extern "C" int ldetr_feature_stats_f64(const float* x, int64_t n, int F, double* raw_mean, double* raw_cov, void* stream) {
    LDETR_CHECK(x && raw_mean && raw_cov, "feature_stats: pointers must be non-null");
    LDETR_CHECK(n >= 0 && F >= 16 && F <= 256 && F % 16 == 0, "feature_stats: needs n >= 0 and F a multiple of 16 up to 256 (got n=%lld F=%d)", (long long)n, F);
    if (n == 0) return LDETR_OK;
    hipLaunchKernelGGL(feature_stats_f64_kernel, dim3((unsigned)(F / 16), (unsigned)(F / 16)), 64, 0, (hipStream_t)stream, x, (long)n, F, raw_mean, raw_cov);
    return check_launch("feature_stats");
}
