// LayoutNet.forward in eval mode as ONE launch (include/ldetr_hip.h: ldetr_layoutnet_forward_f32; reference training/networks_layoutnet.py:68-86):
// the encoder of csrc/layoutnet.hip (same input stage, same layer body: layoutnet_layers.hpp), its row 0 as the features, fc_out_disc, then the
// decoder on the same 16-row tile -- x_n = relu(dec_fc_in([features, pos_token[n]])) as two reduction segments (the features broadcast over the
// rows, the position tokens shared by the samples of a block), four more post-norm layers with the elements' padding mask as key mask and no
// class token (row n = element n), fc_out_cls and sigmoid(fc_out_bbox) as one 16-column tile each.  Activations never leave LDS between the
// eight layers; every weight tile is loaded once per block and multiplied into all NS samples (v_mfma_f32_16x16x4_f32, fp32 operands).
// Outputs are dense ([B][N][..]); padded rows are written as 0 and the caller gathers the valid ones.  A valid element whose label is outside
// the embedding table makes every output of that sample NaN; nothing is read out of bounds.  Per-sample arithmetic does not depend on NS or on
// the other samples of the batch: the same sample gives the same bits alone, in a batch, and from either launch shape.
#include "layoutnet_layers.hpp"
#include "../../include/ldetr_hip.h"

using namespace ldetr;
using namespace ldetr::layoutnet;

namespace {

template <int NS>
__global__ __launch_bounds__(LN_THREADS) void layoutnet_forward_kernel(LayoutNetParams p) {
    __shared__ __attribute__((aligned(16))) float xb[NS * 16 * XP];      // the residual stream
    __shared__ __attribute__((aligned(16))) float ob[NS * 16 * XP];      // attention output (first: the label embeddings; between the stacks: the features, broadcast)
    __shared__ __attribute__((aligned(16))) float st[STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const float* wh = p.w + (long)p.num_label * LN_D;
    const float* wd = p.wd;
    const int N = p.N;
    unsigned valid[NS];
    bool bad[NS];
    encoder_input<NS>(p, xb, ob, valid, bad);
    for (int layer = 0; layer < LN_LAYERS; layer++) transformer_layer<NS>(wh + W_LAYERS + layer * L_SIZE, xb, ob, st, valid);

    // ---- features = row 0; logit_disc = fc_out_disc(features); the decoder's two input segments: features on every row (ob), pos_token[n] (st)
    if (p.out)
        for (int e = tid; e < NS * LN_D; e += LN_THREADS) {
            const int s = e / LN_D, c = e & (LN_D - 1), b = blockIdx.x * NS + s;
            if (b < p.B) p.out[(long)b * LN_D + c] = bad[s] ? __builtin_nanf("") : xb[s * 16 * XP + c];
        }
#pragma unroll
    for (int s = 0; s < NS; s++)
        if (wave == s) {                                                           // wave s: the 256-term dot product of sample s
            const int b = blockIdx.x * NS + s;
            const float4 f = *reinterpret_cast<const float4*>(xb + s * 16 * XP + 4 * lane);
            const float4 w4 = *reinterpret_cast<const float4*>(wd + D_DISCW + 4 * lane);
            const float d = wave_sum((f.x * w4.x + f.y * w4.y) + (f.z * w4.z + f.w * w4.w)) + wd[D_DISCB];
            if (lane == 0 && b < p.B) p.disc[b] = bad[s] ? __builtin_nanf("") : d;
        }
    for (int e = tid; e < NS * 16 * LN_D; e += LN_THREADS) {
        const int s = e / (16 * LN_D), row = (e / LN_D) & 15, c = e & (LN_D - 1);
        ob[s * 16 * XP + row * XP + c] = xb[s * 16 * XP + c];
    }
    for (int e = tid; e < 16 * LN_D; e += LN_THREADS) {
        const int row = e / LN_D, c = e & (LN_D - 1);
        st[row * XP + c] = row < N ? wd[D_POS + (long)row * LN_D + c] : 0.f;      // N <= 15 < max_bbox
    }
    // the decoder's keys: row n = element n; a sample without a valid element (or past the batch) keeps row 0 as a key so that its softmax is
    // defined -- none of its rows is written out
    unsigned dvalid[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) dvalid[s] = (valid[s] >> 1) ? (valid[s] >> 1) : 1u;
    __syncthreads();

    // ---- x = relu(dec_fc_in([features, pos_token[n]])); padded rows 0 (never keys)
    {
        f32x4 acc[NS][2];
        zero_acc<NS, 2>(acc);
        auto wrow = [&](int t) { return 32 * wave + 16 * t; };
        gemm16<NS, 2, 8>(acc, wd + D_FCW, 2 * LN_D, 0, LN_D, wrow, ob, XP, 16 * XP, lane);
        gemm16<NS, 2, 8>(acc, wd + D_FCW, 2 * LN_D, LN_D, LN_D, wrow, st, XP, 0, lane);
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int col = 32 * wave + 16 * t + r;
                const float bias = wd[D_FCB + col];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int row = 4 * g + q;
                    xb[s * 16 * XP + row * XP + col] = (((valid[s] >> 1) >> row) & 1u) ? fmaxf(acc[s][t][q] + bias, 0.f) : 0.f;
                }
            }
        __syncthreads();
    }
    for (int layer = 0; layer < LN_LAYERS; layer++) transformer_layer<NS>(wd + D_LAYERS + layer * L_SIZE, xb, ob, st, dvalid);

    // ---- the heads, one zero-padded 16-column tile each: wave 0 fc_out_cls, wave 1 sigmoid(fc_out_bbox); lane holds rows (= elements) 4 g + q, column r
    if (wave < 2) {
        f32x4 acc[NS][1];
        zero_acc<NS, 1>(acc);
        auto wrow = [&](int) { return 0; };
        gemm16<NS, 1, 8>(acc, wd + (wave == 0 ? D_CLSW : D_BOXW), LN_D, 0, LN_D, wrow, xb, XP, 16 * XP, lane);
        const float bias = wd[(wave == 0 ? D_CLSB : D_BOXB) + r];
        const int cols = wave == 0 ? p.num_label : 4;
        float* dst = wave == 0 ? p.cls : p.box;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int b = blockIdx.x * NS + s;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int row = 4 * g + q;
                if (b < p.B && row < N && r < cols) {
                    float v = acc[s][0][q] + bias;
                    if (wave == 1) v = 1.0f / (1.0f + expf(-v));
                    if (!(((valid[s] >> 1) >> row) & 1u)) v = 0.f;
                    else if (bad[s]) v = __builtin_nanf("");
                    dst[((long)b * N + row) * cols + r] = v;
                }
            }
        }
    }
}

}  // namespace

extern "C" int ldetr_layoutnet_forward_f32(const float* bbox, const int64_t* label, const uint8_t* padding_mask, const float* enc_weights,
                                           int64_t enc_len, const float* dec_weights, int64_t dec_len, int num_label, int B, int N,
                                           float* logit_disc, float* logit_cls, float* bbox_pred, float* features, void* stream) {
    LDETR_CHECK(bbox && label && padding_mask && enc_weights && dec_weights && logit_disc && logit_cls && bbox_pred,
                "layoutnet_forward: pointers must be non-null (only `features` may be)");
    LDETR_CHECK(B >= 0 && N >= 1, "layoutnet_forward: bad shape B=%d N=%d", B, N);
    LDETR_CHECK(N + 1 <= 16, "layoutnet_forward: a sample is the class token plus at most 15 elements (got N=%d); longer layouts take the composed path", N);
    LDETR_CHECK(num_label >= 1 && num_label <= 16, "layoutnet_forward: the class head is one 16-column tile (got %d labels); larger tables take the composed path",
                num_label);
    LDETR_CHECK(enc_len == (int64_t)num_label * LN_D + W_TOTAL, "layoutnet_forward: %lld packed encoder weights do not match LayoutNet(%d) (%lld)",
                (long long)enc_len, num_label, (long long)((int64_t)num_label * LN_D + W_TOTAL));
    LDETR_CHECK(dec_len == (int64_t)D_TOTAL, "layoutnet_forward: %lld packed decoder weights, expected %lld", (long long)dec_len, (long long)D_TOTAL);
    if (B == 0) return LDETR_OK;
    LayoutNetParams p; memset(&p, 0, sizeof(p));
    p.bbox = bbox; p.label = label; p.pad = padding_mask; p.w = enc_weights; p.out = features; p.B = B; p.N = N; p.num_label = num_label; p.map_len = 0;
    p.wd = dec_weights; p.disc = logit_disc; p.cls = logit_cls; p.box = bbox_pred;
    // the launch shapes of ldetr_layoutnet_features_f32: one sample per block while the grid is small, three per weight tile above
    if (B <= 256) hipLaunchKernelGGL(layoutnet_forward_kernel<1>, dim3((unsigned)B), LN_THREADS, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(layoutnet_forward_kernel<3>, dim3((unsigned)cdiv(B, 3)), LN_THREADS, 0, (hipStream_t)stream, p);
    return check_launch("layoutnet_forward");
}
