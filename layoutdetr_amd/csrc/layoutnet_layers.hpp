// The pieces of LayoutNet that its two fused kernels share (csrc/layoutnet.hip: extract_features; csrc/layoutnet_train.hip: forward): the packed
// weight layout, the 16-row MFMA GEMM over LDS activations, LayerNorm, the encoder's input stage and one post-norm transformer layer.  Everything
// is inlined into the kernel that uses it; csrc/layoutnet.hip describes the design (a sample = one 16-row tile, 8 waves, activations in LDS).
#pragma once
#include "ldetr_common.hpp"

namespace ldetr {
namespace layoutnet {

constexpr int LN_D = 256, LN_F = 128, LN_DH = 64, LN_LAYERS = 4, LN_WAVES = 8, LN_THREADS = 64 * LN_WAVES;
constexpr int XP = 260, QP = 196, HP = 132;             // LDS pitches (floats; multiples of 4: float4 rows): x / o, a head's q|k|v, the hidden layer
constexpr int STAGE = 4 * 16 * QP;                      // the four heads' q|k|v of ONE sample (samples take turns); the hidden layer of all samples aliases it

// packed encoder weights (floats), after the embedding table [num_label][256]
constexpr long W_BBW = 0, W_BBB = W_BBW + LN_D * 4, W_FCW = W_BBB + LN_D, W_FCB = W_FCW + LN_D * 2 * LN_D, W_TOK = W_FCB + LN_D, W_LAYERS = W_TOK + LN_D;
constexpr long L_INW = 0, L_INB = L_INW + 3 * LN_D * LN_D, L_OUTW = L_INB + 3 * LN_D, L_OUTB = L_OUTW + LN_D * LN_D, L_N1W = L_OUTB + LN_D, L_N1B = L_N1W + LN_D,
               L_L1W = L_N1B + LN_D, L_L1B = L_L1W + LN_F * LN_D, L_L2W = L_L1B + LN_F, L_L2B = L_L2W + LN_D * LN_F, L_N2W = L_L2B + LN_D, L_N2B = L_N2W + LN_D,
               L_SIZE = L_N2B + LN_D;
constexpr long W_TOTAL = W_LAYERS + LN_LAYERS * L_SIZE;

// packed decoder + heads (floats; include/ldetr_hip.h lists the order): every tensor starts 16-byte aligned, the heads are zero-padded to 16 rows
constexpr int LN_MAX_BBOX = 50;
constexpr long D_POS = 0, D_FCW = D_POS + (long)LN_MAX_BBOX * LN_D, D_FCB = D_FCW + LN_D * 2 * LN_D, D_LAYERS = D_FCB + LN_D,
               D_CLSW = D_LAYERS + LN_LAYERS * L_SIZE, D_CLSB = D_CLSW + 16 * LN_D, D_BOXW = D_CLSB + 16, D_BOXB = D_BOXW + 16 * LN_D,
               D_DISCW = D_BOXB + 16, D_DISCB = D_DISCW + LN_D, D_TOTAL = D_DISCB + 4;

#define LN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

struct LayoutNetParams {
    const float* bbox; const int64_t* label; const uint8_t* pad; const float* w; float* out;
    int B, N, num_label, map_len;
    int map[16];
    // forward only (csrc/layoutnet_train.hip); `out` is then the optional features output
    const float* wd; float* disc; float* cls; float* box;
};

// acc[s][t] += X_s [16 x K] . W[wrow(t) + 0..15][kw0 .. kw0 + K)^T for the samples s of the block; X_s in LDS at xs + s * sstride (row pitch `pitch`).
// U reduction chunks of 16 are fetched together (NT * U float4 loads per lane in flight before the first MFMA: a block streams all weights through one
// CU, so the loads in flight are what its time is made of); K is a multiple of 16 U.
template <int NS, int NT, int U, class RowFn>
__device__ __forceinline__ void gemm16(f32x4 (&acc)[NS][NT], const float* __restrict__ W, int ldw, int kw0, int K, RowFn wrow,
                                       const float* xs, int pitch, int sstride, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const float* wp[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) wp[t] = W + (long)(wrow(t) + r) * ldw + kw0 + 4 * g;
    const float* xp = xs + r * pitch + 4 * g;
    for (int k0 = 0; k0 < K; k0 += 16 * U) {
        float4 b[U][NT];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int t = 0; t < NT; t++) b[u][t] = *reinterpret_cast<const float4*>(wp[t] + k0 + 16 * u);
#pragma unroll
        for (int u = 0; u < U; u++) {
            float4 a[NS];
#pragma unroll
            for (int s = 0; s < NS; s++) a[s] = *reinterpret_cast<const float4*>(xp + s * sstride + k0 + 16 * u);
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    acc[s][t] = LN_MFMA(a[s].x, b[u][t].x, acc[s][t]);
                    acc[s][t] = LN_MFMA(a[s].y, b[u][t].y, acc[s][t]);
                    acc[s][t] = LN_MFMA(a[s].z, b[u][t].z, acc[s][t]);
                    acc[s][t] = LN_MFMA(a[s].w, b[u][t].w, acc[s][t]);
                }
        }
    }
}

template <int NS, int NT>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NS][NT]) {
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// x <- LayerNorm(x) over 256 columns, in place; wave w takes rows 2w, 2w + 1 of every sample (eps 1e-5, biased variance: nn.LayerNorm)
template <int NS>
__device__ __forceinline__ void layernorm_rows(float* xb, const float* __restrict__ gamma, const float* __restrict__ beta, int wave, int lane) {
    const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * lane), bt = *reinterpret_cast<const float4*>(beta + 4 * lane);
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            float* row = xb + s * 16 * XP + (2 * wave + i) * XP + 4 * lane;
            float4 v = *reinterpret_cast<float4*>(row);
            const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / LN_D);
            v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
            const float var = wave_sum((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w)) * (1.0f / LN_D);
            const float rs = 1.0f / sqrtf(var + 1e-5f);
            v.x = v.x * rs * gm.x + bt.x; v.y = v.y * rs * gm.y + bt.y; v.z = v.z * rs * gm.z + bt.z; v.w = v.w * rs * gm.w + bt.w;
            *reinterpret_cast<float4*>(row) = v;
        }
}

// The encoder's input (networks_layoutnet.py:49, 62-65): which rows are keys (valid[s]: bit 0 = the class token, bit n + 1 = element n), whether a
// valid element's label is outside the table (bad[s]), and xb <- [token; relu(enc_fc_in([fc_bbox(bbox), emb_label(label)]))] with padded rows 0.
// ob is scratch (the label embeddings).  Ends synchronised.
template <int NS>
__device__ __forceinline__ void encoder_input(const LayoutNetParams& p, float* xb, float* ob, unsigned (&valid)[NS], bool (&bad)[NS]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const float* emb = p.w;
    const float* wh = p.w + (long)p.num_label * LN_D;
    const int N = p.N;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int b = blockIdx.x * NS + s;
        valid[s] = 1u; bad[s] = false;
        if (b < p.B)
            for (int n = 0; n < N; n++)
                if (!p.pad[(long)b * N + n]) valid[s] |= 2u << n;
    }
    for (int e = tid; e < NS * 16 * LN_D; e += LN_THREADS) {
        const int s = e / (16 * LN_D), row = (e / LN_D) & 15, c = e & (LN_D - 1);
        const int b = blockIdx.x * NS + s;
        float vb = 0.f, vl = 0.f;
        if (row >= 1 && ((valid[s] >> row) & 1u)) {
            const float4 bx = *reinterpret_cast<const float4*>(p.bbox + ((long)b * N + row - 1) * 4);
            const float4 wv = *reinterpret_cast<const float4*>(wh + W_BBW + 4 * c);
            vb = wh[W_BBB + c] + bx.x * wv.x + bx.y * wv.y + bx.z * wv.z + bx.w * wv.w;
            int64_t lb = p.label[(long)b * N + row - 1];
            if (lb >= 0 && lb < p.map_len) lb = p.map[lb];
            if (lb >= 0 && lb < p.num_label) vl = emb[lb * LN_D + c];
        }
        xb[s * 16 * XP + row * XP + c] = vb;
        ob[s * 16 * XP + row * XP + c] = vl;
    }
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int b = blockIdx.x * NS + s;
        if (b < p.B)
            for (int n = 0; n < N; n++) {
                int64_t lb = p.label[(long)b * N + n];
                if (lb >= 0 && lb < p.map_len) lb = p.map[lb];
                if (((valid[s] >> (n + 1)) & 1u) && (lb < 0 || lb >= p.num_label)) bad[s] = true;
            }
    }
    __syncthreads();

    // ---- x = relu(enc_fc_in([b, l])): the concatenation is two reduction segments; the class token goes in front
    {
        f32x4 acc[NS][2];
        zero_acc<NS, 2>(acc);
        auto wrow = [&](int t) { return 32 * wave + 16 * t; };
        gemm16<NS, 2, 8>(acc, wh + W_FCW, 2 * LN_D, 0, LN_D, wrow, xb, XP, 16 * XP, lane);
        gemm16<NS, 2, 8>(acc, wh + W_FCW, 2 * LN_D, LN_D, LN_D, wrow, ob, XP, 16 * XP, lane);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int col = 32 * wave + 16 * t + r;
                const float bias = wh[W_FCB + col], tok = wh[W_TOK + col];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int row = 4 * g + q;
                    const float v = fmaxf(acc[s][t][q] + bias, 0.f);
                    xb[s * 16 * XP + row * XP + col] = row == 0 ? tok : (((valid[s] >> row) & 1u) ? v : 0.f);
                }
            }
        __syncthreads();
    }
}

// One post-norm layer (nn.TransformerEncoderLayer, relu, dropout off) on xb in place; wl = its packed weights (L_* offsets), valid[s] = the key rows
// of sample s.  ob receives the attention output, st is the staging area.  Starts and ends synchronised.
//   wave w: head w >> 1; the two waves of a head split its 12 q|k|v column tiles, both compute the 16 x 16 score tile (64 MFMA-k), the softmax
//   over the valid keys, and half of P V each; out_proj / linear2: 2 column tiles per wave, linear1: 1; LayerNorm: 2 rows per wave and sample.
template <int NS>
__device__ __forceinline__ void transformer_layer(const float* __restrict__ wl, float* xb, float* ob, float* st, const unsigned (&valid)[NS]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int head = wave >> 1, half = wave & 1;
    float* sh = st + head * 16 * QP;
    // ---- q | k | v of the head: 12 column tiles, 6 per wave of the pair (tile u: part u >> 2 of in_proj, columns 64 head + 16 (u & 3))
    {
        f32x4 acc[NS][6];
        zero_acc<NS, 6>(acc);
        auto wrow = [&](int t) { const int u = 6 * half + t; return (u >> 2) * LN_D + LN_DH * head + 16 * (u & 3); };
        gemm16<NS, 6, (NS == 1 ? 4 : 2)>(acc, wl + L_INW, LN_D, 0, LN_D, wrow, xb, XP, 16 * XP, lane);
#pragma unroll
        for (int s = 0; s < NS; s++) {
#pragma unroll
            for (int t = 0; t < 6; t++) {
                const int u = 6 * half + t;
                const float bias = wl[L_INB + wrow(t) + r], sc = u < 4 ? 0.125f : 1.0f;      // q is scaled by 1 / sqrt(64) after its bias
#pragma unroll
                for (int q = 0; q < 4; q++) sh[(4 * g + q) * QP + 16 * u + r] = (acc[s][t][q] + bias) * sc;
            }
            __syncthreads();
            // scores S[i][j] = q_i . k_j: lane holds rows 4 g + q, column (= key) r
            f32x4 sc4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k0 = 0; k0 < LN_DH; k0 += 16) {
                const float4 a = *reinterpret_cast<const float4*>(sh + r * QP + k0 + 4 * g);
                const float4 b = *reinterpret_cast<const float4*>(sh + r * QP + LN_DH + k0 + 4 * g);
                sc4 = LN_MFMA(a.x, b.x, sc4); sc4 = LN_MFMA(a.y, b.y, sc4); sc4 = LN_MFMA(a.z, b.z, sc4); sc4 = LN_MFMA(a.w, b.w, sc4);
            }
            const bool key = (valid[s] >> r) & 1u;
            float pr[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float v = key ? sc4[q] : -INFINITY, m = v;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
                const float e = key ? expf(v - m) : 0.f;
                float sum = e;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
                pr[q] = e / sum;
            }
            __syncthreads();                    // both waves of the pair have read q and k
            if (half == 0)
#pragma unroll
                for (int q = 0; q < 4; q++) sh[(4 * g + q) * QP + r] = pr[q];      // P over the head's q columns 0..15
            __syncthreads();
            // O = P V: two of the head's four column tiles per wave
            const float4 pa = *reinterpret_cast<const float4*>(sh + r * QP + 4 * g);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int c0 = 32 * half + 16 * t;
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                o = LN_MFMA(pa.x, sh[(4 * g + 0) * QP + 2 * LN_DH + c0 + r], o);
                o = LN_MFMA(pa.y, sh[(4 * g + 1) * QP + 2 * LN_DH + c0 + r], o);
                o = LN_MFMA(pa.z, sh[(4 * g + 2) * QP + 2 * LN_DH + c0 + r], o);
                o = LN_MFMA(pa.w, sh[(4 * g + 3) * QP + 2 * LN_DH + c0 + r], o);
#pragma unroll
                for (int q = 0; q < 4; q++) ob[s * 16 * XP + (4 * g + q) * XP + LN_DH * head + c0 + r] = o[q];
            }
            __syncthreads();                    // the next sample overwrites the staging area
        }
    }
    // ---- x = norm1(x + out_proj(o))
    {
        f32x4 acc[NS][2];
        zero_acc<NS, 2>(acc);
        auto wrow = [&](int t) { return 32 * wave + 16 * t; };
        gemm16<NS, 2, 8>(acc, wl + L_OUTW, LN_D, 0, LN_D, wrow, ob, XP, 16 * XP, lane);
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int col = wrow(t) + r;
                const float bias = wl[L_OUTB + col];
#pragma unroll
                for (int q = 0; q < 4; q++) xb[s * 16 * XP + (4 * g + q) * XP + col] += acc[s][t][q] + bias;
            }
        __syncthreads();
        layernorm_rows<NS>(xb, wl + L_N1W, wl + L_N1B, wave, lane);
        __syncthreads();
    }
    // ---- x = norm2(x + linear2(relu(linear1(x))))
    {
        f32x4 acc[NS][1];
        zero_acc<NS, 1>(acc);
        auto wrow = [&](int) { return 16 * wave; };
        gemm16<NS, 1, 8>(acc, wl + L_L1W, LN_D, 0, LN_D, wrow, xb, XP, 16 * XP, lane);
        const float bias = wl[L_L1B + 16 * wave + r];
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int q = 0; q < 4; q++) st[s * 16 * HP + (4 * g + q) * HP + 16 * wave + r] = fmaxf(acc[s][0][q] + bias, 0.f);
        __syncthreads();
    }
    {
        f32x4 acc[NS][2];
        zero_acc<NS, 2>(acc);
        auto wrow = [&](int t) { return 32 * wave + 16 * t; };
        gemm16<NS, 2, 8>(acc, wl + L_L2W, LN_F, 0, LN_F, wrow, st, HP, 16 * HP, lane);
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int col = wrow(t) + r;
                const float bias = wl[L_L2B + col];
#pragma unroll
                for (int q = 0; q < 4; q++) xb[s * 16 * XP + (4 * g + q) * XP + col] += acc[s][t][q] + bias;
            }
        __syncthreads();
        layernorm_rows<NS>(xb, wl + L_N2W, wl + L_N2B, wave, lane);
        __syncthreads();
    }
}

}  // namespace layoutnet
}  // namespace ldetr
