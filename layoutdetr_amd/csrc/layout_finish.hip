// Finishing, scoring and ranking of generated layouts, fused: what the reference's inference loop does per seed after G(...)
//     jitter(bbox, strength, seed)                                         generate.py:88-91, generate_util.py:145-148
//     horizontal_center_aligned / horizontal_left_aligned                  generate_util.py:100-115
//     de_overlap                                                           generate_util.py:117-141
//     compute_overlap / compute_alignment of the finished boxes            metrics/metric_layoutnet.py:153-201 (generate_util.py:442-443)
//     np.argsort of the per-seed overlaps                                  generate_util.py:450
// The reference runs the alignment and de_overlap as Python double loops over 0-d device tensors: every comparison (`if abs(yc2 - yc1) < ...`,
// `if yc1 < yc2`) is a host synchronisation and every update a launch of its own, a few hundred tiny launches per candidate, then two metric
// chains of ~40 launches, a device-to-host copy per value and a host sort.  The arithmetic is about 2 N^2 dependent steps on 4 N floats per
// candidate -- nothing; the cost removed here is launches and synchronisations.  ONE launch handles all C x K layouts: one block per condition,
// one thread per candidate (a thread takes candidates k, k + 128, ...), the candidate's boxes in a private LDS column (element-major, so the
// lanes of a wave hit consecutive banks), ranking after a block barrier over the overlaps kept in LDS.
// Sequential semantics: the reference unpacks `xc1, yc1, w1, h1 = bbox_fake[0, i]` as VIEWS, so every read inside the pair loops sees the
// updates made earlier in the same pass; `diff` and the `yc1 < yc2` branch are evaluated before that pair's updates.  Here every read goes to
// the current value in LDS.  Heights that de_overlap drives to <= 0 are kept, as the reference keeps them.
// Arithmetic: the reference's fp32 operations in the reference's order, one IEEE operation each (no fma contraction), as box_ops.hip.
// Ranking: order[c] is the STABLE ascending order of overlap[c], NaN last -- rank(k) = #{j : ov_j < ov_k or (ov_j == ov_k and j < k)}.
// Candidates without any overlap tie at exactly 0, so the tie rule is part of the contract.
#include "ldetr_common.hpp"
#include "../../include/ldetr_hip.h"

#pragma clang fp contract(off)

namespace ldetr {

constexpr int LF_THREADS = 128;     // candidates in flight per block: 16 slots x 4 floats x 128 columns = 32 KiB of LDS
constexpr int LF_MAX_N = 16;
constexpr int LF_MAX_K = 1024;

struct LayoutFinishParams {
    const float* in; const int* num; const float* factors; const unsigned char* jitter; const unsigned char* mode;
    float* out; float* overlap; float* alignment; int* order;
    int K, N;
};

// total order of the ranking: NaN after every number, NaNs (and equal numbers, -0 == +0) tie
__device__ __forceinline__ bool lf_less(float a, float b) { return a != a ? false : (b != b ? true : a < b); }
__device__ __forceinline__ bool lf_equal(float a, float b) { return (a != a && b != b) || a == b; }

__global__ __launch_bounds__(LF_THREADS) void layout_finish_kernel(LayoutFinishParams p) {
    __shared__ float sb[LF_MAX_N * 4][LF_THREADS];
    __shared__ float sov[LF_MAX_K];
    const int c = blockIdx.x, tid = threadIdx.x, N = p.N, K = p.K;
#define BX(i, f) sb[(i) * 4 + (f)][tid]
    for (int k = tid; k < K; k += LF_THREADS) {
        const long ck = (long)c * K + k, base = ck * N * 4;
        int num = p.num[ck];
        num = num < 0 ? 0 : (num > N ? N : num);
        const bool jit = p.factors != nullptr && p.jitter != nullptr && p.jitter[ck] != 0;
        const int mode = p.mode[ck];
        // 1. jitter: all N slots (the padded ones too: compute_alignment reads them)
        for (int e = 0; e < N * 4; e++) {
            float v = p.in[base + e];
            if (jit) v = v * p.factors[base + e];
            sb[e][tid] = v;
        }
        // 2. alignment
        if (mode == 1) {            // xc of ALL slots = mean xc of the valid prefix
            float s = 0.f;
            for (int i = 0; i < num; i++) s = s + BX(i, 0);
            const float m = s / (float)num;
            for (int i = 0; i < N; i++) BX(i, 0) = m;
        } else if (mode == 2) {     // left edges of the valid prefix to their mean
            float s = 0.f;
            for (int i = 0; i < num; i++) s = s + (BX(i, 0) - BX(i, 2) / 2.f);
            const float m = s / (float)num;
            for (int i = 0; i < num; i++) {
                const float x1 = BX(i, 0) - BX(i, 2) / 2.f;
                BX(i, 0) = BX(i, 0) - (x1 - m);
            }
        }
        // 3. de_overlap: two sequential passes over the ordered pairs, every read sees the current value
        if (mode == 1 || mode == 2) {
            for (int i = 0; i < num; i++)
                for (int j = 0; j < num; j++) {
                    if (i == j) continue;
                    const float yc1 = BX(i, 1), yc2 = BX(j, 1);
                    const float hh = BX(i, 3) / 2.f + BX(j, 3) / 2.f, ad = fabsf(yc2 - yc1);
                    if (ad < hh) {
                        const float half = (hh - ad) / 2.f;
                        if (yc1 < yc2) { BX(i, 1) = yc1 - half; BX(j, 1) = yc2 + half; }
                        else           { BX(i, 1) = yc1 + half; BX(j, 1) = yc2 - half; }
                    }
                }
            for (int i = 0; i < num; i++)
                for (int j = 0; j < num; j++) {
                    if (i == j) continue;
                    const float hh = BX(i, 3) / 2.f + BX(j, 3) / 2.f, ad = fabsf(BX(j, 1) - BX(i, 1));
                    if (ad < hh) {
                        const float half = (hh - ad) / 2.f;
                        BX(i, 3) = BX(i, 3) - half;
                        BX(j, 3) = BX(j, 3) - half;
                    }
                }
        }
        for (int e = 0; e < N * 4; e++) p.out[base + e] = sb[e][tid];
        // 4. compute_overlap: padded boxes are zeroed (they intersect nothing), nan_to_num(ai / a1) summed over the pairs, / number of valid boxes
        const float fnum = (float)num;
        float ov = 0.f;
        for (int i = 0; i < num; i++) {
            const float l1 = BX(i, 0) - BX(i, 2) / 2.f, t1 = BX(i, 1) - BX(i, 3) / 2.f, r1 = BX(i, 0) + BX(i, 2) / 2.f, b1 = BX(i, 1) + BX(i, 3) / 2.f;
            const float a1 = (r1 - l1) * (b1 - t1);
            for (int j = 0; j < num; j++) {
                if (j == i) continue;
                const float l2 = BX(j, 0) - BX(j, 2) / 2.f, t2 = BX(j, 1) - BX(j, 3) / 2.f, r2 = BX(j, 0) + BX(j, 2) / 2.f, b2 = BX(j, 1) + BX(j, 3) / 2.f;
                const float lmx = fmaxf(l1, l2), rmn = fminf(r1, r2), tmx = fmaxf(t1, t2), bmn = fminf(b1, b2);
                if (!((lmx < rmn) && (tmx < bmn))) continue;
                float ar = ((rmn - lmx) * (bmn - tmx)) / a1;
                if (ar != ar) ar = 0.f;                                    // nan_to_num: nan -> 0, +-inf -> +-FLT_MAX
                else if (ar > 3.4028234663852886e38f) ar = 3.4028234663852886e38f;
                else if (ar < -3.4028234663852886e38f) ar = -3.4028234663852886e38f;
                ov = ov + ar;
            }
        }
        ov = ov / fnum;
        // compute_alignment: valid rows against ALL other slots (the reference masks rows only), min over the six edge / centre coordinates
        float al = 0.f;
        for (int i = 0; i < num; i++) {
            const float xi[6] = {BX(i, 0) - BX(i, 2) / 2.f, BX(i, 0), BX(i, 0) + BX(i, 2) / 2.f, BX(i, 1) - BX(i, 3) / 2.f, BX(i, 1), BX(i, 1) + BX(i, 3) / 2.f};
            float best = 1.f;                                              // the diagonal entries are 1
            bool nan = false;
            for (int j = 0; j < N; j++) {
                if (j == i) continue;
                const float xj[6] = {BX(j, 0) - BX(j, 2) / 2.f, BX(j, 0), BX(j, 0) + BX(j, 2) / 2.f, BX(j, 1) - BX(j, 3) / 2.f, BX(j, 1), BX(j, 1) + BX(j, 3) / 2.f};
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    const float d = fabsf(xi[q] - xj[q]);
                    nan = nan || d != d;                                   // torch's min propagates NaN
                    best = d < best ? d : best;
                }
            }
            if (nan) best = __builtin_nanf("");
            if (best != 1.f) al = al + -logf(1.f - best);
        }
        al = al / fnum;
        p.overlap[ck] = ov;
        p.alignment[ck] = al;
        sov[k] = ov;
    }
#undef BX
    __syncthreads();
    // 5. ranking: count-based, stable, NaN last
    for (int k = tid; k < K; k += LF_THREADS) {
        const float v = sov[k];
        int rank = 0;
        for (int j = 0; j < K; j++) {
            const float u = sov[j];
            rank += (lf_less(u, v) || (lf_equal(u, v) && j < k)) ? 1 : 0;
        }
        p.order[(long)c * K + rank] = k;
    }
}

}  // namespace ldetr

using namespace ldetr;

extern "C" int ldetr_layout_finish_f32(const float* bbox_in, const int* num, const float* factors, const unsigned char* jitter,
                                       const unsigned char* mode, float* bbox_out, float* overlap, float* alignment, int* order,
                                       int C, int K, int N, void* stream) {
    LDETR_CHECK(C >= 0 && K >= 0, "layout_finish: negative C or K (got C = %d, K = %d)", C, K);
    LDETR_CHECK(N >= 1 && N <= LF_MAX_N, "layout_finish: needs 1 <= N <= 16 boxes per layout (got %d)", N);
    if ((long)C * K == 0) return LDETR_OK;
    LDETR_CHECK(K <= LF_MAX_K, "layout_finish: needs 1 <= K <= 1024 candidates per condition (got %d)", K);
    LDETR_CHECK(bbox_in, "layout_finish: bbox_in is null");
    LDETR_CHECK(num && mode, "layout_finish: num or mode is null");
    LDETR_CHECK(bbox_out && overlap && alignment && order, "layout_finish: null output pointer");
    LayoutFinishParams p; memset(&p, 0, sizeof(p));
    p.in = bbox_in; p.num = num; p.factors = factors; p.jitter = jitter; p.mode = mode;
    p.out = bbox_out; p.overlap = overlap; p.alignment = alignment; p.order = order; p.K = K; p.N = N;
    hipLaunchKernelGGL(layout_finish_kernel, dim3((unsigned)C), LF_THREADS, 0, (hipStream_t)stream, p);
    return check_launch("layout_finish");
}
