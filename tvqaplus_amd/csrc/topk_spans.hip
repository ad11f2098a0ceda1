// Top-K span proposals of a row of start / end scores (model/model_utils.py:92-123 find_max_triples with topN = K > 1;
// model/stage.py:389-438 get_proposals(max_num_proposal = K)): the K pairs (st <= ed) with the largest p_st[st] * p_ed[ed].
//
// Order: value descending, equal values by ascending flat index st * Li + ed (the tie rule of span_kernel, csrc/groups.hip, and
// STAGE._best_span).  No two pairs share a flat index, so this is a TOTAL order and the K best of a row are one definite list: the
// result cannot depend on how the pairs are dealt to threads or in which order lists are merged.
// Arithmetic: span_kernel's -- expf(v - max), block sum in fixed order, divide, one fp32 multiplication per pair -- so rank 0 has the
// bits stage_gt_spans / stage_grp_eval_head_fwd report.
//
// One workgroup of 256 threads per row, O(Li) memory: the probabilities in LDS (16 KB), every thread's K best pairs in registers (K is
// a template parameter and every list access is unrolled with constant indices: no scratch), the 256 lists merged through LDS
// (2 x 256 x K words) in a tree under the same order.  A thread takes row i together with row Li - 1 - i (Li - i and i + 1 pairs: Li + 1
// for every thread).
//
// Memory safety: i and j are loop counters below Li <= TOPK_MAX_LI; LDS slots are tid * K + k with k < K constant; the global writes
// are (row, k < K) of buffers the caller sized by (R, K).
#include "common.h"
#include "../../include/stage_hip.h"

#define TOPK_MAX_LI 2048     // = SPAN_MAX_LI of csrc/groups.hip, EVAL_MAX_LI of csrc/head_shared.h
#define TOPK_MAX_K 8         // = STAGE_TOPK_MAX of include/stage_hip.h
#define TOPK_NONE 0x7fffffff

static_assert(TOPK_MAX_K == STAGE_TOPK_MAX, "include/stage_hip.h and csrc/topk_spans.hip disagree on the largest K");

namespace {

// (v, i) comes before (w, j) in the order above.  A NaN never comes before anything, so it never enters a list.
__device__ __forceinline__ bool span_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

template <int K>
struct SpanList {
    float v[K];
    int i[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < K; k++) {
            v[k] = -INFINITY;
            i[k] = TOPK_NONE;
        }
    }
    // keep the K best of (list, new pair): the pair replaces the last entry and moves up while it comes before its neighbour
    __device__ __forceinline__ void insert(float nv, int ni) {
        if (!span_before(nv, ni, v[K - 1], i[K - 1])) return;
        v[K - 1] = nv;
        i[K - 1] = ni;
#pragma unroll
        for (int k = K - 1; k > 0; k--) {
            const bool up = span_before(v[k], i[k], v[k - 1], i[k - 1]);
            const float tv = v[k - 1];
            const int ti = i[k - 1];
            v[k - 1] = up ? v[k] : tv;
            i[k - 1] = up ? i[k] : ti;
            v[k] = up ? tv : v[k];
            i[k] = up ? ti : i[k];
        }
    }
};

struct TopkLds {
    float ps[TOPK_MAX_LI], pe[TOPK_MAX_LI], sh[4];
    float mv[256 * TOPK_MAX_K];
    int mi[256 * TOPK_MAX_K];
};

// The K best pairs of the row x (Li, 2); every thread of the workgroup calls it, thread 0 returns the row's list (the other threads'
// lists are partial).  is_prob: x holds probabilities, used as given; otherwise scores, softmaxed over the Li frames here.
template <int K>
__device__ __forceinline__ void row_topk(const float* __restrict__ x, int Li, bool is_prob, TopkLds& L, SpanList<K>& best) {
    const int tid = threadIdx.x;
    if (is_prob) {
        for (int i = tid; i < Li; i += 256) {
            const float2 v = reinterpret_cast<const float2*>(x)[i];
            L.ps[i] = v.x;
            L.pe[i] = v.y;
        }
    } else {
        float m0 = -INFINITY, m1 = -INFINITY;
        for (int i = tid; i < Li; i += 256) {
            const float2 v = reinterpret_cast<const float2*>(x)[i];
            m0 = fmaxf(m0, v.x);
            m1 = fmaxf(m1, v.y);
        }
        m0 = block_max256(m0, L.sh);
        m1 = block_max256(m1, L.sh);
        float s0 = 0.f, s1 = 0.f;
        for (int i = tid; i < Li; i += 256) {
            const float2 v = reinterpret_cast<const float2*>(x)[i];
            const float e0 = expf(v.x - m0), e1 = expf(v.y - m1);
            L.ps[i] = e0;
            L.pe[i] = e1;
            s0 += e0;
            s1 += e1;
        }
        s0 = block_sum256(s0, L.sh);
        s1 = block_sum256(s1, L.sh);
        for (int i = tid; i < Li; i += 256) {
            L.ps[i] = L.ps[i] / s0;
            L.pe[i] = L.pe[i] / s1;
        }
    }
    __syncthreads();
    best.clear();
    for (int r = tid; 2 * r < Li; r += 256) {
        const int i0 = r, i1 = Li - 1 - r;
        const float a0 = L.ps[i0];
        for (int j = i0; j < Li; j++) best.insert(a0 * L.pe[j], i0 * Li + j);
        if (i1 != i0) {
            const float a1 = L.ps[i1];
            for (int j = i1; j < Li; j++) best.insert(a1 * L.pe[j], i1 * Li + j);
        }
    }
    // tree merge: the upper half of the live threads hands its lists over through LDS, the lower half inserts them into its own
    for (int o = 128; o > 0; o >>= 1) {
        if (tid >= o && tid < 2 * o) {
#pragma unroll
            for (int k = 0; k < K; k++) {
                L.mv[(tid - o) * K + k] = best.v[k];
                L.mi[(tid - o) * K + k] = best.i[k];
            }
        }
        __syncthreads();
        if (tid < o) {
#pragma unroll
            for (int k = 0; k < K; k++) best.insert(L.mv[tid * K + k], L.mi[tid * K + k]);
        }
        __syncthreads();
    }
}

// rank k of a finished list as (start, end, confidence).  A rank that no pair fills is (-1, -1, 0) -- except rank 0, which is
// (0, 0, 0) as span_kernel reports a row without any comparable product (NaN scores; Li >= 1 always has a pair otherwise).
template <int K>
__device__ __forceinline__ void rank_of(const SpanList<K>& best, int k, int Li, int& st, int& ed, float& conf) {
    const int idx = best.i[k];
    const bool none = idx == TOPK_NONE;
    st = none ? (k == 0 ? 0 : -1) : idx / Li;
    ed = none ? (k == 0 ? 0 : -1) : idx % Li;
    conf = none ? 0.f : fmaxf(best.v[k], 0.f);
}

// training: the ground-truth candidate's row of t_scores (N, NA, Li, 2); spans (3K + 3, N)
template <int K>
__global__ __launch_bounds__(256) void gt_topk_kernel(const float* __restrict__ t_scores, const long long* __restrict__ target,
                                                      const long long* __restrict__ lab_st, const long long* __restrict__ lab_ed,
                                                      float* __restrict__ spans, int N, int NA, int Li) {
    __shared__ TopkLds L;
    const int n = blockIdx.x;
    // (an out-of-range target: the read is clamped, the temporal loss of the example is NaN -- span_kernel, csrc/groups.hip)
    const float* x = t_scores + ((long)n * NA + min(max((int)target[n], 0), NA - 1)) * Li * 2;
    SpanList<K> best;
    row_topk<K>(x, Li, false, L, best);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            int st, ed;
            float conf;
            rank_of<K>(best, k, Li, st, ed, conf);
            spans[(long)(3 * k + 0) * N + n] = (float)st;
            spans[(long)(3 * k + 1) * N + n] = (float)ed;
            spans[(long)(3 * k + 2) * N + n] = conf;
        }
        spans[(long)(3 * K + 0) * N + n] = (float)lab_st[n];
        spans[(long)(3 * K + 1) * N + n] = (float)lab_ed[n];
        spans[(long)(3 * K + 2) * N + n] = (float)target[n];
    }
}

// R independent rows x (R, Li, 2); span (R, K, 2) int32, conf (R, K)
template <int K>
__global__ __launch_bounds__(256) void rows_topk_kernel(const float* __restrict__ x, int is_prob, int* __restrict__ span,
                                                        float* __restrict__ conf, int Li) {
    __shared__ TopkLds L;
    const long r = blockIdx.x;
    SpanList<K> best;
    row_topk<K>(x + r * Li * 2, Li, is_prob != 0, L, best);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            int st, ed;
            float c;
            rank_of<K>(best, k, Li, st, ed, c);
            *reinterpret_cast<int2*>(span + (r * K + k) * 2) = make_int2(st, ed);
            conf[r * K + k] = c;
        }
    }
}

template <int K>
void launch_gt(const float* t_scores, const long long* target, const long long* lab_st, const long long* lab_ed, float* spans, int N,
               int NA, int Li, hipStream_t st) {
    hipLaunchKernelGGL(gt_topk_kernel<K>, dim3(N), dim3(256), 0, st, t_scores, target, lab_st, lab_ed, spans, N, NA, Li);
}
template <int K>
void launch_rows(const float* x, int is_prob, int* span, float* conf, long long R, int Li, hipStream_t st) {
    hipLaunchKernelGGL(rows_topk_kernel<K>, dim3((unsigned)R), dim3(256), 0, st, x, is_prob, span, conf, Li);
}

}  // namespace

#define TOPK_DISPATCH(K, CALL)             \
    switch (K) {                           \
        case 1: CALL(1); break;            \
        case 2: CALL(2); break;            \
        case 3: CALL(3); break;            \
        case 4: CALL(4); break;            \
        case 5: CALL(5); break;            \
        case 6: CALL(6); break;            \
        case 7: CALL(7); break;            \
        default: CALL(8); break;           \
    }

extern "C" int stage_topk_spans_supported(int Li, int K) { return Li >= 1 && Li <= TOPK_MAX_LI && K >= 1 && K <= TOPK_MAX_K; }

extern "C" int stage_gt_spans_topk(const float* t_scores, const long long* target, const long long* lab_st, const long long* lab_ed,
                                   float* spans, int N, int NA, int Li, int K, void* st) {
    if (!stage_topk_spans_supported(Li, K) || NA < 1) return STAGE_ERR_SHAPE;
    if (N <= 0) return 0;
    if (!t_scores || !target || !lab_st || !lab_ed || !spans || ((uintptr_t)t_scores & 7)) return STAGE_ERR_SHAPE;
#define CALL(KK) launch_gt<KK>(t_scores, target, lab_st, lab_ed, spans, N, NA, Li, (hipStream_t)st)
    TOPK_DISPATCH(K, CALL)
#undef CALL
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_topk_spans(const float* x, int is_prob, int* span, float* conf, long long R, int Li, int K, void* st) {
    if (!stage_topk_spans_supported(Li, K) || R < 0 || R > 0x7fffffffLL) return STAGE_ERR_SHAPE;
    if (R == 0) return 0;
    if (!x || !span || !conf || ((uintptr_t)x & 7) || ((uintptr_t)span & 7)) return STAGE_ERR_SHAPE;
#define CALL(KK) launch_rows<KK>(x, is_prob, span, conf, R, Li, (hipStream_t)st)
    TOPK_DISPATCH(K, CALL)
#undef CALL
    STAGE_LAUNCH_CHECK();
    return 0;
}
