// Evaluation / inference head (model/stage.py:440-467, 526-536 with self.training == False; inference.py:13-35): the span that
// get_proposals finds for EVERY candidate row, the windowed + global pooling of the row, and the writer's span decoder.  No
// backward exists for any of it.  Latency class (last row): R = N * NA rows (80 at the published batch), one
// workgroup of 256 threads per row; every per-row search is O(Li) in time and LDS, Li <= EVAL_MAX_LI.
//
// Memory safety: every index into a row is built from loop bounds below Li or from a scan / reduction result that starts at 0 and
// is only ever replaced by the index of an element below Li (an out-of-range slot holds -inf and never wins a strict compare).
#include "head_shared.h"     // EVAL_MAX_LI, block_scan_max_first, block_argmax_first, answer_span_decode
#include "../../include/stage_hip.h"

namespace {

// Span of one candidate row r = (n, a) (model/stage.py:440-448, model/model_utils.py:92-123): softmax over the frames of the start
// and end scores -- span_kernel's arithmetic: expf(v - max), block sum in fixed order, divide -- then the arg max of
// fl(p_st[i] * p_ed[j]) over i <= j, ties: the smallest flat index i * Li + j (STAGE._best_span).  O(Li): probabilities are >= 0 and
// fp32 multiplication is monotone, so with sm[i] = max(p_ed[i:]) the row maximum of row i is fl(p_st[i] * sm[i]); the winning start
// is the smallest i whose OWN row maximum equals the overall maximum V (a smaller p_st[i] than the running maximum can still round
// to V), the winning end the smallest j >= i with fl(p_st[i] * p_ed[j]) == V.  A row without any comparable product (NaN scores)
// gives (0, 0) with confidence 0, as span_kernel does.
// span (R, 2) [st, ed] and conf (R) may be NULL; win (R, 2) = the pooling window [max(0, st - extra), min(Li, ed + 1 + extra)).
__global__ __launch_bounds__(256) void eval_span_kernel(const float* __restrict__ t_scores, int* __restrict__ span,
                                                        float* __restrict__ conf, int* __restrict__ win, int Li, int extra) {
    __shared__ float ps[EVAL_MAX_LI], pe[EVAL_MAX_LI], sm[EVAL_MAX_LI], sh[4];
    __shared__ float bv[256];
    __shared__ int bi[256], shi[4];
    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const float* x = t_scores + r * Li * 2;
    float m0 = -INFINITY, m1 = -INFINITY;
    for (int i = tid; i < Li; i += 256) {
        const float2 v = reinterpret_cast<const float2*>(x)[i];
        m0 = fmaxf(m0, v.x);
        m1 = fmaxf(m1, v.y);
    }
    m0 = block_max256(m0, sh);
    m1 = block_max256(m1, sh);
    float s0 = 0.f, s1 = 0.f;
    for (int i = tid; i < Li; i += 256) {
        const float2 v = reinterpret_cast<const float2*>(x)[i];
        const float e0 = expf(v.x - m0), e1 = expf(v.y - m1);
        ps[i] = e0;
        pe[i] = e1;
        s0 += e0;
        s1 += e1;
    }
    s0 = block_sum256(s0, sh);
    s1 = block_sum256(s1, sh);
    for (int i = tid; i < Li; i += 256) {
        ps[i] = ps[i] / s0;
        pe[i] = pe[i] / s1;
    }
    __syncthreads();
    block_scan_max_first(pe, sm, nullptr, Li, true, sh, shi);
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int i = tid; i < Li; i += 256) {
        const float v = ps[i] * sm[i];
        if (v > best) { best = v; bidx = i; }               // ascending i, strict >: this thread's first maximum
    }
    block_argmax_first(best, bidx, bv, bi);
    const float V = best;
    const int st = bidx == 0x7fffffff ? 0 : bidx;
    const float a = ps[st];
    float hit = -INFINITY;
    int ed = 0x7fffffff;
    for (int j = st + tid; j < Li; j += 256)
        if (a * pe[j] == V && j < ed) { hit = 0.f; ed = j; }
    block_argmax_first(hit, ed, bv, bi);
    if (ed == 0x7fffffff) ed = st;
    if (tid == 0) {
        if (span) {
            span[2 * r] = st;
            span[2 * r + 1] = ed;
        }
        if (conf) conf[r] = fmaxf(V, 0.f);
        win[2 * r] = max(0, st - extra);
        win[2 * r + 1] = min(Li, ed + 1 + extra);
    }
}

__device__ __forceinline__ void max4(float4& b, const float4 w) {
    if (w.x > b.x) b.x = w.x;
    if (w.y > b.y) b.y = w.y;
    if (w.z > b.z) b.z = w.z;
    if (w.w > b.w) b.w = w.w;
}

// Pooling of one row: first (R, Li, D) and mask (R, Li) are read ONCE; pooled[r, 0:D] = masked max over the row's own window,
// pooled[r, D:2D] = masked max over all frames (local == 0: only the latter, D wide).  masked_max_fwd_kernel's arithmetic,
// x * m + (1 - m) * (-1e10), and its strict compare; a maximum of non-NaN values does not depend on the order, so the frame tiling
// is free: thread (g, q) = (tid / D4, tid % D4) takes the float4 column q of the frames g, g + G, ... (G = 256 / D4 >= 2 frame
// groups), four loads in flight, and the groups are folded through LDS.
__global__ __launch_bounds__(256) void eval_pool_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                        const int* __restrict__ win, float* __restrict__ pooled, int Li, int D4,
                                                        int local) {
    __shared__ float4 sg[256], sl[256];
    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const int G = 256 / D4, g = tid / D4, q = tid % D4;
    int ws = 0, we = 0;
    if (local) {
        ws = max(0, win[2 * r]);
        we = min(Li, win[2 * r + 1]);
    }
    float4 bg = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), bl = bg;
    if (g < G) {
        const float* px = x + (r * Li) * (long)D4 * 4 + 4 * q;
        const float* pm = m + r * Li;
        for (int l0 = g; l0 < Li; l0 += 4 * G) {
            float4 v[4];
            float mk[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int l = min(l0 + u * G, Li - 1);
                v[u] = ld4s(px + (long)l * D4 * 4);
                mk[u] = pm[l];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int l = l0 + u * G;
                if (l < Li) {
                    const float off = (1.0f - mk[u]) * STAGE_NEG;
                    const float4 w = make_float4(v[u].x * mk[u] + off, v[u].y * mk[u] + off, v[u].z * mk[u] + off, v[u].w * mk[u] + off);
                    max4(bg, w);
                    if (l >= ws && l < we) max4(bl, w);
                }
            }
        }
    }
    sg[tid] = bg;
    sl[tid] = bl;
    __syncthreads();
    // fold the G frame groups: slot (g, q) with g < o takes (g + o, q)
    int top = 1;
    while (top < G) top <<= 1;
    for (int o = top >> 1; o > 0; o >>= 1) {
        if (g < o && g + o < G) {
            float4 a = sg[tid], b = sl[tid];
            max4(a, sg[tid + o * D4]);
            max4(b, sl[tid + o * D4]);
            sg[tid] = a;
            sl[tid] = b;
        }
        __syncthreads();
    }
    if (g == 0) {
        if (local) {
            float* po = pooled + r * (long)D4 * 8 + 4 * q;
            st4(po, sl[tid]);
            st4(po + D4 * 4, sg[tid]);
        } else {
            st4(pooled + r * (long)D4 * 4 + 4 * q, sg[tid]);
        }
    }
}

// The prediction writer's decoder for a batch (inference.py:13-35; evaluation.find_max_pair_batch is the specification): per
// example the FIRST arg max of answer[n, :], then over the softmaxed t_prob[n, pred, :, 0 / 1] the sweep that carries the first arg
// max of p_st[:i + 1] and ends at the first position reaching the best product run_max[i] * p_ed[i] (fp32, one multiplication, as
// the specification forms it); a best product <= 0 gives (0, 1).  out (N, 3) int32 [st, ed, answer].  NaN-free input.
__global__ __launch_bounds__(256) void answer_span_kernel(const float* __restrict__ answer, const float* __restrict__ t_prob,
                                                          int* __restrict__ out, int NA, int Li) {
    __shared__ AnswerSpanLds L;
    const long n = blockIdx.x;
    int st, ed, pred;
    answer_span_decode(answer, t_prob, n, NA, Li, L, st, ed, pred);
    if (threadIdx.x == 0) {
        out[3 * n] = st;
        out[3 * n + 1] = ed;
        out[3 * n + 2] = pred;
    }
}
}  // namespace

extern "C" int stage_eval_head_supported(int Li, int D, int local) {
    (void)local;
    return (Li >= 1 && Li <= EVAL_MAX_LI && D >= 4 && D % 4 == 0 && 2 * D <= 1024) ? 1 : 0;
}

// launchers of the two kernels for the group entry (csrc/groups.hip, G7); shapes are checked there
int stage_eval_span_launch(const float* t_scores, int* span, float* conf, int* win, long long R, int Li, int extra, void* st) {
    hipLaunchKernelGGL(eval_span_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)st, t_scores, span, conf, win, Li, extra);
    STAGE_LAUNCH_CHECK();
    return 0;
}
int stage_eval_pool_launch(const float* first, const float* mask, const int* win, float* pooled, long long R, int Li, int D, int local,
                           void* st) {
    hipLaunchKernelGGL(eval_pool_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)st, first, mask, win, pooled, Li, D / 4, local);
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_answer_spans(const float* answer, const float* t_prob, int* out, int N, int NA, int Li, void* st) {
    if (N < 0 || NA < 1 || NA > 64 || Li < 1 || Li > EVAL_MAX_LI || ((uintptr_t)t_prob & 7)) return STAGE_ERR_SHAPE;
    if (N == 0) return 0;
    hipLaunchKernelGGL(answer_span_kernel, dim3(N), dim3(256), 0, (hipStream_t)st, answer, t_prob, out, NA, Li);
    STAGE_LAUNCH_CHECK();
    return 0;
}
