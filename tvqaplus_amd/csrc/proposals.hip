// Which spans train the classifier, decided on the device (model/stage.py:411-438 get_proposals in training; model/model_utils.py:37-89):
// the host loop ``tvqaplus_amd.stage.proposal_rows`` as one kernel, writing the bookkeeping of the pooling + classifier group
// (csrc/groups.hip, G6) at a FIXED capacity -- no read-back of the span table, no upload of the rows, no data-dependent shape.
//
//   spans (3K + 3, N) float   what stage_gt_spans (K = 1) / stage_gt_spans_topk write: rows 3j, 3j + 1, 3j + 2 = start, end (inclusive),
//                             confidence of rank j, then the label's start, end (inclusive) and the answer index
//   meta  (5 Pmax) int32      src[Pmax] | win[2 Pmax] | inv[slots N] | tgt[Pmax], slots = K + 1, Pmax = slots N
//   rows [0, P)               proposal_rows' rows in its order: per example the label's span, then the kept ranks in rank order
//   rows [P, Pmax)            src / win of row 0, tgt = -100; no inv entry names them.  (A duplicate of a real row, not an empty window:
//                             an empty window pools to -inf, LayerNorm turns that into NaN, and 0 * NaN would reach the classifier's
//                             weight gradient.  A real row is finite; its dlogits are exact zeros: head_shared.h, train_loss_rows.)
//   count[0] = P, scale[0] = (float)((double)N / (double)P): the bits of the host's float(N) / len(targets) narrowed to fp32
//
// A rank is kept iff (double)conf >= ce_prob_thd, start >= 0, union != 0 and (double)inter / (double)union >= iou_thd, inter / union
// integers over end-exclusive spans: the host's comparisons, in double (np.float32(0.01) < 0.01: a float comparison would keep it).
//
// One workgroup of 256 threads, one example per thread and chunk of 256; the first row of an example = carry of the earlier chunks +
// block-exclusive scan of the chunk's row counts.  Plain stores, no atomics: every word of meta has exactly one writer.
//
// Memory safety: src / win / tgt rows are first + j with first <= slots * n (at most slots rows per earlier example) and j < cnt <=
// slots, so below slots * N = Pmax; padding rows run over [P, Pmax); inv entries are slots * n + j, j < slots, n < N.  Values of
// the table never become an index: a start / end that is negative, non-finite or >= 2^30 makes its rank absent (a NaN confidence
// fails its comparison), the label's words are clamped to +-2^30 and only travel on as VALUES (the pooling kernel clamps windows
// to [0, Li) itself).
#include "common.h"
#include "../../include/stage_hip.h"

namespace {

#define PROP_BIG 1073741824.f      // 2^30: spans beyond it are no spans (and ed + 1 + extra stays an int)

__device__ __forceinline__ int clamp_word(float v) { return (int)fminf(fmaxf(v, -PROP_BIG), PROP_BIG); }     // NaN -> -2^30

// rank j of example n against the label's span [gs, ge): kept?  (ps, pe): its span, end exclusive
__device__ __forceinline__ bool rank_kept(const float* __restrict__ spans, int N, int n, int j, int gs, int ge, double iou_thd,
                                          double prob_thd, int& ps, int& pe) {
    const float st = spans[(long)(3 * j + 0) * N + n], ed = spans[(long)(3 * j + 1) * N + n], conf = spans[(long)(3 * j + 2) * N + n];
    ps = pe = 0;
    if (!((double)conf >= prob_thd)) return false;
    if (!(st >= 0.f && st < PROP_BIG && ed >= 0.f && ed < PROP_BIG)) return false;
    ps = (int)st;
    pe = (int)ed + 1;
    const int inter = max(0, min(pe, ge) - max(ps, gs));
    const int uni = max(pe, ge) - min(ps, gs);
    return uni != 0 && (double)inter / (double)uni >= iou_thd;
}

__global__ __launch_bounds__(256) void proposal_meta_kernel(const float* __restrict__ spans, int N, int K, double iou_thd, double prob_thd,
                                                            int extra, int* __restrict__ meta, int* __restrict__ count,
                                                            float* __restrict__ scale) {
    __shared__ int sc[256];
    const int tid = threadIdx.x;
    const int slots = K + 1;
    const int Pmax = slots * N;
    const int lab = 3 * K;
    int* __restrict__ src = meta;
    int* __restrict__ win = meta + Pmax;
    int* __restrict__ inv = meta + 3 * Pmax;
    int* __restrict__ tgt = meta + 3 * Pmax + slots * N;
    int carry = 0;
    for (int base = 0; base < N; base += 256) {
        const int n = base + tid;
        const bool live = n < N;
        int gs = 0, ge = 0, keep = 0, cnt = 0;
        if (live) {
            gs = clamp_word(spans[(long)lab * N + n]);
            ge = clamp_word(spans[(long)(lab + 1) * N + n]) + 1;
            cnt = 1;                                           // the label's span is always a row
            for (int j = 0; j < K; j++) {
                int ps, pe;
                if (rank_kept(spans, N, n, j, gs, ge, iou_thd, prob_thd, ps, pe)) {
                    keep |= 1 << j;
                    cnt++;
                }
            }
        }
        // inclusive scan of the chunk's counts, fixed order
        sc[tid] = cnt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int first = carry + sc[tid] - cnt;
        carry += sc[255];
        __syncthreads();                                       // sc is rewritten by the next chunk
        if (live) {
            const int t = clamp_word(spans[(long)(lab + 2) * N + n]);
            int r = first;
            src[r] = n;
            win[2 * r] = max(0, gs - extra);
            win[2 * r + 1] = ge + extra;
            tgt[r] = t;
            inv[slots * n] = r;
            r++;
            for (int j = 0; j < K; j++) {
                if (!((keep >> j) & 1)) continue;
                int ps, pe;
                rank_kept(spans, N, n, j, gs, ge, iou_thd, prob_thd, ps, pe);
                src[r] = n;
                win[2 * r] = max(0, ps - extra);
                win[2 * r + 1] = pe + extra;
                tgt[r] = t;
                inv[slots * n + (r - first)] = r;
                r++;
            }
            for (int j = cnt; j < slots; j++) inv[slots * n + j] = -1;
        }
    }
    // carry = P in every thread (all read the same totals).  Padding: row 0 again (example 0, its label's window), ignored target
    const int P = carry;
    const int gs0 = clamp_word(spans[(long)lab * N]);
    const int ge0 = clamp_word(spans[(long)(lab + 1) * N]) + 1;
    for (int r = P + tid; r < Pmax; r += 256) {
        src[r] = 0;
        win[2 * r] = max(0, gs0 - extra);
        win[2 * r + 1] = ge0 + extra;
        tgt[r] = -100;
    }
    if (tid == 0) {
        count[0] = P;
        scale[0] = (float)((double)N / (double)P);
    }
}

}  // namespace

// thd_host: HOST array {iou_thd, ce_prob_thd} as double, read before the call returns and passed to the kernel by value
extern "C" int stage_proposal_meta(const float* spans, int N, int K, const double* thd_host, int extra, int* meta, int* count,
                                   float* scale, void* st) {
    if (K < 1 || K > STAGE_TOPK_MAX || N <= 0 || (long long)N * (K + 1) > 0x7fffffffLL / 5) return STAGE_ERR_SHAPE;
    if (extra < 0 || extra > (1 << 20)) return STAGE_ERR_SHAPE;
    if (!spans || !thd_host || !meta || !count || !scale) return STAGE_ERR_SHAPE;
    hipLaunchKernelGGL(proposal_meta_kernel, dim3(1), dim3(256), 0, (hipStream_t)st, spans, N, K, thd_host[0], thd_host[1], extra, meta,
                       count, scale);
    STAGE_LAUNCH_CHECK();
    return 0;
}
