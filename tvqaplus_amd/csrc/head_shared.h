// Device code that more than one translation unit runs with the SAME arithmetic: the block scans of the evaluation head, the
// prediction writer's span decoder (stage_answer_spans and stage_meter_spans) and the caller's loss line (stage_train_loss and
// stage_train_loss_meter).  Everything is __forceinline__: each kernel gets its own copy of one definition, so two entry points
// that promise identical bits cannot drift apart.
#pragma once
#include "common.h"

#define EVAL_MAX_LI 2048     // = SPAN_MAX_LI of csrc/groups.hip
#define EVAL_SCAN_PER 8      // EVAL_MAX_LI / 256: elements per thread of the block scan

// Inclusive running maximum of n <= EVAL_MAX_LI LDS floats together with the FIRST position that attains it (a later element
// only takes over with a strictly larger value, as torch.cummax's first-occurrence indices restricted to strict increases and
// evaluation.find_max_pair's `lead`).  rev: the scan runs from the last element down (suffix maximum; the index is then the LAST
// position of the maximum).  out_i may be NULL.  All 256 threads call it; v must be complete (barrier) before the call, the
// outputs are complete (barrier) when it returns; out_v / out_i must not alias v.  shv / shi: 4 words of LDS each.
__device__ __forceinline__ void block_scan_max_first(const float* v, float* out_v, int* out_i, int n, bool rev, float* shv,
                                                     int* shi) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float loc[EVAL_SCAN_PER];
    float bv = -INFINITY;
    int bi = 0;
#pragma unroll
    for (int u = 0; u < EVAL_SCAN_PER; u++) {
        const int k = tid * EVAL_SCAN_PER + u;
        const float x = k < n ? v[rev ? n - 1 - k : k] : -INFINITY;
        loc[u] = x;
        if (x > bv) { bv = x; bi = k; }
    }
    // inclusive scan of the thread aggregates inside the wave: combine(left, right) = right.v > left.v ? right : left
    float sv = bv;
    int si = bi;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float pv = __shfl_up(sv, o);
        const int pi = __shfl_up(si, o);
        if (lane >= o && !(sv > pv)) { sv = pv; si = pi; }
    }
    if (lane == 63) { shv[w] = sv; shi[w] = si; }
    const float lv = __shfl_up(sv, 1);       // aggregate of the wave's lanes before this one
    const int li = __shfl_up(si, 1);
    __syncthreads();
    float ev = -INFINITY;                    // everything before this thread's first element
    int ei = 0;
    for (int ww = 0; ww < w; ww++)
        if (shv[ww] > ev) { ev = shv[ww]; ei = shi[ww]; }
    if (lane > 0 && lv > ev) { ev = lv; ei = li; }
#pragma unroll
    for (int u = 0; u < EVAL_SCAN_PER; u++) {
        const int k = tid * EVAL_SCAN_PER + u;
        if (loc[u] > ev) { ev = loc[u]; ei = k; }
        if (k < n) {
            const int pos = rev ? n - 1 - k : k;
            out_v[pos] = ev;
            if (out_i) out_i[pos] = rev ? n - 1 - ei : ei;
        }
    }
    __syncthreads();
}

// (largest value, smallest index among its holders) over the workgroup; every thread returns the result.  A thread that holds
// nothing passes (-inf, INT_MAX).  bv / bi: 256 words of LDS each.
__device__ __forceinline__ void block_argmax_first(float& val, int& idx, float* bv, int* bi) {
    const int tid = threadIdx.x;
    __syncthreads();
    bv[tid] = val;
    bi[tid] = idx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float v2 = bv[tid + o];
            const int i2 = bi[tid + o];
            if (v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid])) { bv[tid] = v2; bi[tid] = i2; }
        }
        __syncthreads();
    }
    val = bv[0];
    idx = bi[0];
}

// LDS of one span decode (34 KB): a kernel declares ONE __shared__ instance and hands it to answer_span_decode.
struct AnswerSpanLds {
    float ps[EVAL_MAX_LI], pe[EVAL_MAX_LI], rm[EVAL_MAX_LI], sh[4];
    int lead[EVAL_MAX_LI];
    float bv[256];
    int bi[256], shi[4];
};

// The prediction writer's decoder for example n (inference.py:13-35; evaluation.find_max_pair_batch is the specification): the
// FIRST arg max of answer[n, :], then over the softmaxed t_prob[n, pred, :, 0 / 1] the sweep that carries the first arg max of
// p_st[:i + 1] and ends at the first position reaching the best product run_max[i] * p_ed[i] (fp32, one multiplication, as the
// specification forms it); a best product <= 0 gives (0, 1).  NaN-free input.  All 256 threads call it and every thread returns the
// same (st, ed, pred).  A caller that decodes several examples puts a barrier between two calls (the next call rewrites L).
// Memory safety: ed is either the index of an element below Li or replaced by 1 with st = 0; lead[] is only read at such an ed.
__device__ __forceinline__ void answer_span_decode(const float* __restrict__ answer, const float* __restrict__ t_prob, long n, int NA,
                                                   int Li, AnswerSpanLds& L, int& st_out, int& ed_out, int& pred_out) {
    const int tid = threadIdx.x;
    int pred = 0;
    float top = -INFINITY;
    for (int a = 0; a < NA; a++) {           // NA <= 64 words, the same for every thread: broadcast reads
        const float v = answer[n * NA + a];
        if (v > top) { top = v; pred = a; }
    }
    const float* x = t_prob + (n * NA + pred) * (long)Li * 2;
    for (int i = tid; i < Li; i += 256) {
        const float2 v = reinterpret_cast<const float2*>(x)[i];
        L.ps[i] = v.x;
        L.pe[i] = v.y;
    }
    __syncthreads();
    block_scan_max_first(L.ps, L.rm, L.lead, Li, false, L.sh, L.shi);
    float best = -INFINITY;
    int ed = 0x7fffffff;
    for (int i = tid; i < Li; i += 256) {
        const float v = L.rm[i] * L.pe[i];
        if (v > best) { best = v; ed = i; }
    }
    block_argmax_first(best, ed, L.bv, L.bi);
    int st = 0;
    if (ed == 0x7fffffff || !(best > 0.f)) {
        ed = 1;
    } else {
        st = L.lead[ed];
    }
    st_out = st;
    ed_out = ed;
    pred_out = pred;
}

// The caller's loss line (main.py:55-60), part 1: dlogits (P, C) = scale * (softmax - onehot) and the block-wide sum of the row cross
// entropies (every thread returns it; fixed order).  scale = scale_dev[0] if given, else scale_host.  A target outside [0, C) is
// ignored like F.cross_entropy's ignore_index (-100) when negative, NaN otherwise (the eager call raises).  sh: 4 floats of LDS.
__device__ __forceinline__ float train_loss_rows(const float* __restrict__ logits, const long long* __restrict__ targets, float scale,
                                                 float* __restrict__ dlogits, int P, int C, float* sh) {
    const int tid = threadIdx.x;
    float ce = 0.f;
    for (int r = tid; r < P; r += 256) {
        const float* x = logits + (long)r * C;
        float m = -INFINITY;
        for (int c = 0; c < C; c++) m = fmaxf(m, x[c]);
        float sum = 0.f;
        for (int c = 0; c < C; c++) sum += expf(x[c] - m);
        const float lse = m + logf(sum);
        const long long t = targets[r];
        const bool ign = t < 0;
        for (int c = 0; c < C; c++) dlogits[(long)r * C + c] = ign ? 0.f : scale * (expf(x[c] - lse) - (c == (int)t ? 1.f : 0.f));
        ce += ign ? 0.f : (t < C ? lse - x[(int)t] : NAN);
    }
    return block_sum256(ce, sh);
}
// part 2 (one thread): the value of the line from the summed cross entropy
__device__ __forceinline__ float train_loss_value(float ce, float scale, const float* __restrict__ att_loss,
                                                  const float* __restrict__ t_loss, float att_w, float ts_w) {
    return ce * scale + (att_loss ? att_w * att_loss[0] : 0.f) + (t_loss ? ts_w * t_loss[0] : 0.f);
}
