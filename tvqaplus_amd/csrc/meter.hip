// Run meter (include/stage_hip.h "Run meter"): the statistics a training / validation loop keeps per step (main.py:69-74, 90-94,
// 173-183) and the temporal metrics of eval/eval_tvqa_plus.py:14-69, accumulated in ONE caller-owned device buffer by stream-ordered
// launches -- no read-back until the caller copies the buffer at a log interval.
//
// Latency class: every call is one workgroup of 256 threads.  Rows (P) and examples (N) are walked by stride / block loops, so their
// number is unbounded; the per-call partial counts are reduced by a fixed LDS tree (bitwise repeatable) and one thread adds them to
// the buffer.  No atomics: calls on one stream are ordered, and a meter belongs to one stream.
//
// Memory safety: the buffer is addressed through the fixed offsets below; a ring row is written only at a slot in [0, ring_cap);
// logits / targets / gt rows only at indices below P / N; the span decode as documented in head_shared.h.
#include "head_shared.h"
#include "../../include/stage_hip.h"

#define METER_F 8            // doubles in front of the buffer
#define METER_I 24           // 64-bit counters behind them
#define METER_HEAD_BYTES ((METER_F + METER_I) * 8)
// f[]
#define MF_LOSS 0
#define MF_CLS 1
#define MF_ATT 2
#define MF_TS 3
#define MF_GNORM_SUM 4
#define MF_GNORM_MAX 5
#define MF_IOU 6
// i[]
#define MI_STEPS 0
#define MI_ROWS 1
#define MI_CORRECT 2
#define MI_NONFINITE 3
#define MI_CURSOR 4
#define MI_DROPPED 5
#define MI_SPAN_ROWS 6
#define MI_SPAN_RIGHT 7
#define MI_ASA 8
#define MI_RECALL 9          // 9 .. 17: R@0.1 .. R@0.9
#define MI_GNORM_STEPS 18
#define SPAN_COUNTS 12       // span_rows is N; per call: right, asa, nine bins (+ 1 spare row keeps the table a multiple of 4)

namespace {

struct MeterThd { double v[9]; };

// what one update adds besides the rows; has_* say which pointers the caller gave
struct MeterScalars {
    bool has_loss, has_cls, has_att, has_ts, has_gnorm;
    float loss, cls, att, ts, gnorm;     // att / ts already multiplied by their weights in fp32
};

// sum of one int per thread over the workgroup, fixed tree; every thread returns it.  sh: 256 ints of LDS.
__device__ __forceinline__ int block_tree_isum256(int v, int* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}

// first index holding a NaN if the row has one, otherwise the first index of the maximum: CPU torch's outputs.max(1)[1]
__device__ __forceinline__ int row_pred(const float* __restrict__ x, int C) {
    int pred = 0;
    float m = x[0];
    if (m != m) return 0;
    for (int c = 1; c < C; c++) {
        const float v = x[c];
        if (v != v) return c;
        if (v > m) { m = v; pred = c; }
    }
    return pred;
}

// The update proper.  All 256 threads call it (barriers inside).  rows: logits != NULL && targets != NULL && P > 0.
__device__ __forceinline__ void meter_apply(void* meter, long long ring_cap, const float* __restrict__ logits,
                                            const long long* __restrict__ targets, int P, int C, const MeterScalars& s, int* sh) {
    double* f = reinterpret_cast<double*>(meter);
    long long* iv = reinterpret_cast<long long*>(meter) + METER_F;
    unsigned short* ring = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(meter) + METER_HEAD_BYTES);
    const int tid = threadIdx.x;
    const bool rows = logits != nullptr && targets != nullptr && P > 0;
    int correct = 0;
    long long cursor = 0;
    if (rows) {
        cursor = iv[MI_CURSOR];              // read by every thread before thread 0 rewrites it behind the barriers of the tree
        if (cursor < 0) cursor = 0;
        for (int r = tid; r < P; r += 256) {
            const int pred = row_pred(logits + (long)r * C, C);
            const bool ok = targets[r] == (long long)pred;
            correct += ok ? 1 : 0;
            const long long slot = cursor + r;
            if (slot < ring_cap) ring[slot] = (unsigned short)(pred | (ok ? 0x8000 : 0));
        }
        correct = block_tree_isum256(correct, sh);
    }
    if (tid != 0) return;
    if (rows) {
        const long long end = cursor + P;
        const long long kept_end = end < ring_cap ? end : (cursor > ring_cap ? cursor : ring_cap);
        iv[MI_ROWS] += P;
        iv[MI_CORRECT] += correct;
        iv[MI_CURSOR] = kept_end;
        iv[MI_DROPPED] += end - kept_end;
    }
    if (s.has_loss) {
        f[MF_LOSS] = f[MF_LOSS] + (double)s.loss;
        iv[MI_NONFINITE] += isfinite(s.loss) ? 0 : 1;
    }
    if (s.has_cls) f[MF_CLS] = f[MF_CLS] + (double)s.cls;
    if (s.has_att) f[MF_ATT] = f[MF_ATT] + (double)s.att;
    if (s.has_ts) f[MF_TS] = f[MF_TS] + (double)s.ts;
    if (s.has_loss || s.has_cls || s.has_att || s.has_ts) iv[MI_STEPS] += 1;
    if (s.has_gnorm) {
        const double g = (double)s.gnorm;
        f[MF_GNORM_SUM] = f[MF_GNORM_SUM] + g;
        if (g > f[MF_GNORM_MAX]) f[MF_GNORM_MAX] = g;
        iv[MI_GNORM_STEPS] += 1;
    }
}

__global__ __launch_bounds__(256) void meter_update_kernel(void* meter, long long ring_cap, const float* __restrict__ logits,
                                                           const long long* __restrict__ targets, int P, int C,
                                                           const float* __restrict__ loss, const float* __restrict__ cls,
                                                           const float* __restrict__ att, const float* __restrict__ ts, float att_w,
                                                           float ts_w, const float* __restrict__ grad_norm) {
    __shared__ int sh[256];
    MeterScalars s;
    s.has_loss = loss != nullptr;
    s.has_cls = cls != nullptr;
    s.has_att = att != nullptr;
    s.has_ts = ts != nullptr;
    s.has_gnorm = grad_norm != nullptr;
    s.loss = s.has_loss ? loss[0] : 0.f;
    s.cls = s.has_cls ? cls[0] : 0.f;
    s.att = s.has_att ? __fmul_rn(att_w, att[0]) : 0.f;
    s.ts = s.has_ts ? __fmul_rn(ts_w, ts[0]) : 0.f;
    s.gnorm = s.has_gnorm ? grad_norm[0] : 0.f;
    meter_apply(meter, ring_cap, logits, targets, P, C, s, sh);
}

// stage_train_loss (csrc/groups.hip: train_loss_kernel -- the same two device functions, the same bits in loss and dlogits) and the
// update of the step in the same launch: loss = its own loss, cls = ce * scale, att = att_w * att_loss[0], ts = ts_w * t_loss[0].
__global__ __launch_bounds__(256) void train_loss_meter_kernel(const float* __restrict__ logits, const long long* __restrict__ targets,
                                                               const float* __restrict__ att_loss, const float* __restrict__ t_loss,
                                                               const float* __restrict__ scale_dev, float scale_host, float att_w,
                                                               float ts_w, float* __restrict__ loss, float* __restrict__ dlogits, int P,
                                                               int C, void* meter, long long ring_cap) {
    __shared__ float shf[4];
    __shared__ int sh[256];
    const float scale = scale_dev ? scale_dev[0] : scale_host;
    const float ce = train_loss_rows(logits, targets, scale, dlogits, P, C, shf);
    MeterScalars s;
    s.has_loss = s.has_cls = true;
    s.has_att = att_loss != nullptr;
    s.has_ts = t_loss != nullptr;
    s.has_gnorm = false;
    s.loss = train_loss_value(ce, scale, att_loss, t_loss, att_w, ts_w);
    s.cls = __fmul_rn(ce, scale);
    s.att = s.has_att ? __fmul_rn(att_w, att_loss[0]) : 0.f;
    s.ts = s.has_ts ? __fmul_rn(ts_w, t_loss[0]) : 0.f;
    s.gnorm = 0.f;
    if (threadIdx.x == 0) loss[0] = s.loss;
    meter_apply(meter, ring_cap, logits, targets, P, C, s, sh);
}

// Spans of a validation batch: stage_answer_spans' decode per example (the block works on one example at a time), then in double
// what PredictionWriter.add_batch and evaluation.temporal_iou / compute_temporal_metrics do with the row.  Example n is accounted by
// thread n % 256; the per-thread counts meet in one LDS tree (ints, and an fp64 tree for the IoU sum).
__global__ __launch_bounds__(256) void meter_spans_kernel(void* meter, const float* __restrict__ answer, const float* __restrict__ t_prob,
                                                          const long long* __restrict__ targets, const double* __restrict__ gt,
                                                          MeterThd thd, int N, int NA, int Li, int* __restrict__ rows_out) {
    __shared__ AnswerSpanLds L;
    __shared__ int cnt[SPAN_COUNTS][256];
    __shared__ double dsum[256];
    const int tid = threadIdx.x;
    int c_right = 0, c_asa = 0, c_bin[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double iou_acc = 0.0;
    for (int n = 0; n < N; n++) {
        int st, ed, pred;
        answer_span_decode(answer, t_prob, (long)n, NA, Li, L, st, ed, pred);
        if (tid == 0 && rows_out) {
            rows_out[3 * (long)n] = st;
            rows_out[3 * (long)n + 1] = ed;
            rows_out[3 * (long)n + 2] = pred;
        }
        if (tid == (n & 255)) {
            const double g0 = gt[3 * (long)n], g1 = gt[3 * (long)n + 1], off = gt[3 * (long)n + 2];
            const double p0 = (double)(st * 2) + off, p1 = (double)((ed + 1) * 2) + off;
            // evaluation.temporal_iou with Python's min / max (the first argument unless the second is strictly beyond it)
            const double lo_in = g0 > p0 ? g0 : p0, hi_in = g1 < p1 ? g1 : p1;
            const double d = hi_in - lo_in;
            const double inter = d > 0.0 ? d : 0.0;
            const double hull = (g1 > p1 ? g1 : p1) - (g0 < p0 ? g0 : p0);
            const double iou = hull == 0.0 ? 0.0 : inter / hull;
            const bool right = targets[n] == (long long)pred;
            c_right += right ? 1 : 0;
            c_asa += (right && iou >= 0.5) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 9; k++) c_bin[k] += iou >= thd.v[k] ? 1 : 0;
            iou_acc += iou;
        }
        __syncthreads();                     // the next decode rewrites L
    }
    cnt[0][tid] = c_right;
    cnt[1][tid] = c_asa;
#pragma unroll
    for (int k = 0; k < 9; k++) cnt[2 + k][tid] = c_bin[k];
    dsum[tid] = iou_acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int k = 0; k < 11; k++) cnt[k][tid] += cnt[k][tid + o];
            dsum[tid] = dsum[tid] + dsum[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* f = reinterpret_cast<double*>(meter);
        long long* iv = reinterpret_cast<long long*>(meter) + METER_F;
        iv[MI_SPAN_ROWS] += N;
        iv[MI_SPAN_RIGHT] += cnt[0][0];
        iv[MI_ASA] += cnt[1][0];
        for (int k = 0; k < 9; k++) iv[MI_RECALL + k] += cnt[2 + k][0];
        f[MF_IOU] = f[MF_IOU] + dsum[0];
    }
}

inline bool meter_ok(const void* meter, long long ring_cap) { return meter != nullptr && ring_cap >= 0 && ((uintptr_t)meter & 7) == 0; }

}  // namespace

extern "C" size_t stage_meter_bytes(long long ring_cap) {
    if (ring_cap < 0) return 0;
    return (size_t)METER_HEAD_BYTES + (((size_t)ring_cap * 2 + 7) & ~(size_t)7);
}

extern "C" int stage_meter_reset(void* meter, long long ring_cap, void* st) {
    if (!meter_ok(meter, ring_cap)) return STAGE_ERR_SHAPE;
    const hipError_t e = hipMemsetAsync(meter, 0, stage_meter_bytes(ring_cap), (hipStream_t)st);
    return e == hipSuccess ? 0 : (int)e;
}

extern "C" int stage_meter_update(void* meter, long long ring_cap, const float* logits, const long long* targets, int P, int C,
                                  const float* loss, const float* cls, const float* att, const float* ts, float att_w, float ts_w,
                                  const float* grad_norm, void* st) {
    if (!meter_ok(meter, ring_cap) || P < 0) return STAGE_ERR_SHAPE;
    const bool rows = logits != nullptr && targets != nullptr && P > 0;
    if (rows && (C < 1 || C > 4096)) return STAGE_ERR_SHAPE;
    if (!rows && !loss && !cls && !att && !ts && !grad_norm) return 0;       // nothing to add
    hipLaunchKernelGGL(meter_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)st, meter, ring_cap, logits, targets, P, C, loss, cls, att,
                       ts, att_w, ts_w, grad_norm);
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_train_loss_meter(const float* logits, const long long* targets, const float* att_loss, const float* t_loss,
                                      const float* scale_dev, float scale_host, float att_w, float ts_w, float* loss, float* dlogits,
                                      int P, int C, void* st, void* meter, long long ring_cap) {
    if (P <= 0 || C <= 0 || C > 4096 || !meter_ok(meter, ring_cap) || !logits || !targets || !loss || !dlogits) return STAGE_ERR_SHAPE;
    hipLaunchKernelGGL(train_loss_meter_kernel, dim3(1), dim3(256), 0, (hipStream_t)st, logits, targets, att_loss, t_loss, scale_dev,
                       scale_host, att_w, ts_w, loss, dlogits, P, C, meter, ring_cap);
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_meter_spans(void* meter, const float* answer, const float* t_prob, const long long* targets, const double* gt,
                                 const double* thd_host, int N, int NA, int Li, int* rows_out, void* st) {
    if (!meter_ok(meter, 0) || !answer || !t_prob || !targets || !gt || !thd_host) return STAGE_ERR_SHAPE;
    if (N < 0 || NA < 1 || NA > 64 || Li < 1 || Li > EVAL_MAX_LI || ((uintptr_t)t_prob & 7) || ((uintptr_t)gt & 7)) return STAGE_ERR_SHAPE;
    if (N == 0) return 0;
    MeterThd thd;
    for (int k = 0; k < 9; k++) thd.v[k] = thd_host[k];
    hipLaunchKernelGGL(meter_spans_kernel, dim3(1), dim3(256), 0, (hipStream_t)st, meter, answer, t_prob, targets, gt, thd, N, NA, Li,
                       rows_out);
    STAGE_LAUNCH_CHECK();
    return 0;
}
