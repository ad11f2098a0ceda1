// Flat Adam (main.py:63-66: clip_grad_norm_(10) + torch.optim.Adam.step): the clip and the update on the packed gradient buffer
// (tvqaplus_amd/parallel.py: FlatGradBucket.flat) in two launches, with no float atomics and no device read-back.  Memory bound:
// at hsz 128 the step moves ~15 MB (gradients read twice, two moments and the parameters read and written), so what this file
// buys is launches and host time, not bandwidth (include/stage_hip.h "Flat Adam").
//
//   index space   T fp32 elements of `flat`; m and v are flat buffers of the same layout; the parameters stay where they are
//   seg table     per parameter 3 x int64: device address of its data, start offset in flat, numel
//   chunk table   per chunk 3 x int32: segment, offset inside the segment, length (<= FA_CHUNK, never across a segment boundary)
//   step, active  per segment: float step count (torch keeps Adam's step per parameter), one byte "has a gradient in this step"
//
// Summation order: a thread squares 4 consecutive elements ((x0^2 + x1^2) + (x2^2 + x3^2)), the wave and the workgroup add in the
// fixed tree of common.h, one partial per FA_CHUNK elements of flat; every workgroup of the update kernel adds the partials again,
// each thread its stride-256 subsequence in index order and then the same tree -- the same bits in every workgroup and every run.
//
// Memory safety: a chunk is applied only when its segment index is below n_seg and start + offset + length <= total (a table that
// does not match the buffers is skipped, never followed); inside a chunk every element index is below its length.
#include "common.h"
#include "../../include/stage_hip.h"

#define FA_CHUNK 1024        // elements per chunk and per partial sum: 256 threads x 4
#define FA_THREADS 256

namespace {

struct FaCoef {
    float coef;        // clip factor min(1, max_norm / (norm + 1e-6)); 1 without a clip
    float w1, b2, w2;  // 1 - beta1, beta2, 1 - beta2
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float eps, wd;
};

// one element of torch's Adam (torch/optim/adam.py: _single_tensor_adam; the same fp32 expressions as its fused kernel)
__device__ __forceinline__ void fa_elem(float gin, float& p, float& m, float& v, float& gout, const FaCoef& c) {
    gout = c.coef * gin;
    const float g = gout + c.wd * p;
    m = m + c.w1 * (g - m);
    v = c.b2 * v + c.w2 * (g * g);
    p = p - c.step_size * m / (sqrtf(v) / c.bc2_sqrt + c.eps);
}

}  // namespace

__global__ __launch_bounds__(FA_THREADS) void flat_adam_sumsq_kernel(const float* __restrict__ flat, float* __restrict__ partial,
                                                                     float* __restrict__ step,
                                                                     const unsigned char* __restrict__ active, long long total,
                                                                     int n_seg) {
    __shared__ float sh[4];
    const long long i = (long long)blockIdx.x * FA_CHUNK + threadIdx.x * 4;
    float s = 0.f;
    if (i + 3 < total) {                      // flat is 16-byte aligned (checked by the entry point) and i a multiple of 4
        const float4 x = ld4(flat + i);
        s = (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
    } else if (i < total) {
        const float x0 = flat[i], x1 = i + 1 < total ? flat[i + 1] : 0.f, x2 = i + 2 < total ? flat[i + 2] : 0.f;
        s = (x0 * x0 + x1 * x1) + (x2 * x2);
    }
    s = block_sum256(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
    // the step counts of this step's active parameters: written here, only read by the update kernel
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < n_seg; k += FA_THREADS)
            if (active[k]) step[k] += 1.0f;
}

__global__ __launch_bounds__(FA_THREADS) void flat_adam_update_kernel(float* __restrict__ flat, float* __restrict__ m_buf,
                                                                      float* __restrict__ v_buf,
                                                                      const long long* __restrict__ seg_table, int n_seg,
                                                                      const int* __restrict__ chunk_table,
                                                                      const float* __restrict__ step,
                                                                      const unsigned char* __restrict__ active,
                                                                      const float* __restrict__ partial, int n_part,
                                                                      long long total, float lr, double beta1, double beta2,
                                                                      float eps, float wd, float max_norm,
                                                                      float* __restrict__ norm_out) {
    __shared__ float sh[4], bc[2];
    const int tid = threadIdx.x;
    const int seg = chunk_table[3 * blockIdx.x], off = chunk_table[3 * blockIdx.x + 1], len = chunk_table[3 * blockIdx.x + 2];
    bool live = seg >= 0 && seg < n_seg && off >= 0 && len > 0 && len <= FA_CHUNK;
    long long start = 0;
    float* p = nullptr;
    if (live) {
        p = reinterpret_cast<float*>(seg_table[3 * seg]);
        start = seg_table[3 * seg + 1];
        const long long numel = seg_table[3 * seg + 2];
        live = p != nullptr && start >= 0 && (long long)off + len <= numel && start + numel <= total && active[seg] != 0;
    }
    if (!live && blockIdx.x != 0) return;      // (workgroup-uniform) an inactive segment is not touched at all

    float acc = 0.f;
    for (int k = tid; k < n_part; k += FA_THREADS) acc += partial[k];
    const float norm = sqrtf(block_sum256(acc, sh));
    if (blockIdx.x == 0 && tid == 0) *norm_out = norm;
    if (!live) return;

    // the two bias corrections: double arithmetic (as torch forms them), by ONE lane of the workgroup, handed round through LDS
    // (words of their own: other waves may still be reading sh[] for the sum above)
    if (tid == 0) {
        const double t = (double)step[seg];
        bc[0] = (float)((double)lr / (1.0 - pow(beta1, t)));
        bc[1] = (float)sqrt(1.0 - pow(beta2, t));
    }
    __syncthreads();
    FaCoef c;
    c.coef = max_norm > 0.f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
    c.w1 = (float)(1.0 - beta1);
    c.b2 = (float)beta2;
    c.w2 = (float)(1.0 - beta2);
    c.step_size = bc[0];
    c.bc2_sqrt = bc[1];
    c.eps = eps;
    c.wd = wd;
    const bool store_g = c.coef != 1.0f;       // coef == 1: the product is the gradient itself, flat keeps its bits

    p += off;
    const long long base = start + off;
    float* g = flat + base;
    float* m = m_buf + base;
    float* v = v_buf + base;
    const bool vec = ((base & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0);   // m_buf / v_buf / flat are 16-byte aligned
    if (vec) {
        const int j = tid * 4;
        if (j + 3 < len) {
            const float4 g4 = ld4(g + j);
            float4 p4 = ld4(p + j), m4 = ld4(m + j), v4 = ld4(v + j), o4;
            fa_elem(g4.x, p4.x, m4.x, v4.x, o4.x, c);
            fa_elem(g4.y, p4.y, m4.y, v4.y, o4.y, c);
            fa_elem(g4.z, p4.z, m4.z, v4.z, o4.z, c);
            fa_elem(g4.w, p4.w, m4.w, v4.w, o4.w, c);
            st4(p + j, p4);
            st4(m + j, m4);
            st4(v + j, v4);
            if (store_g) st4(g + j, o4);
        } else {
            for (int e = j; e < len; e++) {    // the chunk's last, partial group of 4 (at most 3 elements, one thread)
                float pe = p[e], me = m[e], ve = v[e], oe;
                fa_elem(g[e], pe, me, ve, oe, c);
                p[e] = pe;
                m[e] = me;
                v[e] = ve;
                if (store_g) g[e] = oe;
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < FA_CHUNK / FA_THREADS; u++) {
            const int e = u * FA_THREADS + tid;
            if (e < len) {
                float pe = p[e], me = m[e], ve = v[e], oe;
                fa_elem(g[e], pe, me, ve, oe, c);
                p[e] = pe;
                m[e] = me;
                v[e] = ve;
                if (store_g) g[e] = oe;
            }
        }
    }
}

extern "C" size_t stage_flat_adam_ws_bytes(long long total) {
    if (total <= 0) return 0;
    const long long parts = (total + FA_CHUNK - 1) / FA_CHUNK;
    return (size_t)((parts * 4 + 255) / 256 * 256);
}

extern "C" int stage_flat_adam_step(float* flat, float* m, float* v, const long long* seg_table, int n_seg, const int* chunk_table,
                                    int n_chunk, float* step, const unsigned char* active, long long total, float lr,
                                    const double* betas_host, float eps, float weight_decay, float max_norm, void* ws, size_t ws_bytes,
                                    float* norm_out, void* stream) {
    if (!flat || !m || !v || !seg_table || !chunk_table || !step || !active || !betas_host || !ws || !norm_out) return STAGE_ERR_SHAPE;
    if (total <= 0 || n_seg <= 0 || n_chunk <= 0) return STAGE_ERR_SHAPE;
    const long long parts = (total + FA_CHUNK - 1) / FA_CHUNK;
    if (parts > 0x7fffffffLL) return STAGE_ERR_SHAPE;
    if (((uintptr_t)flat | (uintptr_t)m | (uintptr_t)v) & 15) return STAGE_ERR_SHAPE;
    if (ws_bytes < stage_flat_adam_ws_bytes(total)) return STAGE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)ws;
    hipLaunchKernelGGL(flat_adam_sumsq_kernel, dim3((unsigned)parts), dim3(FA_THREADS), 0, st, flat, partial, step, active, total,
                       n_seg);
    STAGE_LAUNCH_CHECK();
    hipLaunchKernelGGL(flat_adam_update_kernel, dim3((unsigned)n_chunk), dim3(FA_THREADS), 0, st, flat, m, v, seg_table, n_seg,
                       chunk_table, step, active, partial, (int)parts, total, lr, betas_host[0], betas_host[1], eps, weight_decay, max_norm,
                       norm_out);
    STAGE_LAUNCH_CHECK();
    return 0;
}
