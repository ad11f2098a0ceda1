// First stage of the input MLP on HALF-PRECISION feature rows (fp16 or bf16), for the fp32 model:
//     [F.normalize (model/stage.py:256)] -> LayerNorm(K0) + inverted dropout (model/stage.py:85-91, 98-104)
// Loaders store BERT / region features as 16-bit values: a B=16 step reads 862 MB of fp32 features, more than the step's own time
// over PCIe.  The fp32 model used to upcast such features on entry (a fresh fp32 image of the tensor, kept until the backward);
// here the rows are converted IN REGISTERS by the first kernel that touches them.  Neither the fp32 image nor -- on the video
// stream -- the L2-normalised image is written; everything behind the load is the fp32 path's arithmetic.
//
// Same function as stage_l2norm[_gather]_fwd + stage_layernorm[_gather]_fwd on x.float() (csrc/rowops.hip), and the same
// SCHEDULE of floating-point operations: a row group of LPR lanes owns a row, lane sl owns column quads sl + t*LPR, the row sums
// run lane-first and then through group_sum, the column sums of the backward go per lane -> LDS slots -> per-block partials ->
// stage_colreduce, with the fp32 kernels' grid sizes.  A quad of halves is one 8-byte load (rows are 2*K0 bytes, K0 % 4 == 0: every
// quad is 8-byte aligned; a wave instruction covers 512 contiguous bytes).  16-byte loads would hand a lane two adjacent quads, i.e.
// another lane <-> column assignment and another summation order than the fp32 kernels': the two paths would then differ in the
// last bits on rows with a large dynamic range, and this file's reason to exist is that they do not differ.
//
// Dropout: the counter stream of ln_fwd_fast_kernel -- drop4(seed, r * (K0/4) + quad) with r the COMPACT row, not the gathered one.
// The features need no gradient: the backward gives d gamma / d beta only (deterministic two-stage column reduction, no atomics).
#include "common.h"
#include "../../include/stage_hip.h"

namespace {

constexpr int F16_UR = 4;            // row slots per wave iteration (LN_UR of csrc/rowops.hip)
constexpr int F16_GRID_CAP = 1024;   // GRID_CAP
constexpr int F16_PART_CAP = 512;    // PART_CAP: blocks that emit column partials (bounds the workspace)
constexpr int F16_MAXK = 1024;       // 4 quads per lane x 64 lanes x 4

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// 4 consecutive 16-bit values -> fp32, exactly (fp16 subnormals included: v_cvt_f32_f16 does not flush in the default mode)
template <int DT>
__device__ __forceinline__ float4 cvt4(u32x2 u) {
    if (DT == STAGE_DT_F16)
        return make_float4(h_lo_f32(u[0]), h_hi_f32(u[0]), h_lo_f32(u[1]), h_hi_f32(u[1]));
    return make_float4(__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xFFFF0000u), __uint_as_float(u[1] << 16),
                       __uint_as_float(u[1] & 0xFFFF0000u));
}
// streaming read: each kernel reads a row once
__device__ __forceinline__ u32x2 ldh4s(const unsigned short* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
}

// x / max(||x||, eps) over the NQ quads of a lane (quads past the row already zero); the summation order of l2norm_fwd_kernel
template <int NQ>
__device__ __forceinline__ void l2_rows(float4 (&v)[NQ], int LPR, float eps) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NQ; t++) s += f4hsum(f4mul(v[t], v[t]));
    s = group_sum(s, LPR);
    const float n = fmaxf(sqrtf(s), eps);
#pragma unroll
    for (int t = 0; t < NQ; t++) v[t] = make_float4(v[t].x / n, v[t].y / n, v[t].z / n, v[t].w / n);
}

template <int DT, bool L2, bool DROP, int NQ, bool GATHER>
__global__ __launch_bounds__(256) void feat16_ln_fwd_kernel(const unsigned short* __restrict__ x, const int* __restrict__ gather,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ y, float* __restrict__ mean,
                                                            float* __restrict__ rstd, long rows, int K, float eps, float eps_l2,
                                                            int LPR, uint64_t seed, uint32_t th, float inv_keep) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int RPW = 64 / LPR, sub = lane / LPR, sl = lane % LPR;
    const int K4 = K >> 2;
    const float invK = 1.0f / (float)K;
    int jq[NQ], jc[NQ];
    bool jok[NQ];
    float4 gm[NQ], bt[NQ];
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        jq[t] = sl + t * LPR;
        jok[t] = jq[t] < K4;
        jc[t] = jok[t] ? jq[t] : K4 - 1;            // loads come from clamped addresses, stores are predicated
        gm[t] = ld4(gamma + 4 * jc[t]);
        bt[t] = ld4(beta + 4 * jc[t]);
    }
    const long step = (long)gridDim.x * wpb * RPW * F16_UR;
    for (long base = ((long)blockIdx.x * wpb + wave) * RPW * F16_UR; base < rows; base += step) {
        u32x2 raw[F16_UR][NQ];
        long row[F16_UR];
#pragma unroll
        for (int u = 0; u < F16_UR; u++) {
            row[u] = base + u * RPW + sub;
            const long rc = row[u] < rows ? row[u] : rows - 1;
            const long xr = GATHER ? (long)gather[rc] : rc;
#pragma unroll
            for (int t = 0; t < NQ; t++) raw[u][t] = ldh4s(x + xr * K + 4 * jc[t]);
        }
#pragma unroll
        for (int u = 0; u < F16_UR; u++) {
            const bool ok = row[u] < rows;
            float4 v[NQ];
#pragma unroll
            for (int t = 0; t < NQ; t++) v[t] = jok[t] ? cvt4<DT>(raw[u][t]) : f4zero();
            if (L2) l2_rows<NQ>(v, LPR, eps_l2);
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < NQ; t++) s += f4hsum(v[t]);
            s = group_sum(s, LPR);
            const float mu = s * invK;
            float q = 0.f;
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                const float4 d = make_float4(v[t].x - mu, v[t].y - mu, v[t].z - mu, v[t].w - mu);
                if (jok[t]) q += f4hsum(f4mul(d, d));
            }
            q = group_sum(q, LPR);
            const float rs = 1.0f / sqrtf(q * invK + eps);
            if (ok && sl == 0) {
                mean[row[u]] = mu;
                rstd[row[u]] = rs;
            }
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                float4 o;
                o.x = (v[t].x - mu) * rs * gm[t].x + bt[t].x;
                o.y = (v[t].y - mu) * rs * gm[t].y + bt[t].y;
                o.z = (v[t].z - mu) * rs * gm[t].z + bt[t].z;
                o.w = (v[t].w - mu) * rs * gm[t].w + bt[t].w;
                if (DROP) o = f4mul(o, drop4(seed, (uint64_t)row[u] * K4 + jq[t], th, inv_keep));
                if (ok && jok[t]) st4(y + row[u] * K + 4 * jq[t], o);
            }
        }
    }
}

// part layout: [gridDim.x][2][K] (0: d gamma, 1: d beta), reduced by stage_colreduce -- as ln_bwd_fast_kernel without the dx half
template <int DT, bool L2, bool DROP, int NQ, bool GATHER>
__global__ __launch_bounds__(256) void feat16_ln_bwd_kernel(const float* __restrict__ dy, const unsigned short* __restrict__ x,
                                                            const int* __restrict__ gather, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, float* __restrict__ part, long rows,
                                                            int K, float eps_l2, int LPR, uint64_t seed, uint32_t th,
                                                            float inv_keep) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [wpb*RPW][2][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int RPW = 64 / LPR, sub = lane / LPR, sl = lane % LPR;
    const int K4 = K >> 2;
    int jq[NQ], jc[NQ];
    bool jok[NQ];
    float4 ag[NQ], ab[NQ];
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        jq[t] = sl + t * LPR;
        jok[t] = jq[t] < K4;
        jc[t] = jok[t] ? jq[t] : K4 - 1;
        ag[t] = ab[t] = f4zero();
    }
    const long step = (long)gridDim.x * wpb * RPW * F16_UR;
    for (long base = ((long)blockIdx.x * wpb + wave) * RPW * F16_UR; base < rows; base += step) {
        u32x2 raw[F16_UR][NQ];
        float4 d[F16_UR][NQ];
        float mu[F16_UR], rs[F16_UR];
        long row[F16_UR];
#pragma unroll
        for (int u = 0; u < F16_UR; u++) {
            row[u] = base + u * RPW + sub;
            const long rc = row[u] < rows ? row[u] : rows - 1;
            mu[u] = mean[rc];
            rs[u] = rstd[rc];
            const long xr = GATHER ? (long)gather[rc] : rc;
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                raw[u][t] = ldh4s(x + xr * K + 4 * jc[t]);
                d[u][t] = ld4s(dy + rc * K + 4 * jc[t]);
            }
        }
#pragma unroll
        for (int u = 0; u < F16_UR; u++) {
            const bool ok = row[u] < rows;
            float4 v[NQ];
#pragma unroll
            for (int t = 0; t < NQ; t++) v[t] = jok[t] ? cvt4<DT>(raw[u][t]) : f4zero();
            if (L2) l2_rows<NQ>(v, LPR, eps_l2);
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                float4 dd = d[u][t];
                if (DROP) dd = f4mul(dd, drop4(seed, (uint64_t)row[u] * K4 + jq[t], th, inv_keep));
                if (!ok || !jok[t]) dd = f4zero();   // rows / quads past the end were read from a clamped address
                const float4 xh = make_float4((v[t].x - mu[u]) * rs[u], (v[t].y - mu[u]) * rs[u], (v[t].z - mu[u]) * rs[u],
                                              (v[t].w - mu[u]) * rs[u]);
                ag[t] = f4add(ag[t], f4mul(dd, xh));
                ab[t] = f4add(ab[t], dd);
            }
        }
    }
    // block reduction of the per-lane column partials (slot layout and order of the fp32 kernels)
    const int slot = wave * RPW + sub;
    float* sg = smem + (size_t)slot * 2 * K;
#pragma unroll
    for (int t = 0; t < NQ; t++)
        if (jok[t]) {
            st4(sg + 4 * jq[t], ag[t]);
            st4(sg + K + 4 * jq[t], ab[t]);
        }
    __syncthreads();
    const int nslots = wpb * RPW;
    for (int c = threadIdx.x; c < 2 * K; c += blockDim.x) {
        float acc = 0.f;
        for (int s = 0; s < nslots; s++) acc += smem[(size_t)s * 2 * K + c];
        part[(size_t)blockIdx.x * 2 * K + c] = acc;
    }
}

int f16_lpr(int K4) {
    int l = stage_pow2_ceil(K4);
    if (l < 4) l = 4;
    if (l > 64) l = 64;
    return l;
}

struct DropArgs { uint64_t seed; uint32_t th; float inv_keep; };
DropArgs drop_args(float p, unsigned long long seed) {
    if (p > 0.f) return {(uint64_t)seed, drop_thresh16(p), 1.0f / (1.0f - p)};
    return {0, 0u, 1.0f};
}

template <int DT, bool L2, bool DROP, bool GATHER>
void fwd_launch(int nq, int grid, hipStream_t st, const unsigned short* x, const int* gather, const float* gamma, const float* beta,
                float* y, float* mean, float* rstd, long rows, int K, float eps, float eps_l2, int LPR, DropArgs da) {
#define F16_FWD(NQV)                                                                                                                 \
    hipLaunchKernelGGL((feat16_ln_fwd_kernel<DT, L2, DROP, NQV, GATHER>), dim3(grid), dim3(256), 0, st, x, gather, gamma, beta, y, mean, \
                       rstd, rows, K, eps, eps_l2, LPR, da.seed, da.th, da.inv_keep)
    switch (nq) {
        case 1: F16_FWD(1); break;
        case 2: F16_FWD(2); break;
        case 3: F16_FWD(3); break;
        default: F16_FWD(4); break;
    }
#undef F16_FWD
}
template <int DT, bool L2, bool DROP, bool GATHER>
void bwd_launch(int nq, int grid, size_t lds, hipStream_t st, const float* dy, const unsigned short* x, const int* gather,
                const float* mean, const float* rstd, float* part, long rows, int K, float eps_l2, int LPR, DropArgs da) {
#define F16_BWD(NQV)                                                                                                                 \
    hipLaunchKernelGGL((feat16_ln_bwd_kernel<DT, L2, DROP, NQV, GATHER>), dim3(grid), dim3(256), lds, st, dy, x, gather, mean, rstd, part, \
                       rows, K, eps_l2, LPR, da.seed, da.th, da.inv_keep)
    switch (nq) {
        case 1: F16_BWD(1); break;
        case 2: F16_BWD(2); break;
        case 3: F16_BWD(3); break;
        default: F16_BWD(4); break;
    }
#undef F16_BWD
}

// the three run-time switches of a launch -> template arguments
#define F16_DISPATCH(FN, l2, dr, ga, ...)                                                        \
    do {                                                                                         \
        if (l2) { if (dr) { if (ga) FN<DT, true, true, true>(__VA_ARGS__); else FN<DT, true, true, false>(__VA_ARGS__); }      \
                  else    { if (ga) FN<DT, true, false, true>(__VA_ARGS__); else FN<DT, true, false, false>(__VA_ARGS__); } }  \
        else    { if (dr) { if (ga) FN<DT, false, true, true>(__VA_ARGS__); else FN<DT, false, true, false>(__VA_ARGS__); }    \
                  else    { if (ga) FN<DT, false, false, true>(__VA_ARGS__); else FN<DT, false, false, false>(__VA_ARGS__); } } \
    } while (0)

template <int DT>
void fwd_dispatch(bool l2, bool dr, bool ga, int nq, int grid, hipStream_t st, const unsigned short* x, const int* gather,
                  const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int K, float eps, float eps_l2,
                  int LPR, DropArgs da) {
    F16_DISPATCH(fwd_launch, l2, dr, ga, nq, grid, st, x, gather, gamma, beta, y, mean, rstd, rows, K, eps, eps_l2, LPR, da);
}
template <int DT>
void bwd_dispatch(bool l2, bool dr, bool ga, int nq, int grid, size_t lds, hipStream_t st, const float* dy, const unsigned short* x,
                  const int* gather, const float* mean, const float* rstd, float* part, long rows, int K, float eps_l2, int LPR,
                  DropArgs da) {
    F16_DISPATCH(bwd_launch, l2, dr, ga, nq, grid, lds, st, dy, x, gather, mean, rstd, part, rows, K, eps_l2, LPR, da);
}
#undef F16_DISPATCH

// everything a launch relies on, checked on the host: widths, the 8-byte loads' alignment, 32-bit row arithmetic of the grid
bool args_ok(const void* x, int dtype, long long rows, int K0) {
    return stage_feat16_supported(K0, dtype) && x && ((uintptr_t)x & 7) == 0 && rows < (1ll << 31);
}

}  // namespace

extern "C" int stage_feat16_supported(int K0, int dtype) {
    return (dtype == STAGE_DT_F16 || dtype == STAGE_DT_BF16) && K0 >= 4 && K0 % 4 == 0 && K0 <= F16_MAXK;
}

extern "C" size_t stage_feat16_ln_bwd_ws_bytes(int K0) { return (size_t)F16_PART_CAP * 2 * (size_t)(K0 > 0 ? K0 : 0) * sizeof(float); }

extern "C" int stage_feat16_ln_fwd(const void* x, int dtype, const int* src_rows, const float* gamma, const float* beta, float* y0,
                                   float* mean0, float* rstd0, long long rows, int K0, int l2, float eps_ln, float eps_l2,
                                   float p_drop, unsigned long long seed, void* stream) {
    if (!args_ok(x, dtype, rows, K0) || !gamma || !beta || !y0 || !mean0 || !rstd0) return STAGE_ERR_SHAPE;
    if (rows <= 0) return 0;
    const int LPR = f16_lpr(K0 / 4), nq = (K0 / 4 + LPR - 1) / LPR;
    const int grid = stage_grid_for(rows, 4 * (64 / LPR) * F16_UR, F16_GRID_CAP * 2);
    const DropArgs da = drop_args(p_drop, seed);
    const unsigned short* xs = (const unsigned short*)x;
    if (dtype == STAGE_DT_F16)
        fwd_dispatch<STAGE_DT_F16>(l2 != 0, p_drop > 0.f, src_rows != nullptr, nq, grid, (hipStream_t)stream, xs, src_rows, gamma, beta, y0,
                                   mean0, rstd0, (long)rows, K0, eps_ln, eps_l2, LPR, da);
    else
        fwd_dispatch<STAGE_DT_BF16>(l2 != 0, p_drop > 0.f, src_rows != nullptr, nq, grid, (hipStream_t)stream, xs, src_rows, gamma, beta, y0,
                                    mean0, rstd0, (long)rows, K0, eps_ln, eps_l2, LPR, da);
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_feat16_ln_bwd(const float* dy0, const void* x, int dtype, const int* src_rows, const float* mean0,
                                   const float* rstd0, float* dgamma, float* dbeta, long long rows, int K0, int l2, float eps_l2,
                                   float p_drop, unsigned long long seed, void* ws, size_t ws_bytes, void* stream) {
    if (!args_ok(x, dtype, rows, K0) || !dgamma || !dbeta) return STAGE_ERR_SHAPE;
    if (!ws || ws_bytes < stage_feat16_ln_bwd_ws_bytes(K0)) return STAGE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (rows <= 0) {
        (void)hipMemsetAsync(dgamma, 0, sizeof(float) * K0, st);
        (void)hipMemsetAsync(dbeta, 0, sizeof(float) * K0, st);
        return 0;
    }
    if (!dy0 || !mean0 || !rstd0) return STAGE_ERR_SHAPE;
    const int LPR = f16_lpr(K0 / 4), nq = (K0 / 4 + LPR - 1) / LPR;
    const int rows_per_block = 4 * (64 / LPR);
    const int grid = stage_grid_for(rows, rows_per_block * 8, F16_PART_CAP);
    const size_t lds = (size_t)rows_per_block * 2 * K0 * sizeof(float);
    const DropArgs da = drop_args(p_drop, seed);
    const unsigned short* xs = (const unsigned short*)x;
    float* part = (float*)ws;
    if (dtype == STAGE_DT_F16)
        bwd_dispatch<STAGE_DT_F16>(l2 != 0, p_drop > 0.f, src_rows != nullptr, nq, grid, lds, st, dy0, xs, src_rows, mean0, rstd0, part,
                                   (long)rows, K0, eps_l2, LPR, da);
    else
        bwd_dispatch<STAGE_DT_BF16>(l2 != 0, p_drop > 0.f, src_rows != nullptr, nq, grid, lds, st, dy0, xs, src_rows, mean0, rstd0, part,
                                    (long)rows, K0, eps_l2, LPR, da);
    STAGE_LAUNCH_CHECK();
    // column c = t*K0 + d of the [2][K0] partial rows goes to dgamma[d] (t = 0) or dbeta[d] (t = 1)
    stage_colreduce(part, dgamma, dbeta, grid, (long)2 * K0, 2 * K0, K0, 1, st);
    STAGE_LAUNCH_CHECK();
    return 0;
}
