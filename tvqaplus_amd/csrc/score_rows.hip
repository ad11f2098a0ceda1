// Consumers of selected rows of the attention map vid_raw_s (N, NA, Li, Lqa, Lr), Lr <= 64: box prediction for inference
// (model/stage.py:748-806) and the rank order of a row's labelled negatives for hard-negative sampling (model/stage.py:557-611).
// Both rank the Lr scores of K selected rows: one wavefront per row (lane r holds region r), four rows per 256-thread workgroup.
// Latency class (last row): K is a few hundred to a few thousand rows of at most 256 bytes.
//
// Memory safety: a row is read only when 0 <= row_off[k] and row_off[k] + Lr <= n_scores; otherwise nothing is read and a sentinel
// is written (cnt = -1 / flat_neg = -1).  The same holds for a pair slot whose rank position is not below the row's negative count.
#include "common.h"
#include "../../include/stage_hip.h"

namespace {
constexpr int ROWS_PER_WG = 4;

// Rank of this lane among the lanes of `mask` (wave-uniform): the number of lanes j in `mask` that come before it.  DESC: higher
// score first, else lower score first; equal scores (+0 == -0): lower lane first.  A NaN comes after every number, NaNs among
// themselves by lane: "before" is a strict total order, so the ranks of the mask's lanes are a permutation of 0 .. popcount - 1.
template <bool DESC>
__device__ __forceinline__ int rank_in_wave(float s, int lane, unsigned long long mask) {
    int rank = 0;
    const bool i_nan = s != s;
    while (mask) {
        const int j = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float sj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(s), __builtin_amdgcn_readfirstlane(j)));
        const bool j_nan = sj != sj;
        const bool first = DESC ? sj > s : sj < s;
        const bool tie = sj == s || (i_nan && j_nan);
        rank += (first || (i_nan && !j_nan) || (tie && j < lane)) ? 1 : 0;
    }
    return rank;
}

__device__ __forceinline__ bool row_in_range(long long off, int Lr, long long n_scores) {
    return off >= 0 && off <= n_scores - (long long)Lr;
}

// cnt (K), val (K, Lr), idx (K, Lr): the regions of row k with score >= thd in ascending score order, the rest filled (0 / -1)
__global__ __launch_bounds__(64 * ROWS_PER_WG) void att_predict_kernel(const float* __restrict__ scores,
                                                                        const long long* __restrict__ row_off, int K, int Lr,
                                                                        long long n_scores, float thd, int* __restrict__ cnt,
                                                                        float* __restrict__ val, int* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (k >= K) return;                                   // wave-uniform; no barrier in this kernel
    const long long off = row_off[k];
    const bool ok = row_in_range(off, Lr, n_scores);
    const bool in_row = lane < Lr;
    const float s = (ok && in_row) ? scores[off + lane] : 0.f;
    const bool take = ok && in_row && s >= thd;
    const unsigned long long mask = __ballot(take);
    const int n = __popcll(mask);
    const int rank = rank_in_wave<false>(s, lane, mask);
    const long base = (long)k * Lr;
    if (take) {
        val[base + rank] = s;
        idx[base + rank] = lane;
    }
    if (in_row && lane >= n) {
        val[base + lane] = 0.f;
        idx[base + lane] = -1;
    }
    if (lane == 0) cnt[k] = ok ? n : -1;
}

// flat_neg[m] = row_off[k] + (the region at position slot_q[m] of row k's labelled negatives in descending score order) for the
// slots m in [slot_begin[k], slot_begin[k + 1])
__global__ __launch_bounds__(64 * ROWS_PER_WG) void att_hard_neg_kernel(const float* __restrict__ scores,
                                                                         const long long* __restrict__ row_off,
                                                                         const unsigned long long* __restrict__ negbits,
                                                                         const int* __restrict__ slot_begin,
                                                                         const int* __restrict__ slot_q, int K, int M, int Lr,
                                                                         long long n_scores, long long* __restrict__ flat_neg) {
    __shared__ int order[ROWS_PER_WG][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * ROWS_PER_WG + w;
    const bool live = k < K;                              // (no early return: the barrier below is for the whole workgroup)
    long long off = 0;
    bool ok = false;
    unsigned long long neg = 0;
    int sb = 0, se = 0;
    if (live) {
        off = row_off[k];
        ok = row_in_range(off, Lr, n_scores);
        neg = negbits[k] & (Lr >= 64 ? ~0ull : ((1ull << Lr) - 1ull));
        sb = min(max(slot_begin[k], 0), M);
        se = min(max(slot_begin[k + 1], sb), M);
    }
    if (!ok) neg = 0;
    const bool mine = (neg >> lane) & 1ull;
    const float s = mine ? scores[off + lane] : 0.f;
    order[w][lane] = -1;
    const int rank = rank_in_wave<true>(s, lane, neg);
    __syncthreads();
    if (mine) order[w][rank] = lane;
    __syncthreads();
    const int n = __popcll(neg);
    for (int m = sb + lane; m < se; m += 64) {
        const int q = slot_q[m];
        const int r = (q >= 0 && q < n) ? order[w][q] : -1;
        flat_neg[m] = r >= 0 ? off + r : -1ll;
    }
}
}  // namespace

extern "C" int stage_score_rows_supported(int Lr) { return Lr >= 1 && Lr <= 64 ? 1 : 0; }

extern "C" int stage_att_predict(const float* scores, const long long* row_off, int K, int Lr, long long n_scores, float thd, int* cnt,
                                 float* val, int* idx, void* st) {
    if (!stage_score_rows_supported(Lr) || K < 0 || n_scores < 0) return STAGE_ERR_SHAPE;
    if (K == 0) return 0;
    hipLaunchKernelGGL(att_predict_kernel, dim3((K + ROWS_PER_WG - 1) / ROWS_PER_WG), dim3(64 * ROWS_PER_WG), 0, (hipStream_t)st,
                       scores, row_off, K, Lr, n_scores, thd, cnt, val, idx);
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_att_hard_negatives(const float* scores, const long long* row_off, const unsigned long long* negbits,
                                        const int* slot_begin, const int* slot_q, int K, int M, int Lr, long long n_scores,
                                        long long* flat_neg, void* st) {
    if (!stage_score_rows_supported(Lr) || K < 0 || M < 0 || n_scores < 0) return STAGE_ERR_SHAPE;
    if (K == 0 || M == 0) return 0;
    hipLaunchKernelGGL(att_hard_neg_kernel, dim3((K + ROWS_PER_WG - 1) / ROWS_PER_WG), dim3(64 * ROWS_PER_WG), 0, (hipStream_t)st,
                       scores, row_off, negbits, slot_begin, slot_q, K, M, Lr, n_scores, flat_neg);
    STAGE_LAUNCH_CHECK();
    return 0;
}
