// Packed context features (include/stage_hip.h "Packed context features", tvqaplus_amd/packed.py).
//
// The reference's collate (tvqa_dataset.py:515-553) zero-fills a padded (N, Li, L, K) tensor, copies the len(f) rows of every frame f
// into it and builds prefix masks from the lengths: everything behind a frame's length is zero by construction.  A packed stream is
// the rows that exist, frame-major, plus ONE zero row at the end (row P):
//   ptab (frames, 2) int32   (first packed row, len) of every frame
// Two things are built from it on the device:
//   * the source-row table of a ragged context layout (tvqaplus_amd/ragged.py: CtxLayout) pointing INTO the packed buffer -- compact row
//     l of frame f reads packed row ptab[f].x + l, or the zero row when l >= len (the halo of the input encoder's convolutions);
//   * the padded image (and / or the prefix mask) for the paths that keep dense (frames, L, .) tensors.
#include "common.h"
#include "../../include/stage_hip.h"

#include <stdint.h>

namespace {

constexpr int PACK_THREADS = 256;
constexpr int PACK_WAVES = PACK_THREADS / 64;
constexpr int PACK_MAX_BLOCKS = 2048;      // 8 workgroups = 32 waves per CU on 256 CUs; more rows: grid-stride

// as rag_ctx_rows_kernel (csrc/ragged.hip) with the rows behind len redirected to the zero row
__global__ __launch_bounds__(256) void pack_ctx_rows_kernel(const int2* __restrict__ cq, const int2* __restrict__ ptab, long frames, int L,
                                                            int zero_row, int* __restrict__ src) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long f = t / L;
    const int l = (int)(t - f * L);
    if (f >= frames) return;
    const int2 q = cq[f];
    if (l >= q.y) return;
    const int2 p = ptab[f];
    src[(long)q.x + l] = l < p.y ? p.x + l : zero_row;
}

__global__ __launch_bounds__(256) void pack_mask_kernel(const int2* __restrict__ ptab, long rows, int L, float* __restrict__ mask) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    const long f = t / L;
    const int l = (int)(t - f * L);
    mask[t] = l < ptab[f].y ? 1.f : 0.f;
}

// One pass over the dense image: every row of it is written, from its packed row or with zeros.  V = uint4 (16-byte rows on 16-byte
// bases) or uint2.  A group of G = 2^LOG_G lanes (the smallest power of two that holds a row's cpr chunks, 64 at most) walks one row:
// consecutive lanes read and write consecutive chunks, and the 64 / G rows of a wave are consecutive rows of the dense image.
template <typename V>
__global__ __launch_bounds__(PACK_THREADS) void pack_unpack_kernel(const V* __restrict__ packed, const int2* __restrict__ ptab,
                                                                   V* __restrict__ dense, float* __restrict__ mask, long rows, int L, int cpr,
                                                                   int log_g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << log_g, rpw = 64 >> log_g;             // lanes per row, rows per wave
    const int k0 = lane & (G - 1), sub = lane >> log_g;
    const long per_block = (long)PACK_WAVES * rpw;
    V zero;
    __builtin_memset(&zero, 0, sizeof(V));
    for (long base = (long)blockIdx.x * per_block; base < rows; base += (long)gridDim.x * per_block) {
        const long row = base + (long)wave * rpw + sub;
        if (row >= rows) continue;
        const long f = row / L;
        const int l = (int)(row - f * L);
        const int2 p = ptab[f];
        const bool live = l < p.y;
        V* dst = dense + row * cpr;
        if (live) {
            const V* src = packed + ((long)p.x + l) * cpr;
#pragma unroll 4
            for (int k = k0; k < cpr; k += G) dst[k] = src[k];
        } else {
#pragma unroll 4
            for (int k = k0; k < cpr; k += G) dst[k] = zero;
        }
        if (mask != nullptr && k0 == 0) mask[row] = live ? 1.f : 0.f;
    }
}

template <typename V>
int launch_unpack(const void* packed, const int* ptab, void* dense, float* mask, long rows, int L, int row_bytes, hipStream_t stream) {
    const int cpr = row_bytes / (int)sizeof(V);
    int log_g = 0;
    while ((1 << log_g) < cpr && log_g < 6) ++log_g;
    const long per_block = (long)PACK_WAVES * (64 >> log_g);
    long blocks = (rows + per_block - 1) / per_block;
    if (blocks > PACK_MAX_BLOCKS) blocks = PACK_MAX_BLOCKS;
    hipLaunchKernelGGL(pack_unpack_kernel<V>, dim3((unsigned)blocks), dim3(PACK_THREADS), 0, stream, (const V*)packed, (const int2*)ptab,
                       (V*)dense, mask, rows, L, cpr, log_g);
    STAGE_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int stage_pack_ctx_rows(const int* cq, const int* ptab, long long frames, int L, int zero_row, int* src_rows, void* stream) {
    if (L < 1 || (frames > 0 && frames * L >= (1ll << 31))) return STAGE_ERR_SHAPE;
    if (frames <= 0) return 0;
    if (!cq || !ptab || !src_rows || zero_row < 0) return STAGE_ERR_SHAPE;
    const long total = (long)frames * L;
    hipLaunchKernelGGL(pack_ctx_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const int2*)cq,
                       (const int2*)ptab, (long)frames, L, zero_row, src_rows);
    STAGE_LAUNCH_CHECK();
    return 0;
}

extern "C" int stage_pack_unpack(const void* packed, const int* ptab, void* dense, float* mask, long long frames, int L, int row_bytes,
                                 void* stream) {
    if (L < 1 || (frames > 0 && frames * L >= (1ll << 31))) return STAGE_ERR_SHAPE;
    const bool mask_only = packed == nullptr && dense == nullptr;
    if (!mask_only) {
        if (row_bytes % 8 || row_bytes < 8 || row_bytes > 4096) return STAGE_ERR_SHAPE;
        if (!packed || !dense || ((uintptr_t)packed & 7) || ((uintptr_t)dense & 7)) return STAGE_ERR_SHAPE;
    } else if (!mask) {
        return STAGE_ERR_SHAPE;
    }
    if (frames <= 0) return 0;
    if (!ptab) return STAGE_ERR_SHAPE;
    const long rows = (long)frames * L;
    hipStream_t st = (hipStream_t)stream;
    if (mask_only) {
        hipLaunchKernelGGL(pack_mask_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, (const int2*)ptab, rows, L, mask);
        STAGE_LAUNCH_CHECK();
        return 0;
    }
    const bool wide = row_bytes % 16 == 0 && !((uintptr_t)packed & 15) && !((uintptr_t)dense & 15);
    return wide ? launch_unpack<uint4>(packed, ptab, dense, mask, rows, L, row_bytes, st)
                : launch_unpack<uint2>(packed, ptab, dense, mask, rows, L, row_bytes, st);
}
