// Grounding meter (include/stage_hip.h "Grounding meter"): the detection records of eval/eval_tvqa_plus.py's grounding mAP
// (eval/maskrcnn_voc/voc_eval.py through tvqaplus_amd/evaluation.py: load_predictions + detection_map's inner loop), produced next
// to the attention map vid_raw_s (N, NA, Li, Lqa, Lr) and appended to ONE caller-owned device buffer -- nothing is read back until
// the caller copies the buffer.  A task is one (example, annotated image, label) triple; what leaves the kernel per detection is
// (label, score, matched or not); the AP itself is a host-side sort over those (evaluation.average_precision).
//
// Latency class (last row): one wavefront = one 64-thread workgroup per task, a few hundred tasks per batch.
//   lane w:  the word of the answer's statement at position w     -> ballot of the positions that hold the label
//   lane r:  the score of region r of each such row               -> ballot of the regions with score >= thd (fp32; a NaN is not kept)
//   lane c:  candidate c (c, c + 64, ...) of the task's list      -> its IoU row over the ground-truth boxes, its rank by score
//   lane 0:  the greedy matching in rank order (every ground-truth box is taken once)
//   lane 0:  ONE atomic add on the cursor reserves the task's records; they are written by plain vector stores, one lane each
//
// Memory safety: every offset of the task table is checked against the size of the table it points into BEFORE the first read
// through it (words: n_words, score rows: n_scores, region boxes: n_region_boxes, ground-truth boxes: n_gt_boxes); a kept region
// whose index is not below the image's box count is never used as an index.  Such a task is counted in `bad` and writes nothing.
// LDS lists are sized for the limits (8 positions x 64 regions, 32 ground-truth boxes); a task beyond them is counted in `overflow`
// before anything is stored.  Records are written only at slots in [0, capacity).
#include "common.h"
#include "../../include/stage_hip.h"

// The IoU decides a threshold: every product and sum below must round as numpy's float32 does, one operation at a time.
#pragma clang fp contract(off)

#define GROUND_COUNTERS 8      // 64-bit words in front of the records (6 used)
#define GC_CURSOR 0
#define GC_DROPPED 1
#define GC_TASKS 2
#define GC_DETECTIONS 3
#define GC_OVERFLOW 4
#define GC_BAD 5
#define GROUND_HEAD_BYTES (GROUND_COUNTERS * 8)
#define GROUND_TASK_WORDS 8
#define GROUND_MAX_L 64        // Lqa, Lr: one lane each
#define GROUND_MAX_WORDS 8     // positions of the statement that hold the label
#define GROUND_MAX_GT 32       // ground-truth boxes of a task (the `taken` bits of the greedy pass)
#define GROUND_MAX_DET (GROUND_MAX_WORDS * GROUND_MAX_L)

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ void count(u64* head, int which, u64 v) { atomicAdd(head + which, v); }

// a block of `n` >= 0 items starting at `first` lies inside a table of `size` items
__device__ __forceinline__ bool block_in_table(long long first, long long n, long long size) {
    return first >= 0 && n >= 0 && first <= size && n <= size - first;
}

__global__ __launch_bounds__(64) void grounding_kernel(u64* __restrict__ head, uint2* __restrict__ rec, long long capacity,
                                                       const float* __restrict__ scores, long long n_scores,
                                                       const long long* __restrict__ words, long long n_words,
                                                       const long long* __restrict__ tasks, int T,
                                                       const float* __restrict__ region_boxes, long long n_region_boxes,
                                                       const float* __restrict__ gt_boxes, long long n_gt_boxes, int Lqa, int Lr,
                                                       float thd, float iou_thd) {
    __shared__ float s_score[GROUND_MAX_DET];             // candidate c: its score, in (word position, region) order
    __shared__ unsigned short s_reg[GROUND_MAX_DET];      //              its region
    __shared__ unsigned short s_order[GROUND_MAX_DET];    // rank k -> candidate
    __shared__ signed char s_who[GROUND_MAX_DET];         // candidate -> the ground-truth box it may take, or -1
    __shared__ unsigned char s_match[GROUND_MAX_DET];
    __shared__ float s_gt[GROUND_MAX_GT * 4];
    __shared__ long long s_base;
    const int lane = threadIdx.x;
    const int t = blockIdx.x;
    if (t >= T) return;                                   // (block-uniform, like every return below)
    const long long* tk = tasks + (long long)t * GROUND_TASK_WORDS;
    const long long word_off = tk[0], score_off = tk[1], label = tk[2], box_first = tk[3], n_boxes = tk[4], gt_first = tk[5],
                    n_gt = tk[6];
    if (lane == 0) count(head, GC_TASKS, 1);
    // 1. the table row itself
    const bool table_ok = label >= 0 && label <= 0x7fffffffll && block_in_table(word_off, Lqa, n_words) &&
                          block_in_table(score_off, Lr, n_scores) && block_in_table(box_first, n_boxes, n_region_boxes) &&
                          n_gt >= 1 && block_in_table(gt_first, n_gt, n_gt_boxes);
    if (!table_ok) {
        if (lane == 0) count(head, GC_BAD, 1);
        return;
    }
    // 2. the positions of the statement that hold the label
    const long long wd = lane < Lqa ? words[word_off + lane] : -1ll;
    u64 wmask = __ballot(lane < Lqa && wd == label);
    if (__popcll(wmask) > GROUND_MAX_WORDS || n_gt > GROUND_MAX_GT) {
        if (lane == 0) count(head, GC_OVERFLOW, 1);
        return;
    }
    // 3. the kept regions of those rows, in (position, region) order
    int n_det = 0;
    bool rows_ok = true;
    while (wmask) {
        const int w = __builtin_ctzll(wmask);
        wmask &= wmask - 1;
        const long long off = score_off + (long long)w * Lr;
        if (!block_in_table(off, Lr, n_scores)) {
            rows_ok = false;
            break;
        }
        const float s = lane < Lr ? scores[off + lane] : 0.f;
        const bool take = lane < Lr && s >= thd;
        if (__ballot(take && lane >= n_boxes)) {          // a kept region without a box
            rows_ok = false;
            break;
        }
        const u64 m = __ballot(take);
        if (take) {
            const int c = n_det + __popcll(m & ((1ull << lane) - 1ull));
            s_score[c] = s;
            s_reg[c] = (unsigned short)lane;
        }
        n_det += __popcll(m);
    }
    if (!rows_ok) {
        if (lane == 0) count(head, GC_BAD, 1);
        return;
    }
    if (n_det == 0) return;
    for (int i = lane; i < (int)n_gt * 4; i += 64) s_gt[i] = gt_boxes[gt_first * 4 + i];
    __syncthreads();
    // 4. per candidate: the first ground-truth box with the largest IoU (numpy's argmax: a NaN counts as the largest), kept when
    //    that IoU is not below the threshold.  evaluation._pairwise_iou on boxes whose far edges were incremented, operation for operation.
    for (int c = lane; c < n_det; c += 64) {
        const float* pb = region_boxes + (box_first + s_reg[c]) * 4;
        const float a0 = pb[0], a1 = pb[1], a2 = pb[2] + 1.f, a3 = pb[3] + 1.f;
        const float area_a = (a2 - a0 + 1.f) * (a3 - a1 + 1.f);
        float best = 0.f;
        int who = 0;
        for (int j = 0; j < (int)n_gt; j++) {
            const float b0 = s_gt[4 * j], b1 = s_gt[4 * j + 1], b2 = s_gt[4 * j + 2] + 1.f, b3 = s_gt[4 * j + 3] + 1.f;
            const float area_b = (b2 - b0 + 1.f) * (b3 - b1 + 1.f);
            const float w0 = fmaxf(fminf(a2, b2) - fmaxf(a0, b0) + 1.f, 0.f);
            const float w1 = fmaxf(fminf(a3, b3) - fmaxf(a1, b1) + 1.f, 0.f);
            const float inter = w0 * w1;
            const float v = inter / ((area_a + area_b) - inter);
            if (j == 0 || v > best || (v != v && best == best)) {
                best = v;
                who = j;
            }
        }
        s_who[c] = (signed char)(best < iou_thd ? -1 : who);
    }
    // 5. rank by descending score; equal scores: the lower (position, region) first
    for (int c = lane; c < n_det; c += 64) {
        const float s = s_score[c];
        int rank = 0;
        for (int o = 0; o < n_det; o++) {
            const float so = s_score[o];
            rank += (so > s || (so == s && o < c)) ? 1 : 0;
        }
        s_order[rank] = (unsigned short)c;
    }
    __syncthreads();
    // 6. greedy matching in rank order, and the reservation
    if (lane == 0) {
        unsigned int taken = 0u;
        for (int k = 0; k < n_det; k++) {
            const int c = s_order[k];
            const int j = s_who[c];
            unsigned char mt = 0;
            if (j >= 0) {
                mt = ((taken >> j) & 1u) ? 0 : 1;
                taken |= 1u << j;
            }
            s_match[c] = mt;
        }
        const long long base = (long long)atomicAdd(head + GC_CURSOR, (u64)n_det);
        count(head, GC_DETECTIONS, (u64)n_det);
        const long long room = base >= capacity ? 0 : (capacity - base < n_det ? capacity - base : n_det);
        if (room < n_det) count(head, GC_DROPPED, (u64)(n_det - room));
        s_base = base;
    }
    __syncthreads();
    const long long base = s_base;
    for (int c = lane; c < n_det; c += 64) {
        const long long slot = base + c;
        if (slot >= 0 && slot < capacity)
            rec[slot] = make_uint2((unsigned int)label | (s_match[c] ? 0x80000000u : 0u), __float_as_uint(s_score[c]));
    }
}

inline bool grounding_ok(const void* buf, long long capacity) { return buf != nullptr && capacity >= 0 && ((uintptr_t)buf & 7) == 0; }

}  // namespace

extern "C" int stage_grounding_supported(int Lqa, int Lr) {
    return Lqa >= 1 && Lqa <= GROUND_MAX_L && Lr >= 1 && Lr <= GROUND_MAX_L ? 1 : 0;
}

extern "C" size_t stage_grounding_bytes(long long capacity) {
    if (capacity < 0) return 0;
    return (size_t)GROUND_HEAD_BYTES + (size_t)capacity * 8;
}

extern "C" int stage_grounding_reset(void* buf, long long capacity, void* st) {
    if (!grounding_ok(buf, capacity)) return STAGE_ERR_SHAPE;
    const hipError_t e = hipMemsetAsync(buf, 0, stage_grounding_bytes(capacity), (hipStream_t)st);
    return e == hipSuccess ? 0 : (int)e;
}

extern "C" int stage_grounding_update(void* buf, long long capacity, const float* scores, long long n_scores, const long long* words,
                                      long long n_words, const long long* tasks, int T, const float* region_boxes,
                                      long long n_region_boxes, const float* gt_boxes, long long n_gt_boxes, int Lqa, int Lr, float thd,
                                      float iou_thd, void* st) {
    if (!grounding_ok(buf, capacity) || !stage_grounding_supported(Lqa, Lr)) return STAGE_ERR_SHAPE;
    if (T < 0 || n_scores < 0 || n_words < 0 || n_region_boxes < 0 || n_gt_boxes < 0) return STAGE_ERR_SHAPE;
    if (T == 0) return 0;
    if (!scores || !words || !tasks || ((uintptr_t)tasks & 7) || ((uintptr_t)words & 7)) return STAGE_ERR_SHAPE;
    if ((n_region_boxes > 0 && !region_boxes) || (n_gt_boxes > 0 && !gt_boxes)) return STAGE_ERR_SHAPE;
    u64* head = reinterpret_cast<u64*>(buf);
    hipLaunchKernelGGL(grounding_kernel, dim3(T), dim3(64), 0, (hipStream_t)st, head,
                       reinterpret_cast<uint2*>(reinterpret_cast<char*>(buf) + GROUND_HEAD_BYTES), capacity, scores, n_scores, words,
                       n_words, tasks, T, region_boxes, n_region_boxes, gt_boxes, n_gt_boxes, Lqa, Lr, thd, iou_thd);
    STAGE_LAUNCH_CHECK();
    return 0;
}
