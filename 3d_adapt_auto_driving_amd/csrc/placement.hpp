// placement.hpp -- the skeleton of greedy object placement that csrc/aug_scene.hip and csrc/train_input.hip share: one wave takes an
// ordered list of at most PLACE_MAX_CAND candidates, rejects those that meet a label box, then accepts in try order every
// candidate that meets no earlier accepted one.  The record type (Rec, REC values per box) and the pair rule CONFLICT(new box,
// present box) -> "the pair forbids the placement" are the unit's own: the two units follow different overlap rules.
#pragma once
#include "common.hpp"
#include "gt_common.hpp"

namespace prcnn {

constexpr int PLACE_MAX_CAND = 16;               // candidates per placement (prcnn_aug_max_candidates)

// every candidate (scand, nc records) against the nb label boxes, which stage(k0, kn) puts into sorig in chunks of GT_CHUNK (one
// wave; all pairs of a chunk in parallel) -> the candidates' reject bits
template <class Rec, int REC, bool (*CONFLICT)(const Rec *, const Rec *), class Stage>
__device__ __forceinline__ unsigned place_reject_by_labels(const Rec *scand, int nc, const Rec *sorig, int nb, unsigned *srej, Stage stage)
{
    const int lane = threadIdx.x;
    if (lane == 0) *srej = 0u;
    for (int k0 = 0; k0 < nb; k0 += GT_CHUNK) {
        const int kn = min(GT_CHUNK, nb - k0);
        __syncthreads();
        stage(k0, kn);
        __syncthreads();
        for (int p = lane; p < nc * kn; p += WAVE) {
            const int c = p / kn, k = p - c * kn;
            if (CONFLICT(scand + c * REC, sorig + k * REC)) atomicOr(srej, 1u << c);   // LDS; an OR has no order
        }
    }
    __syncthreads();
    return *srej;
}

// every candidate i (scand) against every earlier one jj (searlier: the same boxes as the unit's rule presents an already placed
// one), then the greedy accept in try order -> slots[0..n) = the accepted candidates, slots[-1] = n, the unused slots -1
template <class Rec, int REC, bool (*CONFLICT)(const Rec *, const Rec *)>
__device__ __forceinline__ void place_accept_greedy(const Rec *scand, const Rec *searlier, int nc, unsigned rej, int *slots)
{
    const int lane = threadIdx.x;
    unsigned conf[PLACE_MAX_CAND];               // row i of an iteration's ballot is candidate i's 16-bit conflict word
#pragma unroll
    for (int it = 0; it < PLACE_MAX_CAND * PLACE_MAX_CAND / WAVE; ++it) {
        const int p = it * WAVE + lane, i = p / PLACE_MAX_CAND, jj = p % PLACE_MAX_CAND;
        bool bad = false;
        if (i < nc && jj < i && !((rej >> i) & 1u) && !((rej >> jj) & 1u)) bad = CONFLICT(scand + i * REC, searlier + jj * REC);
        const unsigned long long m = __ballot(bad);
#pragma unroll
        for (int q = 0; q < WAVE / PLACE_MAX_CAND; ++q)
            conf[it * (WAVE / PLACE_MAX_CAND) + q] = (unsigned)(m >> (PLACE_MAX_CAND * q)) & 0xffffu;
    }
    unsigned acc = 0u;                           // (uniform in the wave)
    int n_acc = 0;
#pragma unroll
    for (int i = 0; i < PLACE_MAX_CAND; ++i) {
        if (i < nc && !((rej >> i) & 1u) && !(conf[i] & acc)) {
            acc |= 1u << i;
            if (lane == 0) slots[n_acc] = i;
            ++n_acc;
        }
    }
    if (lane == 0) {
        slots[-1] = n_acc;
        for (int k = n_acc; k < PLACE_MAX_CAND; ++k) slots[k] = -1;
    }
}

// the accepted boxes of candidate row q0 (slots as place_accept_greedy wrote them), h + 2 -> inside records in lds (all threads of
// the workgroup; a barrier behind) -> their number
__device__ __forceinline__ int stage_accepted(const int *slots, long q0, const float *cand_box, const float *cand_trig, float *lds)
{
    const int na = min(max(slots[-1], 0), PLACE_MAX_CAND);
    if ((int)threadIdx.x < na) {
        const long q = q0 + min(max(slots[threadIdx.x], 0), PLACE_MAX_CAND - 1);
        const float *bx = cand_box + 7L * q;
        gt_box_record(bx, __fadd_rn(bx[3], 2.0f), cand_trig[2 * q], cand_trig[2 * q + 1], lds + threadIdx.x * GT_REC);
    }
    __syncthreads();
    return na;
}

}  // namespace prcnn
