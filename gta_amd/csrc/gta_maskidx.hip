// gta_maskidx.hip -- every mask-derived tensor of a masked attention call in one launch (gta_mask_index).
//
// From a key mask [B, Tk] (one byte per token, non-zero = live):
//   key_idx[b]   the permutation of [0, Tk) with scene b's live tokens first, ascending, then its masked tokens, ascending
//                (a stable sort of the negated mask);
//   key_lens[b]  the number of live tokens, unclamped (0 for a row without one);
//   k_live[b]    the mask as 0 / 1 bytes, with token 0 of a row without a live token set (optional).
// From a query mask [B, Tq]:
//   q_lens[b]    1 + the index of the last live token, 0 for a row without one.
//
//   * one 256-thread workgroup per (scene, side): blockIdx.x = scene, blockIdx.y = side (the key side first when both are given);
//   * the key side walks its row twice in chunks of 256 tokens, one byte per lane (the row is a few KiB: the second walk hits L2).
//     Pass 1 counts the live tokens: a 64-bit wave ballot and its popcount per chunk, the four waves' sums joined through LDS once.
//     Pass 2 places every token: live_before(t) = base + (live tokens of the lower waves of this chunk) + popcount(ballot below the
//     lane), with `base` the live tokens of the chunks before (carried in a register: every wave reads all four wave counts of the
//     chunk).  A live token goes to live_before(t), a masked one to count + t - live_before(t).  The wave counts are double-buffered
//     in LDS, so a chunk costs one barrier;
//   * the query side is one walk: the highest set bit of each chunk's ballot, the four waves' maxima joined through LDS;
//   * every output element has exactly one writer: no atomics, no workspace, nothing read back by the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gta_common.h"
#include "../../include/gta_hip.h"

namespace {

constexpr int MASKIDX_CHUNK = 256;      // tokens per trip of the row loops = threads per workgroup

__global__ __launch_bounds__(256) void gta_mask_index_kernel(const uint8_t* __restrict__ key_mask, int Tk, int32_t* __restrict__ key_idx,
                                                             int32_t* __restrict__ key_lens, uint8_t* __restrict__ k_live,
                                                             const uint8_t* __restrict__ query_mask, int Tq, int32_t* __restrict__ q_lens) {
    __shared__ int s_wave[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool key_side = key_mask && blockIdx.y == 0;

    if (!key_side) {
        const uint8_t* row = query_mask + (long)b * Tq;
        int last = 0;                                                // 1 + the highest live index this wave has seen
        for (int t0 = 0; t0 < Tq; t0 += MASKIDX_CHUNK) {
            const int t = t0 + tid;
            const bool live = t < Tq && row[t] != 0;
            const unsigned long long bal = __ballot(live);
            if (bal) last = t0 + wave * 64 + 64 - __builtin_clzll(bal);
        }
        if (lane == 0) s_wave[0][wave] = last;
        __syncthreads();
        if (tid == 0) q_lens[b] = max(max(s_wave[0][0], s_wave[0][1]), max(s_wave[0][2], s_wave[0][3]));
        return;
    }

    const uint8_t* row = key_mask + (long)b * Tk;
    // pass 1: the number of live tokens
    int mine = 0;
    for (int t0 = 0; t0 < Tk; t0 += MASKIDX_CHUNK) {
        const int t = t0 + tid;
        const bool live = t < Tk && row[t] != 0;
        mine += __builtin_popcountll(__ballot(live));
    }
    if (lane == 0) s_wave[1][wave] = mine;
    __syncthreads();
    const int count = s_wave[1][0] + s_wave[1][1] + s_wave[1][2] + s_wave[1][3];
    if (tid == 0) key_lens[b] = count;

    // pass 2: every token to its place (the first chunk writes s_wave[0], the sums above were read from s_wave[1]: after the chunk's
    // barrier nobody reads the buffer the next chunk writes)
    int32_t* idx = key_idx + (long)b * Tk;
    uint8_t* kl = k_live ? k_live + (long)b * Tk : nullptr;
    int base = 0;
    for (int t0 = 0, buf = 0; t0 < Tk; t0 += MASKIDX_CHUNK, buf ^= 1) {
        const int t = t0 + tid;
        const bool in = t < Tk;
        const bool live = in && row[t] != 0;
        const unsigned long long bal = __ballot(live);
        if (lane == 0) s_wave[buf][wave] = __builtin_popcountll(bal);
        __syncthreads();
        const int w0 = s_wave[buf][0], w1 = s_wave[buf][1], w2 = s_wave[buf][2], w3 = s_wave[buf][3];
        const int below = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
        const int before = base + below + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        if (in) {
            idx[live ? before : count + t - before] = t;
            if (kl) kl[t] = (live || (count == 0 && t == 0)) ? 1 : 0;
        }
        base += w0 + w1 + w2 + w3;
    }
}

}  // namespace

int gta_maskidx_dispatch(const uint8_t* key_mask, int B, int Tk, int32_t* key_idx, int32_t* key_lens, uint8_t* k_live,
                         const uint8_t* query_mask, int Tq, int32_t* q_lens, hipStream_t stream) {
    const unsigned sides = (key_mask ? 1u : 0u) + (query_mask ? 1u : 0u);
    hipLaunchKernelGGL(gta_mask_index_kernel, dim3((unsigned)B, sides), dim3(256), 0, stream, key_mask, Tk, key_idx, key_lens, k_live,
                       query_mask, Tq, q_lens);
    return hipGetLastError() == hipSuccess ? GTA_OK : GTA_E_LAUNCH;
}
