// gta_fwd2_tile.h -- the tile-loop pieces of the 128-row two-stage attention kernels (gta_fwd2.hip, gta_fwd_gen.hip): LDS layout of the
// K'/V' image ring, its LDS-DMA, the lazy online softmax on S^T accumulators and the slab-major P V steps.
// Everything has internal linkage (anonymous namespace): each .hip is its own module.
#pragma once
#include "gta_flash_common.h"

namespace {

// X3 = the fp32-faithful instances (GTA_FLAG_FP32_PRODUCTS on the two-stage plan, fp32 inputs, dh <= 64): a tile is FOUR images
// [K'hi | V'hi | K'lo | V'lo] (gta_prep.hip), the ring has two stages (2 x 32 KiB at dh = 64: two workgroups per CU).
template <int DHP, bool X3 = false>
struct Smem2 {
    static constexpr int NW = 4;
    static constexpr int BM = 32 * NW;                  // 128 query rows per work item
    static constexpr int NT = 64 * NW;
    static constexpr int CHP = DHP / 8;
    static constexpr int IMG = BN * DHP * 2;            // one K' or V' tile image
    static constexpr int STAGE = (X3 ? 4 : 2) * IMG;    // K' image then V' image (X3: then their lo parts)
    static constexpr int NST = X3 ? 2 : NSTAGE;         // ring stages
    static constexpr int RING_BYTES = NST * STAGE;
    // layout: [ring | q-side view records, two buffers (item parity) of nrec records each]
    static constexpr int OFF_RING = 0;
    static constexpr int OFF_QREC = RING_BYTES;
    __host__ __device__ static int total(int nrec) { return RING_BYTES + 2 * nrec * GTA_QREC * 4; }
};

// issue the LDS-DMA of one K'/V' tile image pair (STAGE bytes, linear) into ring stage `st` (dma_group: gta_common.h)
template <int DHP, bool X3 = false>
GTA_DEV void dma_stage(char* ring, int st, const char* img, int wave, int lane) {
    using S = Smem2<DHP, X3>;
    constexpr int PIECES = S::STAGE / 1024;             // 1 KiB per wave-instruction
    constexpr int PER_WAVE = PIECES / 4;
    static_assert(PIECES % 4 == 0, "stage must split evenly over the waves");
    const unsigned voff = (unsigned)lane * 16u;
    const char* base = img + wave * (PER_WAVE * 1024);
    const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)(ring + st * S::STAGE + wave * (PER_WAVE * 1024));
    static_for<(PER_WAVE + 3) / 4>([&](auto GC) {
        constexpr int g = decltype(GC)::value, np = PER_WAVE - 4 * g < 4 ? PER_WAVE - 4 * g : 4;
        dma_group<np>(lds + g * 4096, base + g * 4096, voff);
    });
}

// Full path of the lazy softmax (tile 0, masked tail, violated bound): true row max of S' (= S - m_run), move
// m_run there, rescale l and O, re-base S' and the -m splat.  key of register r = kbase + (r&3) + 8(r>>2) (+32).
// The masked last key tile: the rows past Tk are zero rows of the images (score 0, not -inf), so their probabilities must be struck
// from the row sums.  Key of register r = 4 lh + (r & 3) + 8 (r >> 2) (+ 32 for s1): when the tile's valid keys are a whole number g of
// 8-key groups (CLEVR-TR: 600 = 9 x 64 + 24) the dead registers are the same in every lane -- wave-uniform branches and moves, no
// per-register compare / select pairs, and no reason to leave the lazy softmax (other remainders keep the full path's per-register mask).
GTA_DEV void mask_tail8(f32x16_t& s0, f32x16_t& s1, int g) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q >= g) {
#pragma unroll
            for (int i = 0; i < 4; ++i) s0[4 * q + i] = -1e30f;
        }
        if (q + 4 >= g) {
#pragma unroll
            for (int i = 0; i < 4; ++i) s1[4 * q + i] = -1e30f;
        }
    }
}
template <int DHP, bool MASK = true>
GTA_DEV void softmax_rebase(f32x16_t& s0, f32x16_t& s1, float& m_run, float& l_run, f32x16_t (&oacc)[DHP / 32],
                            f32x16_t& msplat, bool first, bool tail, int kbase, int Tk) {
    if (MASK && tail) {                         // (the skewed dh = 96 loop masks here, per register: a call of mask_tail costs that instance 10 spills)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kbase + (r & 3) + 8 * (r >> 2);
            if (key >= Tk) s0[r] = -1e30f;
            if (key + 32 >= Tk) s1[r] = -1e30f;
        }
    }
    float mx = s0[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s0[r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s1[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float delta = first ? mx : fmaxf(mx, 0.f);
    const float alpha = __builtin_amdgcn_exp2f(-delta);
    m_run += delta;
    l_run *= alpha;
#pragma unroll
    for (int d = 0; d < DHP / 32; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[d][i] *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] -= delta; s1[r] -= delta; msplat[r] = -m_run; }
}
// P = exp2(S'), row sum, bf16 MFMA B fragments
GTA_DEV void softmax_exp_pack(f32x16_t& s0, f32x16_t& s1, float& l_run, bf16x8_t (&pf)[2][2]) {
    float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = __builtin_amdgcn_exp2f(s0[r]); rs0 += s0[r]; }
#pragma unroll
    for (int r = 0; r < 16; ++r) { s1[r] = __builtin_amdgcn_exp2f(s1[r]); rs1 += s1[r]; }
    l_run += rs0 + rs1;
    u32x4_t ww;
    ww.x = pack_bf16x2(s0[0], s0[1]); ww.y = pack_bf16x2(s0[2], s0[3]);
    ww.z = pack_bf16x2(s0[4], s0[5]); ww.w = pack_bf16x2(s0[6], s0[7]);
    pf[0][0] = __builtin_bit_cast(bf16x8_t, ww);
    ww.x = pack_bf16x2(s0[8], s0[9]); ww.y = pack_bf16x2(s0[10], s0[11]);
    ww.z = pack_bf16x2(s0[12], s0[13]); ww.w = pack_bf16x2(s0[14], s0[15]);
    pf[0][1] = __builtin_bit_cast(bf16x8_t, ww);
    ww.x = pack_bf16x2(s1[0], s1[1]); ww.y = pack_bf16x2(s1[2], s1[3]);
    ww.z = pack_bf16x2(s1[4], s1[5]); ww.w = pack_bf16x2(s1[6], s1[7]);
    pf[1][0] = __builtin_bit_cast(bf16x8_t, ww);
    ww.x = pack_bf16x2(s1[8], s1[9]); ww.y = pack_bf16x2(s1[10], s1[11]);
    ww.z = pack_bf16x2(s1[12], s1[13]); ww.w = pack_bf16x2(s1[14], s1[15]);
    pf[1][1] = __builtin_bit_cast(bf16x8_t, ww);
}

// transpose-reads of one 16-key slab of V' for all DB channel blocks (2*DB reads)
template <int DHP, int SLAB>
GTA_DEV void pv_reads_slab(uint32_t vbase, const int (&voff)[DHP / 32][2], u32x2_t (&vlo)[DHP / 32], u32x2_t (&vhi)[DHP / 32]) {
    constexpr int OFF = SLAB * 16 * (DHP / 8) * 16;
#pragma unroll
    for (int d = 0; d < DHP / 32; ++d) {
        vlo[d] = lds_tr16_b64<OFF>(vbase + voff[d][0]);
        vhi[d] = lds_tr16_b64<OFF>(vbase + voff[d][1]);
    }
}
// SLAB-major PV: one slab's fragments multiply into DB independent accumulators
// (a chain on one accumulator would run at the dependent latency instead of the issue rate)
template <int DHP>
GTA_DEV void pv_mfma_slab(const u32x2_t (&vlo)[DHP / 32], const u32x2_t (&vhi)[DHP / 32], const bf16x8_t (&pf)[2][2],
                          int kb, int t, f32x16_t (&oacc)[DHP / 32]) {
#pragma unroll
    for (int d = 0; d < DHP / 32; ++d) {
        const u32x4_t av = {vlo[d].x, vlo[d].y, vhi[d].x, vhi[d].y};
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, av), pf[kb][t], oacc[d], 0, 0, 0);
    }
}

// work item V (virtual workgroup id) -> w: all query tiles of one (b,h) land on one XCD (K'/V' stay in that XCD's L2).
// Virtual ids V = blockIdx.x + k * gridDim.x keep the XCD of blockIdx.x when gridDim.x is a multiple of 8.
GTA_DEV int item_of(int V, int n_items) {
    const int xcd = V & 7, idx = V >> 3, q8 = n_items >> 3, r8 = n_items & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
}

}  // namespace
