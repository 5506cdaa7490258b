// gta_fwd_gen.hip -- staged generic forward for gfx950: the two-stage plan of gta_fwd2.hip for ANY f_dims layout (t2 slab, euclid
// similarity, so3 of degree 1, slabs that start anywhere), dh % 8 == 0, dh <= 128.
//
// The fused kernels apply rho per 8-channel CHUNK in registers, which ties them to layouts whose blocks never straddle a chunk.  Here
// rho is applied per ROW in LDS by the row transform of the generic path (gta_rep_row.h: one lane walks its row's slabs block by
// block, fp32), which does not care where a slab starts; the matrix work is the loop of gta_fwd2.hip unchanged.
//
//   gta_gen_prep_kernel   one 64-key tile of one (b,h) per workgroup: K and V rows -> fp32 LDS stages (coalesced 16-byte loads),
//                         lane == key row applies rho_k (wave 0: K, with the euclid key bias -0.5 scale |k'|^2 from the fp32 k';
//                         wave 1: V), all four waves round to bf16 and write the K'/V' TILE IMAGES (the rotation-swizzled byte
//                         image the ring streams, gta_prep.hip's format) with 1-KiB wave stores.
//   gta_gen_attn_kernel   one work item = 128 query rows of one (b,h), 4 waves x 32 rows.  Prologue: a wave stages ITS 32 rows in
//                         LDS (the ring's space: the stream has not started), lanes 0-31 apply rho_q in place, every lane builds its
//                         bf16 MFMA B fragments (pre-scaled by scale * log2(e) / tau).  Loop: the 3-stage LDS-DMA ring, S^T = K' Q'^T
//                         and O^T = V'^T P^T on v_mfma_f32_32x32x16_bf16; under euclid a wave also streams the tile's 64 bias values
//                         into a slot of its own (one 256-byte LDS-DMA per tile) and adds them to S in fp32.  Epilogue: O~ / l through
//                         LDS (the ring's space again), rho_q^-1 per row, coalesced stores, LSE.
// No q', k', v' or o~ tensor exists in HBM; the only intermediate is the workspace [images | bias].
#include <hip/hip_runtime.h>
#include "gta_fwd2_tile.h"
#include "gta_rep_row.h"
#include "gta_gen_params.h"

namespace {

constexpr int GEN_BIAS_SLOT = BN * 4;                    // bytes of one tile's bias values

// the row transform's argument block for one side of the call: mode 0 / 2 the query side's tables, mode 1 the key side's
GTA_DEV ApplyParams gen_row_params(const GtaGenParams& p, int mode) {
    ApplyParams a;
    a.x = nullptr; a.y = nullptr;
    a.x_sb = a.x_sh = a.x_st = a.y_sb = a.y_sh = a.y_st = 0;
    a.vrep = mode == 1 ? p.vrep_k : p.vrep_q;
    a.cs = mode == 1 ? p.cs_k : p.cs_q;
    a.coord = mode == 1 ? p.coord_k : p.coord_q;
    a.trans_coeff = p.trans_coeff;
    a.key_bias = nullptr; a.bias_scale = p.scale; a.bias_pitch = (long)p.n_tiles * BN;
    a.B = p.B; a.H = p.H;
    a.T = mode == 1 ? p.Tk : p.Tq;
    a.N = mode == 1 ? p.Nk : p.Nq;
    a.P = a.T / a.N;
    a.d_triv = p.d_triv; a.d_se3 = p.d_se3; a.d_so3 = p.d_so3; a.d_so2 = p.d_so2; a.d_t2 = p.d_t2; a.L = p.L;
    a.mode = mode; a.euclid = p.euclid; a.esz = p.esz;
    return a;
}

// Rows [t0, t0 + R) of one (b,h) (base: its row 0, rs bytes between rows) -> an fp32 stage [R][dh + 1]: 16-byte units, consecutive
// threads take consecutive units of a row (coalesced); rows past T become zero rows.  NT threads share the work.  GATHER: stage row r is the
// row of token tok[r] (an LDS row of R token numbers, each inside the scene), still for t0 + r < T alone.
template <int NT, bool GATHER = false>
GTA_DEV void gen_rows_in(float* stage, const char* base, long rs, int t0, int T, int R, int dh, int esz, int tid, const int* tok = nullptr) {
    const int U = dh * esz / 16, per = 16 / esz;
    for (int idx = tid; idx < R * U; idx += NT) {
        const int r = idx / U, u = idx - r * U;
        float* dst = stage + r * (dh + 1) + u * per;
        u32x4_t w = {0u, 0u, 0u, 0u};
        if constexpr (GATHER) {
            if (t0 + r < T) w = *reinterpret_cast<const u32x4_t*>(base + (long)tok[r] * rs + u * 16);
        } else {
            if (t0 + r < T) w = *reinterpret_cast<const u32x4_t*>(base + (long)(t0 + r) * rs + u * 16);
        }
        if (esz == 2) {
            float x[8];
            unpack8(w, x);
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i] = x[i];
        } else {
            dst[0] = __uint_as_float(w.x); dst[1] = __uint_as_float(w.y); dst[2] = __uint_as_float(w.z); dst[3] = __uint_as_float(w.w);
        }
    }
}
// ... and back: the rows below T are written, rounded to the output type
template <int NT>
GTA_DEV void gen_rows_out(const float* stage, char* base, long rs, int t0, int T, int R, int dh, int esz, int tid) {
    const int U = dh * esz / 16, per = 16 / esz;
    for (int idx = tid; idx < R * U; idx += NT) {
        const int r = idx / U, u = idx - r * U;
        if (t0 + r >= T) continue;
        const float* src = stage + r * (dh + 1) + u * per;
        u32x4_t w;
        if (esz == 2) {
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = src[i];
            w = pack8(x);
        } else {
            w = u32x4_t{__float_as_uint(src[0]), __float_as_uint(src[1]), __float_as_uint(src[2]), __float_as_uint(src[3])};
        }
        *reinterpret_cast<u32x4_t*>(base + (long)(t0 + r) * rs + u * 16) = w;
    }
}

GTA_DEV const int32_t* first_gen_idx(const int32_t* key_idx) { return key_idx; }

template <int DHP>
struct GenPrepSmem {
    static constexpr int CHP = DHP / 8;
    static constexpr int IMG = BN * DHP * 2;
    static constexpr int STAGE_F = BN * (DHP + 1);        // floats of one fp32 row stage
    static constexpr int OFF_SK = 0;
    static constexpr int OFF_SV = OFF_SK + STAGE_F * 4;
    static constexpr int OFF_IMGK = OFF_SV + STAGE_F * 4;
    static constexpr int OFF_IMGV = OFF_IMGK + IMG;
    static constexpr int TOTAL = OFF_IMGV + IMG;
    static constexpr int OFF_TOK = TOTAL;                 // (GATHER instances alone) the tile's 64 token numbers
    static constexpr int TOTAL_GATHER = TOTAL + BN * 4;
    static_assert(OFF_IMGK % 16 == 0, "image alignment");
};

// VARLEN (both kernels): scene b's keys are the prefix of p.key_lens[b] tokens -- the pre-pass skips the tiles past it and treats the rows
// of its last tile past it as it treats the rows past Tk (zero rows, bias 0, no table read); the attention kernel walks and masks by it.
//
// GATHER (gta_attn_fwd_staged_gather; VARLEN plus a gather): scene b's keys are ANY p.key_lens[b] of its tokens, compacted -- image row r of
// tile j is built from token key_idx[b * Tk + 64 j + r] (clamped into [0, Tk): no value moves a load out of the scene's K, V or table rows):
// its K / V rows, its view record, its (cos, sin) and coord rows; its bias goes to the COMPACTED position 64 j + r.  The zero rows and the
// skipped tiles are those of VARLEN.  key_idx entries at or past the count are never read, nor is any token that no live entry names.  The
// GATHER instances alone take the trailing argument (IDX = const int32_t*: key_idx, [B, Tk] on the device) and 256 bytes of LDS for the
// tile's token numbers; without it IDX is empty and the kernel's arguments are what they were.
template <int DHP, bool VARLEN = false, class... IDX>
__global__ __launch_bounds__(256) void gta_gen_prep_kernel(const GtaGenParams p, const IDX... idx) {
    using S = GenPrepSmem<DHP>;
    constexpr int CHP = S::CHP;
    constexpr bool GATHER = sizeof...(IDX) == 1;
    static_assert(sizeof...(IDX) <= 1 && (!GATHER || VARLEN), "key_idx comes with GATHER, which compacts into a per-scene prefix");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // work map of gta_kv_prep_kernel: the H workgroups of one 64-token row tile are consecutive on ONE XCD (neighbouring heads share lines)
    int j, h, b;
    {
        const int L = blockIdx.x, x = L & 7, i = L >> 3;
        const int r = x + 8 * (i / p.H);
        h = i - (i / p.H) * p.H;
        if (r >= p.B * p.n_tiles) return;
        b = r / p.n_tiles;
        j = r - b * p.n_tiles;
    }
    int tk_b = 0;
    if constexpr (VARLEN) {
        tk_b = key_len_of(p.key_lens, b, p.Tk);
        if (j * BN >= tk_b) return;
    }
#define GTA_TKB (VARLEN ? tk_b : p.Tk)
    const int dh = p.dh, rowf = dh + 1;
    float* sk = reinterpret_cast<float*>(smem + S::OFF_SK);
    float* sv = reinterpret_cast<float*>(smem + S::OFF_SV);
    const char* kg = (const char*)p.k + ((long)b * p.k_sb + (long)h * p.k_sh) * p.esz;
    const char* vg = (const char*)p.v + ((long)b * p.v_sb + (long)h * p.v_sh) * p.esz;
    const int t = j * BN + lane;
    const int* stok = nullptr;
    if constexpr (GATHER) {
        // the tile's token numbers -> LDS (a dead row's entry is not read from key_idx, and never used)
        int* w = reinterpret_cast<int*>(smem + S::OFF_TOK);
        if (wave == 0) w[lane] = t < tk_b ? min(max(first_gen_idx(idx...)[(long)b * p.Tk + t], 0), p.Tk - 1) : 0;
        __syncthreads();
        stok = w;
    }
    gen_rows_in<256, GATHER>(sk, kg, p.k_st * p.esz, j * BN, GTA_TKB, BN, dh, p.esz, tid, stok);
    gen_rows_in<256, GATHER>(sv, vg, p.v_st * p.esz, j * BN, GTA_TKB, BN, dh, p.esz, tid, stok);
    __syncthreads();
    // rho_k: lane == key row; the rows past Tk stay zero rows (score 0 and bias 0: the attention kernel masks them).  (GATHER) rho_k of the
    // row's TOKEN -- its view record, its (cos, sin) and coord rows --, the bias at the compacted position t
    int tok = t;
    if constexpr (GATHER) tok = stok[lane];
    if (wave == 0) {
        ApplyParams a = gen_row_params(p, 1);
        a.key_bias = p.kbias;
        if (t < GTA_TKB) apply_row(a, b, h, tok, LIn{sk + lane * rowf}, LOut{sk + lane * rowf}, GATHER ? t : -1);
        else if (p.kbias) p.kbias[((long)b * p.H + h) * a.bias_pitch + t] = 0.f;
    } else if (wave == 1 && p.xv) {
        const ApplyParams a = gen_row_params(p, 1);
        if (t < GTA_TKB) apply_row(a, b, h, tok, LIn{sv + lane * rowf}, LOut{sv + lane * rowf});
    }
#undef GTA_TKB
    __syncthreads();
    // fp32 rows -> bf16 images: an 8-channel chunk per wave and iteration, lane == key row (odd row pitch: conflict-free reads)
#pragma unroll
    for (int it = 0; it < CHP / 4; ++it) {
        const int c = wave + 4 * it;
        const int off = (lane * CHP + swz<CHP>(lane, c)) * 16;
        float x[8], y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            x[i] = 8 * c < dh ? sk[lane * rowf + 8 * c + i] : 0.f;
            y[i] = 8 * c < dh ? sv[lane * rowf + 8 * c + i] : 0.f;
        }
        *reinterpret_cast<u32x4_t*>(smem + S::OFF_IMGK + off) = pack8(x);
        *reinterpret_cast<u32x4_t*>(smem + S::OFF_IMGV + off) = pack8(y);
    }
    __syncthreads();
    // LDS images -> workspace, 1 KiB contiguous per wave-instruction ([K' image | V' image] are adjacent on both sides)
    char* gimg = (char*)p.img + (((long)b * p.H + h) * p.n_tiles + j) * (2L * S::IMG);
    constexpr int PIECES = 2 * S::IMG / 1024;
#pragma unroll
    for (int i = 0; i < PIECES / 4; ++i) {
        const int piece = wave + 4 * i;
        *reinterpret_cast<u32x4_t*>(gimg + piece * 1024 + lane * 16) = *reinterpret_cast<const u32x4_t*>(smem + S::OFF_IMGK + piece * 1024 + lane * 16);
    }
}

// one tile's 64 bias values -> a wave's slot, one LDS-DMA (4 bytes per lane); consumers sit behind the ring's counted vmcnt wait
GTA_DEV void gen_bias_dma(uint32_t lds, const float* src, int lane) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" ::"s"(lds), "v"((unsigned)lane * 4u), "s"(src) : "memory");
}

template <int DHP, bool BIAS, bool VARLEN = false>
__global__ __launch_bounds__(256, (DHP <= 96 ? 2 : 1)) void gta_gen_attn_kernel(const GtaGenParams p) {
    using S = Smem2<DHP>;
    constexpr int CHP = S::CHP, KS = DHP / 16, DB = DHP / 32, BM = S::BM;
    constexpr int DMA_PER_WAVE = S::STAGE / 1024 / 4 + (BIAS ? 1 : 0);
    static_assert(BM * (DHP + 1) * 4 <= S::RING_BYTES, "the query / output row stages live in the ring's space");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;
    char* bias_ring = smem + S::RING_BYTES;               // [NST][4 waves][64] floats (BIAS)
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_tiles = p.n_tiles, dh = p.dh, rowf = dh + 1;
    const int w = item_of(blockIdx.x, p.n_items);
    const int bh = w / p.n_qtiles, qt = w - bh * p.n_qtiles;
    const int b = bh / p.H, h = bh - b * p.H, q0 = qt * BM;
    const float inv_tau = 1.0f / (p.tau ? *p.tau : 1.0f);
    const float qscale = p.scale * LOG2E * inv_tau, bsc = LOG2E * inv_tau;
    // (VARLEN) this item's key side: tk_b keys in nt_b tiles; the workspace keeps the strides of n_tiles
    int tk_b = 0, nt_b = 0;
    if constexpr (VARLEN) {
        tk_b = key_len_of(p.key_lens, b, p.Tk);
        nt_b = (tk_b + BN - 1) / BN;
    }
#define GTA_NT (VARLEN ? nt_b : n_tiles)
#define GTA_TK (VARLEN ? tk_b : p.Tk)

    // ---- prologue: this wave's 32 query rows -> LDS, rho_q per row (fp32, in place), bf16 B fragments ----
    float* srow = reinterpret_cast<float*>(smem) + wave * 32 * rowf;
    const int t0 = q0 + wave * 32;
    {
        const char* qg = (const char*)p.q + ((long)b * p.q_sb + (long)h * p.q_sh) * p.esz;
        gen_rows_in<64>(srow, qg, p.q_st * p.esz, t0, p.Tq, 32, dh, p.esz, lane);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (one wave, LDS in order: the rows are there for every lane)
    if (lane < 32 && t0 + lane < p.Tq) {
        const ApplyParams a = gen_row_params(p, 0);
        apply_row(a, b, h, t0 + lane, LIn{srow + lane * rowf}, LOut{srow + lane * rowf});
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8_t qf[KS];                                     // lane (l31, lh): row 32 wave + l31, chunks 2 ks + lh
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        float x[8];
        const int ch = 16 * ks + 8 * lh;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = ch < dh ? srow[l31 * rowf + ch + i] * qscale : 0.f;
        qf[ks] = __builtin_bit_cast(bf16x8_t, pack8(x));
    }
    __syncthreads();                                     // every wave is done with its rows: the ring may start

    // ---- the K'/V' (+ bias) DMA stream: tile t into ring stage t % 3 ----
    int dma_t = 0, dma_st = 0, cons_st = 0;
    const char* img = (const char*)p.img + (long)bh * n_tiles * (long)S::STAGE;
    const float* kb = BIAS ? p.kbias + (long)bh * n_tiles * BN : nullptr;
    auto dma_next = [&]() {
        if (dma_t < GTA_NT) {
            dma_stage<DHP>(ring, dma_st, img + (long)dma_t * S::STAGE, wave, lane);
            if constexpr (BIAS) gen_bias_dma(lds_addr(bias_ring + (dma_st * 4 + wave) * GEN_BIAS_SLOT), kb + dma_t * BN, lane);
            dma_st = dma_st == S::NST - 1 ? 0 : dma_st + 1;
            ++dma_t;
        }
    };
#pragma unroll
    for (int i0 = 0; i0 < S::NST - 1; ++i0) dma_next();

    // lane-constant LDS offsets (gta_fwd2_kernel): K' fragment row l31, unit 2ks + lh; V' transpose-read
    int koff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = (l31 * CHP + swz<CHP>(l31, 2 * ks + lh)) * 16;
    int voff[DB][2];
    {
        const int g16 = lane >> 4, p16 = lane & 15;
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            const int u = 4 * d + 2 * (g16 & 1) + ((p16 & 3) >> 1);
            const int hb = (p16 & 1) * 8;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int r = 4 * lh + (p16 >> 2) + 8 * hf;
                voff[d][hf] = (r * CHP + swz<CHP>(r, u)) * 16 + hb;
            }
        }
    }
    f32x16_t oacc[DB];
    float m_run = 0.f, l_run = 0.f;
    f32x16_t msplat;                      // -m_run in every element: C operand of each tile's first MFMA (S' = S - m)
#pragma unroll
    for (int i = 0; i < 16; ++i) msplat[i] = 0.f;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[d][i] = 0.f;
    const bool has_tail = (GTA_TK & (BN - 1)) != 0;

    for (int j = 0; j < GTA_NT; ++j) {
        // tile j has landed (only the stream's next tile may still be in flight), everyone is past tile j - 1
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S::NST - 2) * DMA_PER_WAVE) : "memory");
        if (dma_t >= GTA_NT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the stream has ended: nothing younger to count on)
        __builtin_amdgcn_s_barrier();
        dma_next();
        const char* kf = ring + cons_st * S::STAGE;
        const float* bl = reinterpret_cast<const float*>(bias_ring + (cons_st * 4 + wave) * GEN_BIAS_SLOT) + 4 * lh;
        cons_st = cons_st == S::NST - 1 ? 0 : cons_st + 1;

        // ---- S^T = K' Q'^T (relative to the running max) ----
        f32x16_t s[2];
        {
            bf16x8_t ka[KS], kb2[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                ka[ks] = *reinterpret_cast<const bf16x8_t*>(kf + koff[ks]);
                kb2[ks] = *reinterpret_cast<const bf16x8_t*>(kf + koff[ks] + 32 * CHP * 16);
            }
            __builtin_amdgcn_sched_barrier(0);
            s[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[0], qf[0], msplat, 0, 0, 0);
            s[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2[0], qf[0], msplat, 0, 0, 0);
#pragma unroll
            for (int ks = 1; ks < KS; ++ks) {
                s[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[ks], qf[ks], s[0], 0, 0, 0);
                s[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb2[ks], qf[ks], s[1], 0, 0, 0);
            }
        }
        // the per-key bias, given before the temperature (gta_fwd_kernel): key of register r = 4 lh + (r & 3) + 8 (r >> 2) (+ 32 for s[1])
        if constexpr (BIAS) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bl + 8 * g);
                const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(bl + 32 + 8 * g);
                s[0][4 * g] += bsc * b0.x; s[0][4 * g + 1] += bsc * b0.y; s[0][4 * g + 2] += bsc * b0.z; s[0][4 * g + 3] += bsc * b0.w;
                s[1][4 * g] += bsc * b1.x; s[1][4 * g + 1] += bsc * b1.y; s[1][4 * g + 2] += bsc * b1.z; s[1][4 * g + 3] += bsc * b1.w;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // (no compiler-tracked LDS read is in flight past here)
        __builtin_amdgcn_sched_barrier(0);
        // V' slab 0 transpose-reads fly under the softmax
        const uint32_t vbase = lds_addr(kf + S::IMG);
        u32x2_t v0l[DB], v0h[DB], v1l[DB], v1h[DB], v2l[DB], v2h[DB], v3l[DB], v3h[DB];
        pv_reads_slab<DHP, 0>(vbase, voff, v0l, v0h);

        // online softmax with the true row max of every tile (a bias is unbounded below: the lazy bound of gta_fwd2_kernel does not hold)
        bf16x8_t pf[2][2];
        softmax_rebase<DHP>(s[0], s[1], m_run, l_run, oacc, msplat, j == 0, has_tail && j == GTA_NT - 1, j * BN + 4 * lh, GTA_TK);
        softmax_exp_pack(s[0], s[1], l_run, pf);

        // ---- O^T += V'^T P^T, slab-major; reads stay one slab ahead (LDS returns in order) ----
        pv_reads_slab<DHP, 1>(vbase, voff, v1l, v1h);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * DB) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        pv_mfma_slab<DHP>(v0l, v0h, pf, 0, 0, oacc);
        pv_reads_slab<DHP, 2>(vbase, voff, v2l, v2h);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * DB) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        pv_mfma_slab<DHP>(v1l, v1h, pf, 0, 1, oacc);
        pv_reads_slab<DHP, 3>(vbase, voff, v3l, v3h);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * DB) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        pv_mfma_slab<DHP>(v2l, v2h, pf, 1, 0, oacc);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        pv_mfma_slab<DHP>(v3l, v3h, pf, 1, 1, oacc);
    }
    __syncthreads();                                     // every wave is past the last tile: the ring's space is free again

    // ---- epilogue: O~ / l -> this wave's rows in LDS, rho_q^-1 per row, coalesced stores ----
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv_l = 1.0f / l_tot;
    if (p.lse && lh == 0 && t0 + l31 < p.Tq) p.lse[((long)b * p.H + h) * p.Tq + t0 + l31] = (m_run + __log2f(l_tot)) * LN2;
    // the accumulators hold, per lane (row l31), the 4-channel half lh of every chunk: channel 32 d + 8 g + 4 lh + i in oacc[d][4 g + i]
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = 32 * d + 8 * g + 4 * lh;
            if (ch < dh) {
#pragma unroll
                for (int i = 0; i < 4; ++i) srow[l31 * rowf + ch + i] = oacc[d][4 * g + i] * inv_l;
            }
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (p.xv && lane < 32 && t0 + lane < p.Tq) {
        const ApplyParams a = gen_row_params(p, 2);
        apply_row(a, b, h, t0 + lane, LIn{srow + lane * rowf}, LOut{srow + lane * rowf});
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    {
        char* og = (char*)p.o + ((long)b * p.o_sb + (long)h * p.o_sh) * p.esz;
        gen_rows_out<64>(srow, og, p.o_st * p.esz, t0, p.Tq, 32, dh, p.esz, lane);
    }
#undef GTA_NT
#undef GTA_TK
}

// what HIP said about the launch that failed: reading the error clears it, so the reader keeps the text for the caller's message
thread_local const char* g_gen_error = "";
int gen_hip_status(int rc_on_error) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        if (rc_on_error == GTA_E_NODEVICE) g_gen_error = "no HIP device";
        return GTA_OK;
    }
    g_gen_error = hipGetErrorString(e);
    return rc_on_error;
}

template <int DHP, bool VARLEN, class... IDX>
int launch_gen_prep(const GtaGenParams& p, hipStream_t stream, IDX... idx) {
    using S = GenPrepSmem<DHP>;
    constexpr int lds = sizeof...(IDX) ? S::TOTAL_GATHER : S::TOTAL;
    if (int rc = gta_lds_optin<&gta_gen_prep_kernel<DHP, VARLEN, IDX...>>(lds)) { gen_hip_status(rc); return rc; }
    const long rows = (long)p.B * p.n_tiles;
    const long grid = (rows + 7) / 8 * 8 * p.H;
    if (grid > 0x7fffffffL) { g_gen_error = "pre-pass grid too large"; return GTA_E_UNSUPPORTED; }
    hipLaunchKernelGGL((gta_gen_prep_kernel<DHP, VARLEN, IDX...>), dim3((unsigned)grid), dim3(256), lds, stream, p, idx...);
    return gen_hip_status(GTA_E_LAUNCH);
}

template <int DHP, bool BIAS>
constexpr int gen_attn_lds() { return Smem2<DHP>::RING_BYTES + (BIAS ? Smem2<DHP>::NST * 4 * GEN_BIAS_SLOT : 0); }

template <int DHP, bool BIAS, bool VARLEN>
int launch_gen_attn(const GtaGenParams& p, hipStream_t stream) {
    constexpr int lds = gen_attn_lds<DHP, BIAS>();
    if (int rc = gta_lds_optin<&gta_gen_attn_kernel<DHP, BIAS, VARLEN>>(lds)) { gen_hip_status(rc); return rc; }
    hipLaunchKernelGGL((gta_gen_attn_kernel<DHP, BIAS, VARLEN>), dim3((unsigned)p.n_items), dim3(256), lds, stream, p);
    return gen_hip_status(GTA_E_LAUNCH);
}

// The LDS of every instance, as profiles/staged_generic/README.md and tools/audit_spills.py report it: a change of the layouts above
// fails here until those are brought along.
static_assert(GenPrepSmem<32>::TOTAL == 25088 && GenPrepSmem<64>::TOTAL == 49664 && GenPrepSmem<96>::TOTAL == 74240 &&
              GenPrepSmem<128>::TOTAL == 98816, "pre-pass LDS bytes");
static_assert(gen_attn_lds<32, false>() == 24576 && gen_attn_lds<64, false>() == 49152 && gen_attn_lds<96, false>() == 73728 &&
              gen_attn_lds<128, false>() == 98304, "attention LDS bytes");
static_assert(gen_attn_lds<32, true>() == 27648 && gen_attn_lds<64, true>() == 52224 && gen_attn_lds<96, true>() == 76800 &&
              gen_attn_lds<128, true>() == 101376, "attention LDS bytes with the bias slots");

template <int DHP>
int gen_dispatch(const GtaGenParams& p, bool gather, const int32_t* key_idx, bool run_prep, bool run_attn, hipStream_t stream) {
    if (p.key_lens) {                                     // the VARLEN instances (gta_attn_fwd_staged_varlen); gather: the GATHER pre-pass before them
        if (run_prep)
            if (int rc = gather ? launch_gen_prep<DHP, true>(p, stream, key_idx) : launch_gen_prep<DHP, true>(p, stream)) return rc;
        if (!run_attn) return GTA_OK;
        return p.kbias ? launch_gen_attn<DHP, true, true>(p, stream) : launch_gen_attn<DHP, false, true>(p, stream);
    }
    if (run_prep)
        if (int rc = launch_gen_prep<DHP, false>(p, stream)) return rc;
    if (!run_attn) return GTA_OK;
    return p.kbias ? launch_gen_attn<DHP, true, false>(p, stream) : launch_gen_attn<DHP, false, false>(p, stream);
}

}  // namespace

long gta_gen_image_bytes(int B, int H, int Tk, int dhp) {
    const long n_tiles = (Tk + BN - 1) / BN;
    return (long)B * H * n_tiles * 2L * BN * dhp * 2;
}
// workspace = [K'/V' tile images | per-key bias, 64 floats per tile (written under euclid)]
long gta_gen_workspace_bytes(int B, int H, int Tk, int dhp) {
    const long n_tiles = (Tk + BN - 1) / BN;
    return ((gta_gen_image_bytes(B, H, Tk, dhp) + 255) & ~255L) + (long)B * H * n_tiles * GEN_BIAS_SLOT;
}

const char* gta_gen_error() { return g_gen_error; }

namespace {
int gen_dispatch_dhp(const GtaGenParams& p, bool gather, const int32_t* key_idx, int dhp, bool run_prep, bool run_attn, void* stream) {
    g_gen_error = "no kernel instance";
    switch (dhp) {
        case 32: return gen_dispatch<32>(p, gather, key_idx, run_prep, run_attn, (hipStream_t)stream);
        case 64: return gen_dispatch<64>(p, gather, key_idx, run_prep, run_attn, (hipStream_t)stream);
        case 96: return gen_dispatch<96>(p, gather, key_idx, run_prep, run_attn, (hipStream_t)stream);
        case 128: return gen_dispatch<128>(p, gather, key_idx, run_prep, run_attn, (hipStream_t)stream);
    }
    return GTA_E_UNSUPPORTED;
}
}  // namespace

int gta_gen_dispatch(const GtaGenParams& p, int dhp, bool run_prep, bool run_attn, void* stream) {
    return gen_dispatch_dhp(p, false, nullptr, dhp, run_prep, run_attn, stream);
}

// the GATHER pre-pass (gta_attn_fwd_staged_gather): p.key_lens counts the compacted keys, key_idx names them (read by the pre-pass alone)
int gta_gen_gather_dispatch(const GtaGenParams& p, const int32_t* key_idx, int dhp, bool run_prep, bool run_attn, void* stream) {
    g_gen_error = "the gather comes with key_lens, and its pre-pass with key_idx";
    if (!p.key_lens || (run_prep && !key_idx)) return GTA_E_BADARG;
    return gen_dispatch_dhp(p, true, key_idx, dhp, run_prep, run_attn, stream);
}
