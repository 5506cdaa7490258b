// gta_fwd_params.h -- kernel argument block of the fused forward (host fills it in gta_abi.cpp).
#pragma once
#include <stdint.h>

struct GtaFwdParams {
    const void* q; const void* k; const void* v; void* o; float* lse;
    void* kp;                                   // K'/V' tile-image workspace (two-stage path)
    float* kn;                                  // per key tile: max_k |k'_k| of the bf16 image rows, [B,H,n_tiles] (or null)
    void* qtiles;                               // q-side rep matrices as bf16 MFMA operand tiles, [B,Nq,GTA_QT_TILES][1 KiB] (gta_flash_common.h; or null)
    const float* vrep_q; const float* vrep_k;   // [B,N,GTA_VREP_STRIDE]
    const float* cs_q; const float* cs_k;       // [B,T,nso2,2] (cos,sin)
    const float* trans_coeff; const float* tau; // device scalars or null
    // One slot, two readers that never meet.  kbias: optional additive per-key bias (log2 units), [B,H,pitch] -- read by the single-kernel
    // forward alone (gta_fwd_kernel under gta_attn_fwd_plain).  key_lens: valid keys per scene (a prefix of Tk), [B] int32 on the device --
    // read by the VARLEN instances of the two-stage plan alone (gta_kv_prep_kernel, gta_fwd2_kernel), which GtaFwdSel::varlen selects (never the
    // pointer: a bias that reached the two-stage dispatch would otherwise be read as lengths).  The block
    // stays 96 dwords, so the hidden arguments behind it (the grid size the item loops read) stay put and every other instance compiles as before.
    union { const float* kbias; const int32_t* key_lens; };
    long kbias_pitch;
    long q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st;  // element strides
    int B, H, Tq, Tk, Nq, Nk, Pq, Pk;           // P* = tokens per view
    float invPq, invPk;
    float inv_nqt, invH;                        // 1 / n_qtiles, 1 / H (gta_attn64_kernel's item decode)
    int dh, nso2, n_qtiles;
    int n_items;                                // work items of the attention kernel: B * H * n_qtiles
    int per_cu;                                 // persistent grid: workgroups resident per CU (0: one workgroup per item)
    int nrec;                                   // q-side view records staged per item (views a 128-row tile can touch)
    uint32_t flags;
    unsigned long long* prof;                   // debug: per-workgroup phase timestamps (or null)
    uint32_t dbg;                               // ablation bits (GTA_DBG env; 0 in production)
    float scale;
    uint32_t ctab[16];                          // chunk descriptors (gta_common.h)
};

// the split-bf16 (X3) instances of GTA_FLAG_FP32_PRODUCTS exist on the two-stage forward and in the backward for fp32 inputs at dh <= 64
// (CLEVR-TR, runs/clevrtr/GTA/gta/config.yaml:55); other head sizes keep the single-kernel forward (gta_fwd_kernel<..., x3>)
inline bool gta_x3_takes(int dhp, int esz) { return esz == 4 && dhp <= 64; }

// which forward instance a call runs: gta_fwd_select (gta_fwd64.hip) decides once per call; the launches, the profiler's item count and
// gta_debug_attention_kernel read the decision
enum GtaFwdKind { GTA_FWD_SINGLE, GTA_FWD_FWD2, GTA_FWD_FWD2_X3, GTA_FWD_FWDC, GTA_FWD_ATTN64, GTA_FWD_ATTN64_ITEMS };
struct GtaFwdSel {
    GtaFwdKind kind;
    int layout;                                 // GTA_LAYOUT_* the chunk table is (gta_common.h)
    bool coal;                                  // attn64 kinds: the instance with coalesced item I/O
    bool qtiles;                                // the attention kernel reads the q-side rep tiles (p.qtiles)
    int rows;                                   // query rows per work item
    const char* name;                           // the kernel's own name
    bool varlen = false;                        // the VARLEN instances of the pre-pass and of gta_fwd2_kernel: p.key_lens is the slot's reader (gta_attn_fwd_varlen sets it)
    // the GATHER instances of the pre-pass (gta_attn_fwd_gather sets both, with varlen): the scene's keys are the tokens key_idx names, [B, Tk]
    // int32 on the device, compacted into the prefix p.key_lens counts.  The attention kernel is the VARLEN one and never sees the indices.
    bool gather = false;
    const int32_t* key_idx = nullptr;
    // the QMASK instances of gta_fwd2_kernel (gta_attn_fwd_qmask sets both, with varlen and gather): q_live [B, Tq] uint8 on the device, non-zero =
    // a live query row.  A trailing kernel argument of those instances alone, so it rides here and not in GtaFwdParams
    bool qmask = false;
    const uint8_t* q_live = nullptr;
};
// p: the argument block with the operands of the call (p.kp = the workspace or null; p.kn, p.qtiles inside it)
GtaFwdSel gta_fwd_select(const GtaFwdParams& p, int dhp, int esz);
