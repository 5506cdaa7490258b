// gta_gen_params.h -- kernel argument block of the staged generic forward (gta_fwd_gen.hip; the host fills it in gta_abi.cpp).
#pragma once
#include <stdint.h>

struct GtaGenParams {
    const void* q; const void* k; const void* v; void* o; float* lse;
    void* img;                                  // workspace: K'/V' tile images, [B,H,n_tiles][K' image | V' image] (the ring format of gta_fwd2.hip)
    float* kbias;                               // workspace: per-key bias -0.5 scale |k'|^2, [B,H,n_tiles * 64] fp32 (euclid; else null)
    const float* vrep_q; const float* vrep_k;   // [B,N,GTA_VREP_STRIDE]
    const float* cs_q; const float* cs_k;       // [B,T,nso2,2] (cos,sin)
    const float* coord_q; const float* coord_k; // [B,T,2] (t2 slab)
    const float* trans_coeff; const float* tau; // device scalars or null
    long q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st;  // element strides
    int B, H, Tq, Tk, Nq, Nk;
    int dh, d_triv, d_se3, d_so3, d_so2, d_t2, L;
    int euclid, xv, esz;                        // GTA_FLAG_EUCLID, GTA_FLAG_V_TRANSFORM, bytes per element of q/k/v/out
    int n_qtiles, n_items, n_tiles;             // 128-row query tiles per (b,h); B * H * n_qtiles; 64-key tiles per (b,h)
    float scale;
    const int32_t* key_lens;                    // VARLEN instances: valid keys per scene (a prefix of Tk), [B] int32 on the device; else null (last: no other field moves)
};

long gta_gen_image_bytes(int B, int H, int Tk, int dhp);
long gta_gen_workspace_bytes(int B, int H, int Tk, int dhp);
int gta_gen_dispatch(const GtaGenParams& p, int dhp, bool run_prep, bool run_attn, void* stream);      // (p.key_lens set: the VARLEN instances)
// the same with the GATHER instances of the pre-pass: image row r of tile j of scene b from token key_idx[b, 64 j + r] ([B, Tk] int32 on the device)
int gta_gen_gather_dispatch(const GtaGenParams& p, const int32_t* key_idx, int dhp, bool run_prep, bool run_attn, void* stream);
const char* gta_gen_error();               // after a failed gta_gen_dispatch on this thread: HIP's own words for it (static storage)
