// gta_abi.cpp -- extern "C" boundary of libgta_hip.so: argument validation, the chunk table that
// encodes the reference's slab layout (gta.py:115-122), kernel dispatch.  No state, no allocation.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdlib.h>

#include "../../include/gta_hip.h"
#include "gta_fwd_params.h"
#include "gta_bwd_params.h"
#include "gta_repgrad_params.h"
#include "gta_gen_params.h"
#include "gta_merge_params.h"

// chunk-descriptor constants (mirrors gta_common.h, which is device-only)
#define HALF_ID 0u
#define HALF_SE3 1u
#define HALF_SO2 2u
#define CHUNK_SO3 (1u << 4)

int gta_fwd_lds_bytes(int dhp, int esz);
int gta_fwd_dispatch(const GtaFwdParams& p, int dhp, int esz, bool dma, int n_wg, hipStream_t stream);
long gta_fwd2_workspace_bytes(int B, int H, int Tk, int dhp, int Nq, int esz, bool x3);
long gta_fwd2_qtiles_offset(int B, int H, int Tk, int dhp, bool x3);
long gta_fwd2_image_bytes(int B, int H, int Tk, int dhp, bool x3);
int gta_fwd2_lds_bytes(int dhp, int nq);
int gta_fwd2_dispatch(GtaFwdParams& p, const GtaFwdSel& s, int dhp, int esz, bool run_prep, bool run_flash, hipStream_t stream);
int gta_bwd_dispatch(const GtaBwdParams& p, const float* dlse, int dhp, int esz, hipStream_t stream);
int gta_merge_dispatch(const GtaMergeParams& p, int esz, hipStream_t stream);
int gta_merge_bwd_dispatch(const GtaMergeBwdParams& p, int esz, hipStream_t stream);
int gta_maskidx_dispatch(const uint8_t* key_mask, int B, int Tk, int32_t* key_idx, int32_t* key_lens, uint8_t* k_live,
                         const uint8_t* query_mask, int Tq, int32_t* q_lens, hipStream_t stream);
int gta_bwd_varlen_dispatch(const GtaBwdParams& p, const int32_t* key_lens, const int32_t* q_lens, const float* dlse, int dhp, int esz, hipStream_t stream);
int gta_bwd_gather_dispatch(const GtaBwdParams& p, const int32_t* key_idx, const int32_t* key_lens, const float* dlse, int dhp, int esz, hipStream_t stream);
int gta_bwd_qmask_dispatch(const GtaBwdParams& p, const int32_t* key_idx, const int32_t* key_lens, const int32_t* q_lens, const uint8_t* q_live,
                           const float* dlse, int dhp, int esz, hipStream_t stream);

namespace {

thread_local const char* g_detail = "";

int fail(int code, const char* why) { g_detail = why; return code; }

int padded_dh(int dh) { return dh <= 32 ? 32 : dh <= 64 ? 64 : dh <= 96 ? 96 : dh <= 128 ? 128 : -1; }

int esz_of(const GtaAttnDesc* d) { return d->dtype == GTA_DTYPE_BF16 ? 2 : 4; }

// what a dispatcher returned: GTA_E_LAUNCH carries HIP's text, anything else `what`
int launch_status(int rc, const char* what) {
    return rc ? fail(rc, rc == GTA_E_LAUNCH ? hipGetErrorString(hipGetLastError()) : what) : GTA_OK;
}

int check_header(const GtaAttnDesc* d) {
    if (!d) return fail(GTA_E_BADARG, "null descriptor");
    if (d->abi_version != GTA_ABI_VERSION) return fail(GTA_E_BADARG, "abi_version mismatch");
    return GTA_OK;
}

// the (batch, head, token) strides of q, k, v, out into an argument block (GtaFwdParams, GtaGenParams, GtaBwdParams)
template <class P> void copy_strides(P& p, const GtaAttnDesc* d) {
    p.q_sb = d->q_stride[0]; p.q_sh = d->q_stride[1]; p.q_st = d->q_stride[2];
    p.k_sb = d->k_stride[0]; p.k_sh = d->k_stride[1]; p.k_st = d->k_stride[2];
    p.v_sb = d->v_stride[0]; p.v_sh = d->v_stride[1]; p.v_st = d->v_stride[2];
    p.o_sb = d->o_stride[0]; p.o_sh = d->o_stride[1]; p.o_st = d->o_stride[2];
}

// the two slab rules every entry words alike: sizes >= 0 that sum to dh (the group-size rules differ between the entries and stay with them)
int check_slabs(const GtaAttnDesc* d) {
    if (d->d_triv < 0 || d->d_se3 < 0 || d->d_so3 < 0 || d->d_so2 < 0 || d->d_t2 < 0) return fail(GTA_E_LAYOUT, "negative slab size");
    if (d->d_triv + d->d_se3 + d->d_so3 + d->d_so2 + d->d_t2 != d->dh) return fail(GTA_E_LAYOUT, "f_dims do not sum to dh");
    return GTA_OK;
}

// Build the per-chunk descriptors for the fused kernels, or say why this layout needs the
// generic (unfused) path.
int build_ctab(const GtaAttnDesc* d, uint32_t* ctab) {
    if (int rc = check_slabs(d)) return rc;
    if (d->flags & GTA_FLAG_EUCLID) {
        if (d->d_se3 % 3) return fail(GTA_E_LAYOUT, "under euclid_sim the se3 slab holds 3-vectors (gta.py:147)");
        return fail(GTA_E_UNSUPPORTED, "euclid similarity has no fused kernel (gta_rep_apply + gta_attn_fwd_plain)");
    }
    if (d->d_se3 % 4) return fail(GTA_E_LAYOUT, "se3 slab must be a multiple of 4 channels (gta.py:161)");
    if (d->d_so2 % 4) return fail(GTA_E_LAYOUT, "so2 slab must be 4*nfreqs channels (gta.py:212-214)");
    if (d->d_t2 % 3) return fail(GTA_E_LAYOUT, "t2 slab must be a multiple of 3 channels (gta.py:231)");
    if (d->d_so3 > 0) {
        int tot = 0;
        for (int l = 1; l <= d->so3_degree; ++l) tot += 2 * l + 1;
        if (d->so3_degree < 1 || d->d_so3 % tot) return fail(GTA_E_LAYOUT, "so3 slab must be r*sum(2l+1) channels (gta.py:182)");
    }
    if (d->dh % 8 || d->dh > 128) return fail(GTA_E_UNSUPPORTED, "fused kernel needs dh % 8 == 0 and dh <= 128");
    if (d->d_t2 > 0) return fail(GTA_E_UNSUPPORTED, "t2 slab has no fused kernel (ablation; use the unfused path)");
    if (d->d_so3 > 0 && (d->so3_degree != 2 || d->d_so3 % 8))
        return fail(GTA_E_UNSUPPORTED, "fused so3 needs degree 2 ([3|5] groups of 8 channels)");
    const int s_se3 = d->d_triv, s_so3 = s_se3 + d->d_se3, s_so2 = s_so3 + d->d_so3;
    if (s_se3 % 4 || (d->d_so3 > 0 && s_so3 % 8) || s_so2 % 4)
        return fail(GTA_E_UNSUPPORTED, "fused kernel needs 4-aligned se3/so2 slabs and an 8-aligned so3 slab");
    for (int c = 0; c < 16; ++c) ctab[c] = 0;
    for (int c = 0; c < d->dh / 8; ++c) {
        uint32_t desc = 0;
        const int lo = 8 * c, hi = 8 * c + 4;
        if (d->d_so3 > 0 && lo >= s_so3 && lo < s_so2) { ctab[c] = CHUNK_SO3; continue; }
        for (int half = 0; half < 2; ++half) {
            const int ch = half ? hi : lo;
            uint32_t kind = HALF_ID, blk = 0;
            if (ch >= s_se3 && ch < s_so3) kind = HALF_SE3;
            else if (ch >= s_so2 && ch < s_so2 + d->d_so2) { kind = HALF_SO2; blk = (uint32_t)(ch - s_so2) / 2; }
            desc |= kind << (2 * half);
            desc |= blk << (8 + 8 * half);
        }
        ctab[c] = desc;
    }
    return GTA_OK;
}

int check_common(const GtaAttnDesc* d) {
    if (int rc = check_header(d)) return rc;
    if (d->dtype != GTA_DTYPE_F32 && d->dtype != GTA_DTYPE_BF16) return fail(GTA_E_BADARG, "bad dtype");
    if (d->B <= 0 || d->H <= 0 || d->Tq <= 0 || d->Tk <= 0 || d->dh <= 0) return fail(GTA_E_BADARG, "non-positive size");
    if (d->Nq <= 0 || d->Nk <= 0 || d->Tq % d->Nq || d->Tk % d->Nk)
        return fail(GTA_E_BADARG, "tokens must split evenly into views (gta.py:160-162)");
    if (d->Nq > GTA_MAX_VIEWS || d->Nk > GTA_MAX_VIEWS) return fail(GTA_E_UNSUPPORTED, "more than GTA_MAX_VIEWS views per side");
    if (d->Tq >= (1 << 22) || d->Tk >= (1 << 22)) return fail(GTA_E_UNSUPPORTED, "more than 2^22 tokens per side");
    const int esz = esz_of(d);
    const int64_t* st[4] = {d->q_stride, d->k_stride, d->v_stride, d->o_stride};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j)
            if ((st[i][j] * esz) % 16) return fail(GTA_E_BADARG, "strides must keep every head row 16-byte aligned");
    return GTA_OK;
}

// The fused forward's argument block for d and the operands of a call (null where the call has none).  A workspace holds the two-stage
// plan's K'/V' tile images, per-tile key norms and (bf16 at dh = 96 with view reps) q-side rep tiles; the single-kernel plan reads none of them.
int fwd_params(GtaFwdParams& p, const GtaAttnDesc* d, const void* q, const void* k, const void* v, const float* vrep_q, const float* vrep_k,
               const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau, void* out, float* lse, void* workspace) {
    memset(&p, 0, sizeof p);
    if (int rc = build_ctab(d, p.ctab)) return rc;
    const bool need_view = d->d_se3 > 0 || d->d_so3 > 0, need_cs = d->d_so2 > 0;
    p.q = q; p.k = k; p.v = v; p.o = out; p.lse = lse;
    p.vrep_q = need_view ? vrep_q : nullptr; p.vrep_k = need_view ? vrep_k : nullptr;
    p.cs_q = need_cs ? cs_q : nullptr; p.cs_k = need_cs ? cs_k : nullptr;
    p.trans_coeff = trans_coeff; p.tau = tau;
    copy_strides(p, d);
    p.B = d->B; p.H = d->H; p.Tq = d->Tq; p.Tk = d->Tk; p.Nq = d->Nq; p.Nk = d->Nk;
    p.Pq = d->Tq / d->Nq; p.Pk = d->Tk / d->Nk;
    p.invPq = 1.0f / (float)p.Pq; p.invPk = 1.0f / (float)p.Pk;
    p.dh = d->dh; p.nso2 = d->d_so2 / 2;
    p.n_qtiles = (d->Tq + 127) / 128;
    p.flags = d->flags; p.scale = d->scale;
    if (workspace) {
        const int dhp = padded_dh(d->dh);
        p.kp = workspace;
        p.kn = (float*)((char*)workspace + ((gta_fwd2_image_bytes(d->B, d->H, d->Tk, dhp, (d->flags & GTA_FLAG_FP32_PRODUCTS) != 0) + 255) & ~255L));
        if (dhp == 96 && d->dtype == GTA_DTYPE_BF16 && need_view) p.qtiles = (char*)workspace + gta_fwd2_qtiles_offset(d->B, d->H, d->Tk, 96, false);
    }
    return GTA_OK;
}

// the forward instance of a full call with LSE and a workspace, for a supported d: every operand at one placeholder address (the selection
// reads only whether a pointer is null and how it is aligned)
GtaFwdSel full_call_selection(const GtaAttnDesc* d) {
    float* const x = (float*)256;
    GtaFwdParams p;
    fwd_params(p, d, x, x, x, x, x, x, x, x, x, x, x, x);
    return gta_fwd_select(p, padded_dh(d->dh), esz_of(d));
}

}  // namespace

// debug hook (not part of the product ABI): device buffer [capacity_items][8] for the per-item s_memtime stamps of the NEXT attention
// launch this thread makes through gta_attn_fwd -- thread-local and one-shot, like gta_debug_time_next_attention_kernel, and dropped
// (no stamps) when the launch has more work items than the buffer holds
static thread_local unsigned long long* t_prof = nullptr;
static thread_local int64_t t_prof_items = 0;
extern "C" void gta_debug_profile_next_attention_kernel(void* p, int64_t capacity_items) {
    t_prof = (unsigned long long*)p;
    t_prof_items = p ? capacity_items : 0;
}
extern "C" int gta_abi_version(void) { return GTA_ABI_VERSION; }
extern "C" int gta_sizeof_attn_desc(void) { return (int)sizeof(GtaAttnDesc); }

extern "C" const char* gta_strerror(int code) {
    static thread_local char buf[256];
    const char* base = "unknown";
    switch (code) {
        case GTA_OK: return "ok";
        case GTA_E_BADARG: base = "bad argument"; break;
        case GTA_E_LAYOUT: base = "inconsistent f_dims layout"; break;
        case GTA_E_UNSUPPORTED: base = "unsupported by this build"; break;
        case GTA_E_LAUNCH: base = "HIP launch failed"; break;
        case GTA_E_NODEVICE: base = "no HIP device"; break;
    }
    snprintf(buf, sizeof buf, "%s: %s", base, g_detail);
    return buf;
}

extern "C" int gta_attn_fwd_supported(const GtaAttnDesc* desc) {
    if (int rc = check_header(desc)) return rc;
    uint32_t ctab[16];
    if (int rc = build_ctab(desc, ctab)) return rc;      // layout first: "no fused kernel" must not be masked by a stride complaint
    return check_common(desc);
}

extern "C" int64_t gta_attn_fwd_workspace_bytes(const GtaAttnDesc* desc) {
    if (gta_attn_fwd_supported(desc)) return 0;
    const bool x3 = (desc->flags & GTA_FLAG_FP32_PRODUCTS) != 0;
    if (x3 && full_call_selection(desc).kind == GTA_FWD_SINGLE) return 0;       // (that mode runs the single-kernel plan here)
    return gta_fwd2_workspace_bytes(desc->B, desc->H, desc->Tk, padded_dh(desc->dh), desc->Nq, esz_of(desc), x3);
}

extern "C" int gta_attn_fwd_launch_info(const GtaAttnDesc* desc, int32_t* lds_bytes, int32_t* n_workgroups,
                                        int32_t* threads_per_wg) {
    int rc = gta_attn_fwd_supported(desc);
    if (rc) return rc;
    if (lds_bytes) *lds_bytes = gta_fwd_lds_bytes(padded_dh(desc->dh), esz_of(desc));
    if (n_workgroups) *n_workgroups = desc->B * desc->H * ((desc->Tq + 127) / 128);
    if (threads_per_wg) *threads_per_wg = 256;
    return GTA_OK;
}

// which attention kernel gta_attn_fwd launches for desc when given a workspace (diagnostic; the names are the kernels' own)
extern "C" const char* gta_debug_attention_kernel(const GtaAttnDesc* d, int32_t* n_items, int32_t* rows_per_item) {
    if (gta_attn_fwd_supported(d)) return "";
    const GtaFwdSel s = full_call_selection(d);
    if (n_items) *n_items = d->B * d->H * ((d->Tq + s.rows - 1) / s.rows);
    if (rows_per_item) *rows_per_item = s.rows;
    return s.name;
}

namespace {
// what per-scene key prefixes (gta_attn_fwd_varlen, gta_attn_bwd_varlen) cannot be combined with
int varlen_flags(const GtaAttnDesc* d) {
    if (d->flags & GTA_FLAG_FUSED_KV) return fail(GTA_E_UNSUPPORTED, "per-scene key prefixes run the two-stage plan: no GTA_FLAG_FUSED_KV");
    if (d->flags & GTA_FLAG_FP32_PRODUCTS) return fail(GTA_E_UNSUPPORTED, "per-scene key prefixes have no GTA_FLAG_FP32_PRODUCTS instances");
    if (d->flags & GTA_FLAG_PRETRANSFORMED) return fail(GTA_E_UNSUPPORTED, "per-scene key prefixes apply rho_k in the pre-pass: no GTA_FLAG_PRETRANSFORMED");
    return GTA_OK;
}

// the fused forward entries.  varlen (gta_attn_fwd_varlen) is the explicit selector of per-scene key prefixes -- never "key_lens is non-null":
// always the two-stage plan, with the VARLEN instances of the pre-pass and of gta_fwd2_kernel (GtaFwdSel::varlen selects them in
// gta_fwd2_dispatch), whatever attention kernel gta_fwd_select would give the shape.  gather (gta_attn_fwd_gather; with varlen) is the explicit selector
// of the GATHER instances of the pre-pass -- never "key_idx is non-null": the keys are the tokens key_idx names, key_lens counts them, and the
// attention step is the VARLEN gta_fwd2_kernel under the same key_lens.  With GTA_FLAG_KV_READY the indices are not read.
int fwd_call(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
             const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
             const float* trans_coeff, const float* tau, bool varlen, const int32_t* key_lens, bool gather, const int32_t* key_idx,
             bool qmask, const uint8_t* q_live, void* out, float* lse, void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_common(d);
    if (rc) return rc;
    if (!k || !v || ((!q || !out) && !(d->flags & GTA_FLAG_PREP_ONLY))) return fail(GTA_E_BADARG, "null q/k/v/out");
    if (qmask && !(varlen && gather)) return fail(GTA_E_BADARG, "the query mask comes with the gather");
    if (varlen) {
        if (!key_lens) return fail(GTA_E_BADARG, "null key_lens");
        if (gather && !key_idx && !(d->flags & GTA_FLAG_KV_READY)) return fail(GTA_E_BADARG, "null key_idx");
        if (qmask && !q_live) return fail(GTA_E_BADARG, "null q_live");
        if (!workspace) return fail(GTA_E_BADARG, "per-scene key prefixes need the workspace of gta_attn_fwd_workspace_bytes()");
    }
    GtaFwdParams p;
    rc = fwd_params(p, d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, out, lse, workspace);
    if (rc) return rc;
    if (varlen && (rc = varlen_flags(d))) return rc;
    const bool pre = (d->flags & GTA_FLAG_PRETRANSFORMED) != 0;
    if ((d->d_se3 > 0 || d->d_so3 > 0) && (!vrep_q || (!pre && !vrep_k))) return fail(GTA_E_BADARG, "se3/so3 slabs need vrep_q and vrep_k");
    if (d->d_so2 > 0 && (!cs_q || (!pre && !cs_k))) return fail(GTA_E_BADARG, "so2 slab needs cs_q and cs_k");
    const int dhp = padded_dh(d->dh), esz = esz_of(d);
#ifdef GTA_ABLATE
    if (!varlen) { const char* e = getenv("GTA_DBG"); p.dbg = e ? (uint32_t)atoi(e) : 0u; }
#endif
    GtaFwdSel s = gta_fwd_select(p, dhp, esz);
    if (varlen) {       // (the selection gave the layout of the chunk table; the kernel is fixed)
        s.kind = GTA_FWD_FWD2; s.coal = false; s.qtiles = false; s.rows = 128; s.name = "gta_fwd2_kernel"; s.varlen = true;
        p.key_lens = key_lens;
        if (gather) { s.gather = true; s.key_idx = (d->flags & GTA_FLAG_KV_READY) ? nullptr : key_idx; }
        if (qmask) { s.qmask = true; s.q_live = q_live; }      // (the QMASK twins of the VARLEN attention kernel)
    } else if (t_prof && !(d->flags & GTA_FLAG_PREP_ONLY)) {      // (start / end stamps of every work item: gta_debug_profile_next_attention_kernel)
        if ((int64_t)d->B * d->H * ((d->Tq + s.rows - 1) / s.rows) <= t_prof_items) p.prof = t_prof;
        t_prof = nullptr;
        t_prof_items = 0;
    }
    const long n_wg = (long)d->B * d->H * p.n_qtiles;
    if (n_wg > 0x7fffffffL) return fail(GTA_E_UNSUPPORTED, "grid too large");
    if ((d->flags & GTA_FLAG_FP32_PRODUCTS) && d->dtype != GTA_DTYPE_F32)
        return fail(GTA_E_BADARG, "GTA_FLAG_FP32_PRODUCTS is for fp32 inputs (bf16 inputs ask for bf16 arithmetic)");
    if (s.kind == GTA_FWD_SINGLE)
        return launch_status(gta_fwd_dispatch(p, dhp, esz, !(d->flags & GTA_FLAG_NO_DMA), (int)n_wg, (hipStream_t)stream), "no kernel instance");
    if (workspace_bytes < gta_fwd2_workspace_bytes(d->B, d->H, d->Tk, dhp, d->Nq, esz, (d->flags & GTA_FLAG_FP32_PRODUCTS) != 0))
        return fail(GTA_E_BADARG, "workspace smaller than gta_attn_fwd_workspace_bytes()");
    if (d->H > 65535 || d->B > 65535) return fail(GTA_E_UNSUPPORTED, "B or H above 65535");
    return launch_status(gta_fwd2_dispatch(p, s, dhp, esz, !(d->flags & GTA_FLAG_KV_READY), !(d->flags & GTA_FLAG_PREP_ONLY), (hipStream_t)stream),
                         "no kernel instance");
}
}  // namespace

extern "C" int gta_attn_fwd(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                            const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                            const float* trans_coeff, const float* tau, void* out, float* lse,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    return fwd_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, false, nullptr, false, nullptr, false, nullptr, out, lse, workspace, workspace_bytes, stream);
}

extern "C" int gta_attn_fwd_varlen_supported(const GtaAttnDesc* desc) {
    if (int rc = gta_attn_fwd_supported(desc)) return rc;
    return varlen_flags(desc);
}

extern "C" int gta_attn_fwd_varlen(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                   const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                                   const float* trans_coeff, const float* tau, const int32_t* key_lens, void* out, float* lse,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    return fwd_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, false, nullptr, false, nullptr, out, lse, workspace, workspace_bytes, stream);
}

// Any per-scene subset of the key tokens: the rules and the workspace of gta_attn_fwd_varlen, the GATHER instances of the pre-pass
extern "C" int gta_attn_fwd_gather_supported(const GtaAttnDesc* desc) { return gta_attn_fwd_varlen_supported(desc); }

extern "C" int gta_attn_fwd_gather(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                   const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                                   const float* trans_coeff, const float* tau, const int32_t* key_idx, const int32_t* key_lens, void* out, float* lse,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    return fwd_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, true, key_idx, false, nullptr, out, lse, workspace, workspace_bytes, stream);
}

// gta_attn_fwd_gather under a query-side mask: the QMASK twins of the VARLEN gta_fwd2_kernel (dead rows: never used, out and lse +0.0)
extern "C" int gta_attn_fwd_qmask_supported(const GtaAttnDesc* desc) { return gta_attn_fwd_gather_supported(desc); }

extern "C" int gta_attn_fwd_qmask(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                  const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                                  const float* trans_coeff, const float* tau, const int32_t* key_idx, const int32_t* key_lens,
                                  const uint8_t* q_live, void* out, float* lse,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (d && (d->flags & GTA_FLAG_PREP_ONLY)) return fail(GTA_E_BADARG, "gta_attn_fwd_qmask runs the attention step: no GTA_FLAG_PREP_ONLY (gta_attn_fwd_gather builds the images)");
    return fwd_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, true, key_idx, true, q_live, out, lse, workspace, workspace_bytes, stream);
}


// ---------------------------------------------------------------------------------------------
// staged generic forward (gta_fwd_gen.hip): the two-stage plan for any f_dims layout
// ---------------------------------------------------------------------------------------------
namespace {
// the layout rules of the generic path (gta_rep_apply), then what the staged kernels add
int staged_layout(const GtaAttnDesc* d) {
    if (int rc = check_slabs(d)) return rc;
    const bool euclid = (d->flags & GTA_FLAG_EUCLID) != 0;
    if (euclid && d->d_se3 % 3) return fail(GTA_E_LAYOUT, "under euclid_sim the se3 slab holds 3-vectors (gta.py:147)");
    if (!euclid && d->d_se3 % 4) return fail(GTA_E_LAYOUT, "se3 slab must be a multiple of 4 channels (gta.py:161)");
    if (d->d_so2 % 2) return fail(GTA_E_LAYOUT, "so2 slab must be a whole number of 2-channel blocks");
    if (d->d_t2 % 3) return fail(GTA_E_LAYOUT, "t2 slab must be a multiple of 3 channels (gta.py:231)");
    if (d->d_so3 > 0 && (d->so3_degree < 1 || d->so3_degree > 2)) return fail(GTA_E_UNSUPPORTED, "so3 of degree 1 or 2");
    if (d->d_so3 > 0 && d->d_so3 % (d->so3_degree == 2 ? 8 : 3)) return fail(GTA_E_LAYOUT, "so3 slab must be r*sum(2l+1) channels (gta.py:182)");
    if (d->dh % 8) return fail(GTA_E_UNSUPPORTED, "staged generic forward needs dh % 8 == 0 (gta_rep_apply + gta_attn_fwd_plain on padded channels)");
    if (d->dh > 128) return fail(GTA_E_UNSUPPORTED, "staged generic forward needs dh <= 128");
    if (d->flags & GTA_FLAG_FP32_PRODUCTS) return fail(GTA_E_UNSUPPORTED, "staged generic forward has no GTA_FLAG_FP32_PRODUCTS instances (gta_rep_apply + gta_attn_fwd_plain)");
    if (d->flags & GTA_FLAG_PRETRANSFORMED) return fail(GTA_E_UNSUPPORTED, "staged generic forward applies rho itself: no GTA_FLAG_PRETRANSFORMED");
    return GTA_OK;
}
}  // namespace

extern "C" int gta_attn_fwd_staged_supported(const GtaAttnDesc* desc) {
    if (int rc = check_header(desc)) return rc;
    if (int rc = staged_layout(desc)) return rc;      // layout first, as gta_attn_fwd_supported
    return check_common(desc);
}

extern "C" int64_t gta_attn_fwd_staged_workspace_bytes(const GtaAttnDesc* desc) {
    if (gta_attn_fwd_staged_supported(desc)) return 0;
    return gta_gen_workspace_bytes(desc->B, desc->H, desc->Tk, padded_dh(desc->dh));
}

namespace {
// the staged entries: key_lens == nullptr is gta_attn_fwd_staged.  gather (gta_attn_fwd_staged_gather; with key_lens) is the explicit selector of
// the GATHER instances of the pre-pass -- never "key_idx is non-null"; with GTA_FLAG_KV_READY the indices are not read.
int staged_call(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau, const int32_t* key_lens,
                bool gather, const int32_t* key_idx, void* out, float* lse, void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_common(d);
    if (rc) return rc;
    if (!k || !v || ((!q || !out) && !(d->flags & GTA_FLAG_PREP_ONLY))) return fail(GTA_E_BADARG, "null q/k/v/out");
    if (gather && !key_idx && !(d->flags & GTA_FLAG_KV_READY)) return fail(GTA_E_BADARG, "null key_idx");
    if ((rc = staged_layout(d))) return rc;
    if ((d->d_se3 > 0 || d->d_so3 > 0) && (!vrep_q || !vrep_k)) return fail(GTA_E_BADARG, "se3/so3 slabs need vrep_q and vrep_k");
    if (d->d_so2 > 0 && (!cs_q || !cs_k)) return fail(GTA_E_BADARG, "so2 slab needs cs_q and cs_k");
    if (d->d_t2 > 0 && (!coord_q || !coord_k)) return fail(GTA_E_BADARG, "t2 slab needs coord_q and coord_k");
    const int dhp = padded_dh(d->dh);
    if (!workspace || workspace_bytes < gta_gen_workspace_bytes(d->B, d->H, d->Tk, dhp))
        return fail(GTA_E_BADARG, "workspace smaller than gta_attn_fwd_staged_workspace_bytes()");
    if ((uintptr_t)workspace % 256) return fail(GTA_E_BADARG, "workspace must be 256-byte aligned");
    GtaGenParams p;
    memset(&p, 0, sizeof p);
    p.q = q; p.k = k; p.v = v; p.o = out; p.lse = lse;
    p.img = workspace;
    if (d->flags & GTA_FLAG_EUCLID) p.kbias = (float*)((char*)workspace + ((gta_gen_image_bytes(d->B, d->H, d->Tk, dhp) + 255) & ~255L));
    p.vrep_q = vrep_q; p.vrep_k = vrep_k; p.cs_q = cs_q; p.cs_k = cs_k; p.coord_q = coord_q; p.coord_k = coord_k;
    p.trans_coeff = trans_coeff; p.tau = tau;
    copy_strides(p, d);
    p.B = d->B; p.H = d->H; p.Tq = d->Tq; p.Tk = d->Tk; p.Nq = d->Nq; p.Nk = d->Nk;
    p.dh = d->dh; p.d_triv = d->d_triv; p.d_se3 = d->d_se3; p.d_so3 = d->d_so3; p.d_so2 = d->d_so2; p.d_t2 = d->d_t2; p.L = d->so3_degree;
    p.euclid = (d->flags & GTA_FLAG_EUCLID) ? 1 : 0;
    p.xv = (d->flags & GTA_FLAG_V_TRANSFORM) ? 1 : 0;
    p.esz = esz_of(d);
    p.n_qtiles = (d->Tq + 127) / 128;
    p.n_tiles = (d->Tk + 63) / 64;
    const long n_items = (long)d->B * d->H * p.n_qtiles;
    if (n_items > 0x7fffffffL) return fail(GTA_E_UNSUPPORTED, "grid too large");
    p.n_items = (int)n_items;
    p.scale = d->scale;
    p.key_lens = key_lens;
    const bool run_prep = !(d->flags & GTA_FLAG_KV_READY), run_attn = !(d->flags & GTA_FLAG_PREP_ONLY);
    rc = gather ? gta_gen_gather_dispatch(p, run_prep ? key_idx : nullptr, dhp, run_prep, run_attn, stream) : gta_gen_dispatch(p, dhp, run_prep, run_attn, stream);
    if (rc) return fail(rc, gta_gen_error());       // (the launchers read HIP's error, which clears it: they keep its text)
    return GTA_OK;
}
}  // namespace

extern "C" int gta_attn_fwd_staged(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                   const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                                   const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau,
                                   void* out, float* lse, void* workspace, int64_t workspace_bytes, void* stream) {
    return staged_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, coord_q, coord_k, trans_coeff, tau, nullptr, false, nullptr, out, lse, workspace, workspace_bytes, stream);
}

extern "C" int gta_attn_fwd_staged_varlen_supported(const GtaAttnDesc* desc) { return gta_attn_fwd_staged_supported(desc); }

extern "C" int gta_attn_fwd_staged_varlen(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                          const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                                          const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau,
                                          const int32_t* key_lens, void* out, float* lse, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!key_lens) return fail(GTA_E_BADARG, "null key_lens");
    return staged_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, coord_q, coord_k, trans_coeff, tau, key_lens, false, nullptr, out, lse, workspace, workspace_bytes, stream);
}

// Any per-scene subset of the key tokens on the staged layouts: gta_attn_fwd_staged_varlen with the GATHER instances of gta_gen_prep_kernel
extern "C" int gta_attn_fwd_staged_gather_supported(const GtaAttnDesc* desc) { return gta_attn_fwd_staged_supported(desc); }

extern "C" int gta_attn_fwd_staged_gather(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                          const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                                          const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau,
                                          const int32_t* key_idx, const int32_t* key_lens, void* out, float* lse,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
    if (!key_lens) return fail(GTA_E_BADARG, "null key_lens");
    return staged_call(d, q, k, v, vrep_q, vrep_k, cs_q, cs_k, coord_q, coord_k, trans_coeff, tau, key_lens, true, key_idx, out, lse, workspace, workspace_bytes, stream);
}


// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
namespace {
struct BwdLayout { int64_t off_qimg, off_stats, off_dc, off_dt, off_kv, total; int n_prep, n_dq, n_dkv; };
BwdLayout bwd_layout(const GtaAttnDesc* d) {
    BwdLayout L;
    const int dhp = padded_dh(d->dh);
    const int64_t n_qt = (d->Tq + 63) / 64, n_kt = (d->Tk + 63) / 64;
    // (the fp32-faithful backward, r06: four images per tile -- hi and lo -- on both sides)
    const int64_t stage = ((d->flags & GTA_FLAG_FP32_PRODUCTS) ? 4LL : 2LL) * 64 * dhp * 2;
    L.n_prep = (int)(d->B * d->H * n_qt);
    L.n_dq = d->B * d->H * ((d->Tq + 127) / 128);
    L.n_dkv = d->B * d->H * ((d->Tk + 127) / 128);
    auto al = [](int64_t x) { return (x + 255) & ~255LL; };
    L.off_qimg = 0;
    L.off_stats = al(L.off_qimg + (int64_t)d->B * d->H * n_qt * stage);
    L.off_dc = al(L.off_stats + (int64_t)d->B * d->H * n_qt * 128 * 4);
    L.off_dt = al(L.off_dc + (int64_t)(L.n_prep + L.n_dq + L.n_dkv) * 4);
    L.off_kv = al(L.off_dt + (int64_t)L.n_dq * 4);
    L.total = al(L.off_kv + (int64_t)d->B * d->H * n_kt * stage);
    return L;
}
}  // namespace

extern "C" int64_t gta_attn_bwd_workspace_bytes(const GtaAttnDesc* desc) {
    if (gta_attn_fwd_supported(desc)) return 0;
    return bwd_layout(desc).total;
}

namespace {
// what no backward entry serves, whatever the layout (gta_attn_bwd_dlse_supported asks before a launch; bwd_call at one)
int bwd_flags(const GtaAttnDesc* d) {
    if (d->flags & GTA_FLAG_PRETRANSFORMED) return fail(GTA_E_UNSUPPORTED, "backward of the pretransformed mode");
    if ((d->flags & GTA_FLAG_FP32_PRODUCTS) && !gta_x3_takes(padded_dh(d->dh), esz_of(d)))
        return fail(GTA_E_UNSUPPORTED, "GTA_FLAG_FP32_PRODUCTS backward: fp32 inputs at dh <= 64 (other sizes: gta_rep_apply + gta_attn_bwd_plain_f32)");
    return GTA_OK;
}

// the four backward entries.  varlen (gta_attn_bwd_varlen) is the explicit selector of the VARLEN instances -- never "key_lens is non-null";
// gather (gta_attn_bwd_gather; with varlen, q_lens null) that of the GATHER dK/dV walk -- never "key_idx is non-null"; with_dlse
// (gta_attn_bwd_dlse) likewise selects the instances that read dlse; qmask (gta_attn_bwd_qmask; with gather, q_lens allowed) the QMASK instances
// of the q-side pre-pass and of the dQ walk
int bwd_call(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
             const void* dout, const float* lse, const float* vrep_q, const float* vrep_k,
             const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
             bool varlen, const int32_t* key_lens, const int32_t* q_lens, bool gather, const int32_t* key_idx, bool qmask, const uint8_t* q_live,
             bool with_dlse, const float* dlse, const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
             const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
             int64_t workspace_bytes, void* stream) {
    int rc = check_common(d);
    if (rc) return rc;
    if (varlen) {
        if (!key_lens) return fail(GTA_E_BADARG, "null key_lens");
        if (gather && !key_idx) return fail(GTA_E_BADARG, "null key_idx (the backward scatters dk / dv through it, with kv_images too)");
        if (qmask && !gather) return fail(GTA_E_BADARG, "the query mask comes with the gather");
        if (qmask && !q_live) return fail(GTA_E_BADARG, "null q_live");
        if ((rc = varlen_flags(d))) return rc;
    } else if (gather || qmask) {
        return fail(GTA_E_BADARG, "the gather comes with per-scene key counts");
    }
    if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv || !dqkv_stride || !dout_stride || !workspace)
        return fail(GTA_E_BADARG, "null argument");
    if (with_dlse && !dlse) return fail(GTA_E_BADARG, "null dlse");
    if ((rc = bwd_flags(d))) return rc;
    const int dhp = padded_dh(d->dh), esz = esz_of(d);
    GtaBwdParams p;
    memset(&p, 0, sizeof p);
    rc = build_ctab(d, p.ctab);
    if (rc) return rc;
    const bool need_view = d->d_se3 > 0 || d->d_so3 > 0, need_cs = d->d_so2 > 0;
    if (need_view && (!vrep_q || !vrep_k)) return fail(GTA_E_BADARG, "se3/so3 slabs need vrep_q and vrep_k");
    if (need_cs && (!cs_q || !cs_k)) return fail(GTA_E_BADARG, "so2 slab needs cs_q and cs_k");
    for (int i = 0; i < 9; ++i) if ((dqkv_stride[i] * esz) % 16) return fail(GTA_E_BADARG, "gradient strides must keep rows 16-byte aligned");
    for (int i = 0; i < 3; ++i) if ((dout_stride[i] * esz) % 16) return fail(GTA_E_BADARG, "dout strides must keep rows 16-byte aligned");
    const BwdLayout L = bwd_layout(d);
    if (workspace_bytes < L.total) return fail(GTA_E_BADARG, "workspace smaller than gta_attn_bwd_workspace_bytes()");
    char* ws = (char*)workspace;
    if (!kv_images) {     // recompute K'/V' images with the forward's pre-pass (GTA_FLAG_FP32_PRODUCTS: hi and lo images, as the X3 walks read them)
        GtaFwdParams f;
        fwd_params(f, d, nullptr, k, v, nullptr, vrep_k, nullptr, cs_k, trans_coeff, nullptr, nullptr, nullptr, nullptr);
        f.kp = ws + L.off_kv;
        GtaFwdSel s = gta_fwd_select(f, dhp, esz);
        if (varlen) {                      // the VARLEN instance of the pre-pass: the images of gta_attn_fwd_varlen under the same key_lens
            s.varlen = true;
            f.key_lens = key_lens;
            if (gather) { s.gather = true; s.key_idx = key_idx; }      // (the GATHER instance: the images of gta_attn_fwd_gather under the same index)
        }
        rc = gta_fwd2_dispatch(f, s, dhp, esz, true, false, (hipStream_t)stream);
        if (rc) return fail(rc, "K/V pre-pass launch failed");
        kv_images = ws + L.off_kv;
    }
    p.q = q; p.k = k; p.v = v; p.out = out; p.dout = dout; p.lse = lse; p.dq = dq; p.dk = dk; p.dv = dv;
    p.vrep_q = need_view ? vrep_q : nullptr; p.vrep_k = need_view ? vrep_k : nullptr;
    p.cs_q = need_cs ? cs_q : nullptr; p.cs_k = need_cs ? cs_k : nullptr;
    p.trans_coeff = trans_coeff; p.tau = tau;
    p.kvimg = kv_images; p.qimg = ws + L.off_qimg; p.stats = (float*)(ws + L.off_stats);
    p.dc_partial = (float*)(ws + L.off_dc); p.dtrans_coeff = (d->d_se3 > 0) ? dtrans_coeff : nullptr;
    p.dt_partial = (tau && dtau) ? (float*)(ws + L.off_dt) : nullptr; p.dtau = (tau && dtau) ? dtau : nullptr;
    copy_strides(p, d);
    p.do_sb = dout_stride[0]; p.do_sh = dout_stride[1]; p.do_st = dout_stride[2];
    p.dq_sb = dqkv_stride[0]; p.dq_sh = dqkv_stride[1]; p.dq_st = dqkv_stride[2];
    p.dk_sb = dqkv_stride[3]; p.dk_sh = dqkv_stride[4]; p.dk_st = dqkv_stride[5];
    p.dv_sb = dqkv_stride[6]; p.dv_sh = dqkv_stride[7]; p.dv_st = dqkv_stride[8];
    p.dc_off_prep = 0; p.dc_off_dq = L.n_prep; p.dc_off_dkv = L.n_prep + L.n_dq; p.dc_total = L.n_prep + L.n_dq + L.n_dkv;
    p.B = d->B; p.H = d->H; p.Tq = d->Tq; p.Tk = d->Tk; p.Nq = d->Nq; p.Nk = d->Nk;
    p.Pq = d->Tq / d->Nq; p.Pk = d->Tk / d->Nk; p.invPq = 1.0f / (float)p.Pq; p.invPk = 1.0f / (float)p.Pk;
    p.dh = d->dh; p.nso2 = d->d_so2 / 2; p.flags = d->flags; p.scale = d->scale;
    if (d->H > 65535 || d->B > 65535) return fail(GTA_E_UNSUPPORTED, "B or H above 65535");
    if (!with_dlse) dlse = nullptr;
    return launch_status(qmask ? gta_bwd_qmask_dispatch(p, key_idx, key_lens, q_lens, q_live, dlse, dhp, esz, (hipStream_t)stream)
                         : gather ? gta_bwd_gather_dispatch(p, key_idx, key_lens, dlse, dhp, esz, (hipStream_t)stream)
                         : varlen ? gta_bwd_varlen_dispatch(p, key_lens, q_lens, dlse, dhp, esz, (hipStream_t)stream)
                                : gta_bwd_dispatch(p, dlse, dhp, esz, (hipStream_t)stream), "no kernel instance");
}
}  // namespace

extern "C" int gta_attn_bwd(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                            const void* dout, const float* lse, const float* vrep_q, const float* vrep_k,
                            const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                            const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                            const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                            int64_t workspace_bytes,
                            void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, false, nullptr, nullptr, false, nullptr, false, nullptr, false, nullptr, kv_images, dq, dk, dv,
                    dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

// Backward of the pair (out, lse): the DLSE instances of the q-side pre-pass (and of the X3 dQ walk's d tau), every other kernel as in gta_attn_bwd
extern "C" int gta_attn_bwd_dlse_supported(const GtaAttnDesc* desc) {
    if (int rc = gta_attn_fwd_supported(desc)) return rc;
    return bwd_flags(desc);
}

extern "C" int gta_attn_bwd_dlse(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                 const void* dout, const float* lse, const float* dlse, const float* vrep_q, const float* vrep_k,
                                 const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                 const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                 const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, false, nullptr, nullptr, false, nullptr, false, nullptr, true, dlse, kv_images, dq, dk, dv,
                    dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

// Backward with per-scene prefixes: the VARLEN instances of the compiled backward kernels (gta_bwd.hip), never the generated streams
extern "C" int gta_attn_bwd_varlen_supported(const GtaAttnDesc* desc) { return gta_attn_fwd_varlen_supported(desc); }

extern "C" int gta_attn_bwd_varlen(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                   const void* dout, const float* lse, const float* vrep_q, const float* vrep_k,
                                   const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                   const int32_t* key_lens, const int32_t* q_lens,
                                   const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                   const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, q_lens, false, nullptr, false, nullptr, false, nullptr, kv_images, dq, dk, dv,
                    dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

// Backward over any per-scene subset of the key tokens: gta_attn_bwd_varlen (no q_lens) with the GATHER instances of the dK/dV walk and, when
// the images are rebuilt, of the K/V pre-pass
extern "C" int gta_attn_bwd_gather_supported(const GtaAttnDesc* desc) { return gta_attn_bwd_varlen_supported(desc); }

extern "C" int gta_attn_bwd_gather(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                   const void* dout, const float* lse, const float* vrep_q, const float* vrep_k,
                                   const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                   const int32_t* key_idx, const int32_t* key_lens,
                                   const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                   const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, nullptr, true, key_idx, false, nullptr, false, nullptr,
                    kv_images, dq, dk, dv, dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

// gta_attn_bwd_gather under a query-side mask: the backward of gta_attn_fwd_qmask (the QMASK instances of the q-side pre-pass and of the dQ
// walk; the GATHER dK/dV walk under q_lens)
extern "C" int gta_attn_bwd_qmask_supported(const GtaAttnDesc* desc) { return gta_attn_bwd_gather_supported(desc); }

extern "C" int gta_attn_bwd_qmask(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                  const void* dout, const float* lse, const float* vrep_q, const float* vrep_k,
                                  const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                  const int32_t* key_idx, const int32_t* key_lens, const uint8_t* q_live, const int32_t* q_lens,
                                  const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                  const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, q_lens, true, key_idx, true, q_live, false, nullptr,
                    kv_images, dq, dk, dv, dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

// The masked backwards of the pair (out, lse): each base entry with dlse behind lse, as gta_attn_bwd_dlse relates to gta_attn_bwd -- the DLSE
// twin of the entry's q-side pre-pass, every walk as in the base entry.  A dead row's dlse is never read
extern "C" int gta_attn_bwd_varlen_dlse_supported(const GtaAttnDesc* desc) { return gta_attn_bwd_varlen_supported(desc); }

extern "C" int gta_attn_bwd_varlen_dlse(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                        const void* dout, const float* lse, const float* dlse, const float* vrep_q, const float* vrep_k,
                                        const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                        const int32_t* key_lens, const int32_t* q_lens,
                                        const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                        const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, q_lens, false, nullptr, false, nullptr, true, dlse, kv_images, dq, dk, dv,
                    dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

extern "C" int gta_attn_bwd_gather_dlse_supported(const GtaAttnDesc* desc) { return gta_attn_bwd_gather_supported(desc); }

extern "C" int gta_attn_bwd_gather_dlse(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                        const void* dout, const float* lse, const float* dlse, const float* vrep_q, const float* vrep_k,
                                        const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                        const int32_t* key_idx, const int32_t* key_lens,
                                        const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                        const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, nullptr, true, key_idx, false, nullptr, true, dlse,
                    kv_images, dq, dk, dv, dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

extern "C" int gta_attn_bwd_qmask_dlse_supported(const GtaAttnDesc* desc) { return gta_attn_bwd_qmask_supported(desc); }

extern "C" int gta_attn_bwd_qmask_dlse(const GtaAttnDesc* d, const void* q, const void* k, const void* v, const void* out,
                                       const void* dout, const float* lse, const float* dlse, const float* vrep_q, const float* vrep_k,
                                       const float* cs_q, const float* cs_k, const float* trans_coeff, const float* tau,
                                       const int32_t* key_idx, const int32_t* key_lens, const uint8_t* q_live, const int32_t* q_lens,
                                       const void* kv_images, void* dq, void* dk, void* dv, const int64_t* dqkv_stride,
                                       const int64_t* dout_stride, float* dtrans_coeff, float* dtau, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    return bwd_call(d, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, trans_coeff, tau, true, key_lens, q_lens, true, key_idx, true, q_live, true, dlse,
                    kv_images, dq, dk, dv, dqkv_stride, dout_stride, dtrans_coeff, dtau, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// merge of partial attentions (gta_merge.hip)
// ---------------------------------------------------------------------------------------------
namespace {
int merge_check(int32_t dtype, int32_t n, int32_t B, int32_t H, int32_t Tq, int32_t dh) {
    if (dtype != GTA_DTYPE_F32 && dtype != GTA_DTYPE_BF16) return fail(GTA_E_BADARG, "bad dtype");
    if (n < 1 || n > GTA_MERGE_MAX) return fail(GTA_E_BADARG, "a merge takes 1 to 8 partial attentions");
    if (B <= 0 || H <= 0 || Tq <= 0 || dh <= 0) return fail(GTA_E_BADARG, "non-positive size");
    if (dh % 8 || dh > 128) return fail(GTA_E_UNSUPPORTED, "the merge needs dh % 8 == 0 and dh <= 128");
    return GTA_OK;
}
// a [B,H,Tq,dh] operand the kernels move in 16-byte units: aligned base and (b, h, t) strides
int merge_rows_ok(const void* ptr, const int64_t* st, int esz) {
    if (!ptr) return fail(GTA_E_BADARG, "null argument");
    if ((uintptr_t)ptr % 16) return fail(GTA_E_BADARG, "merge operands must be 16-byte aligned");
    for (int i = 0; i < 3; ++i) if ((st[i] * esz) % 16) return fail(GTA_E_BADARG, "merge operand strides must keep rows 16-byte aligned");
    return GTA_OK;
}
}  // namespace

extern "C" int gta_attn_merge(int32_t dtype, int32_t n, int32_t B, int32_t H, int32_t Tq, int32_t dh,
                              const void* const* outs, const int64_t* outs_stride, const float* const* lses, const int64_t* lses_stride,
                              void* out, const int64_t* out_stride, float* lse, const int64_t* lse_stride, void* stream) {
    if (int rc = merge_check(dtype, n, B, H, Tq, dh)) return rc;
    if (!outs || !outs_stride || !lses || !lses_stride || !out_stride || !lse || !lse_stride) return fail(GTA_E_BADARG, "null argument");
    const int esz = dtype == GTA_DTYPE_BF16 ? 2 : 4;
    GtaMergeParams p;
    memset(&p, 0, sizeof p);
    for (int i = 0; i < n; ++i) {
        if (int rc = merge_rows_ok(outs[i], outs_stride + 3 * i, esz)) return rc;
        if (!lses[i]) return fail(GTA_E_BADARG, "null argument");
        p.outs[i] = outs[i]; p.lses[i] = lses[i];
        for (int j = 0; j < 3; ++j) { p.outs_st[i][j] = outs_stride[3 * i + j]; p.lses_st[i][j] = lses_stride[3 * i + j]; }
    }
    if (int rc = merge_rows_ok(out, out_stride, esz)) return rc;
    p.out = out; p.lse = lse;
    for (int j = 0; j < 3; ++j) { p.out_st[j] = out_stride[j]; p.lse_st[j] = lse_stride[j]; }
    p.n = n; p.B = B; p.H = H; p.Tq = Tq; p.dh = dh;
    return launch_status(gta_merge_dispatch(p, esz, (hipStream_t)stream), "no kernel instance");
}

extern "C" int gta_attn_merge_bwd(int32_t dtype, int32_t n, int32_t B, int32_t H, int32_t Tq, int32_t dh,
                                  const void* const* outs, const int64_t* outs_stride, const float* const* lses, const int64_t* lses_stride,
                                  const void* dout, const int64_t* dout_stride, const float* dlse, const int64_t* dlse_stride,
                                  void* const* douts, const int64_t* douts_stride, float* const* dlses, const int64_t* dlses_stride,
                                  void* stream) {
    if (int rc = merge_check(dtype, n, B, H, Tq, dh)) return rc;
    if (!outs || !outs_stride || !lses || !lses_stride || !dout_stride || !douts || !douts_stride || !dlses || !dlses_stride || (dlse && !dlse_stride))
        return fail(GTA_E_BADARG, "null argument");
    const int esz = dtype == GTA_DTYPE_BF16 ? 2 : 4;
    GtaMergeBwdParams p;
    memset(&p, 0, sizeof p);
    for (int i = 0; i < n; ++i) {
        if (int rc = merge_rows_ok(outs[i], outs_stride + 3 * i, esz)) return rc;
        if (int rc = merge_rows_ok(douts[i], douts_stride + 3 * i, esz)) return rc;
        if (!lses[i] || !dlses[i]) return fail(GTA_E_BADARG, "null argument");
        p.outs[i] = outs[i]; p.lses[i] = lses[i]; p.douts[i] = douts[i]; p.dlses[i] = dlses[i];
        for (int j = 0; j < 3; ++j) {
            p.outs_st[i][j] = outs_stride[3 * i + j]; p.lses_st[i][j] = lses_stride[3 * i + j];
            p.douts_st[i][j] = douts_stride[3 * i + j]; p.dlses_st[i][j] = dlses_stride[3 * i + j];
        }
    }
    if (int rc = merge_rows_ok(dout, dout_stride, esz)) return rc;
    p.dout = dout; p.dlse = dlse;
    for (int j = 0; j < 3; ++j) { p.dout_st[j] = dout_stride[j]; p.dlse_st[j] = dlse ? dlse_stride[j] : 0; }
    p.n = n; p.B = B; p.H = H; p.Tq = Tq; p.dh = dh;
    return launch_status(gta_merge_bwd_dispatch(p, esz, (hipStream_t)stream), "no kernel instance");
}

// ---------------------------------------------------------------------------------------------
// index tensors of a key mask and a query mask (gta_maskidx.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int gta_mask_index(const uint8_t* key_mask, int32_t B, int32_t Tk, int32_t* key_idx, int32_t* key_lens, uint8_t* k_live,
                              const uint8_t* query_mask, int32_t Tq, int32_t* q_lens, void* stream) {
    if (B < 1) return fail(GTA_E_BADARG, "B must be at least 1");
    if (!key_mask && !query_mask) return fail(GTA_E_BADARG, "null key_mask and null query_mask: one of the two is needed");
    if (key_mask && Tk < 1) return fail(GTA_E_BADARG, "Tk must be at least 1 with a key_mask");
    if (query_mask && Tq < 1) return fail(GTA_E_BADARG, "Tq must be at least 1 with a query_mask");
    if (key_mask && !key_idx) return fail(GTA_E_BADARG, "null key_idx (a key_mask comes with key_idx and key_lens)");
    if (key_mask && !key_lens) return fail(GTA_E_BADARG, "null key_lens (a key_mask comes with key_idx and key_lens)");
    if (query_mask && !q_lens) return fail(GTA_E_BADARG, "null q_lens (a query_mask comes with q_lens)");
    return launch_status(gta_maskidx_dispatch(key_mask, B, Tk, key_idx, key_lens, k_live, query_mask, Tq, q_lens, (hipStream_t)stream),
                         "no kernel instance");
}

// ---------------------------------------------------------------------------------------------
// plain attention (identity layout) with an optional key bias: the attention stage of the generic path
// ---------------------------------------------------------------------------------------------
extern "C" int gta_attn_fwd_plain(const GtaAttnDesc* d, const void* q, const void* k, const void* v,
                                  const float* key_bias, int64_t bias_pitch, const float* tau, void* out, float* lse,
                                  void* stream) {
    if (!d || !q || !k || !v || !out) return fail(GTA_E_BADARG, "null argument");
    if (d->abi_version != GTA_ABI_VERSION) return fail(GTA_E_BADARG, "abi_version mismatch");
    if (d->dtype != GTA_DTYPE_F32 && d->dtype != GTA_DTYPE_BF16) return fail(GTA_E_BADARG, "bad dtype");
    if (d->B <= 0 || d->H <= 0 || d->Tq <= 0 || d->Tk <= 0 || d->dh <= 0) return fail(GTA_E_BADARG, "non-positive size");
    const int dhp = (d->dh + 7) / 8 * 8;
    if (dhp != d->dh || d->dh > 128) return fail(GTA_E_UNSUPPORTED, "plain attention needs dh % 8 == 0 and dh <= 128 (pad the channels)");
    if (key_bias && (bias_pitch % 64 || bias_pitch < d->Tk)) return fail(GTA_E_BADARG, "bias_pitch must be a multiple of 64 >= Tk");
    GtaFwdParams p;
    memset(&p, 0, sizeof p);
    p.q = q; p.k = k; p.v = v; p.o = out; p.lse = lse; p.tau = tau;
    p.kbias = key_bias; p.kbias_pitch = bias_pitch;
    copy_strides(p, d);
    p.B = d->B; p.H = d->H; p.Tq = d->Tq; p.Tk = d->Tk; p.Nq = 1; p.Nk = 1; p.Pq = d->Tq; p.Pk = d->Tk;
    p.invPq = 1.0f / p.Pq; p.invPk = 1.0f / p.Pk;
    p.dh = d->dh; p.nso2 = 0; p.n_qtiles = (d->Tq + 127) / 128; p.scale = d->scale;
    p.flags = d->flags & GTA_FLAG_FP32_PRODUCTS;
    if (p.flags && d->dtype != GTA_DTYPE_F32) return fail(GTA_E_BADARG, "GTA_FLAG_FP32_PRODUCTS is for fp32 inputs");
    const long n_wg = (long)d->B * d->H * p.n_qtiles;
    return launch_status(gta_fwd_dispatch(p, padded_dh(d->dh), esz_of(d), true, (int)n_wg, (hipStream_t)stream), "no kernel instance");
}

// -------------------------------------------------------------------------------------------------------------------------------
// rep-gradient sums (gta_repgrad.hip)
// -------------------------------------------------------------------------------------------------------------------------------
namespace {

// the side's (T, N, tokens per workgroup, workgroups per view), or an error
int repgrad_geometry(const GtaAttnDesc* d, int32_t side, int& T, int& N, int& tpb, long& chunks) {
    if (int rc = check_header(d)) return rc;
    if (side != 0 && side != 1) return fail(GTA_E_BADARG, "side must be 0 (query) or 1 (key)");
    T = side ? d->Tk : d->Tq;
    N = side ? d->Nk : d->Nq;
    if (d->B <= 0 || d->H <= 0 || T <= 0 || N <= 0 || T % N) return fail(GTA_E_BADARG, "non-positive size or tokens not a multiple of views");
    tpb = gta_repgrad_tpb(d->H);
    if (!tpb) return fail(GTA_E_UNSUPPORTED, "rep-gradient sums serve at most 256 heads");
    chunks = (T / N + tpb - 1) / tpb;
    if ((long)d->B * N * chunks > 0x7fffffffL) return fail(GTA_E_UNSUPPORTED, "rep-gradient sums: grid too large");
    return GTA_OK;
}

bool bad_operand(const void* ptr, const int64_t* st, int esz) {
    return !ptr || !st || ((uintptr_t)ptr % esz) != 0 || st[0] < 0 || st[1] < 0 || st[2] < 0;
}

}  // namespace

extern "C" int64_t gta_rep_grad_workspace_bytes(const GtaAttnDesc* d, int32_t side) {
    int T, N, tpb;
    long chunks;
    if (int rc = repgrad_geometry(d, side, T, N, tpb, chunks)) return rc;
    return (int64_t)d->B * N * chunks * 16 * (int64_t)sizeof(float);
}

// the three sums entries.  varlen (gta_rep_grad_sums_varlen) and masked (gta_rep_grad_sums_masked) are the explicit selectors of the
// VARLEN / MASKED instances -- never "lens (live) is non-null"
static int rep_grad_call(const GtaAttnDesc* d, int32_t side, int32_t n_pairs,
                         const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                         const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                         bool varlen, const int32_t* lens, bool masked, const uint8_t* live,
                         float* view_sums, float* so2_sums, float* t2_sums,
                         void* workspace, int64_t workspace_bytes, void* stream) {
    int T, N, tpb;
    long chunks;
    if (int rc = repgrad_geometry(d, side, T, N, tpb, chunks)) return rc;
    if (varlen && !lens) return fail(GTA_E_BADARG, "null lens");
    if (masked && !live) return fail(GTA_E_BADARG, "null live");
    if (d->dtype != GTA_DTYPE_F32 && d->dtype != GTA_DTYPE_BF16) return fail(GTA_E_BADARG, "dtype must be GTA_DTYPE_F32 or GTA_DTYPE_BF16");
    if (n_pairs != 1 && n_pairs != 2) return fail(GTA_E_BADARG, "n_pairs must be 1 or 2");
    if (!view_sums && !so2_sums && !t2_sums) return fail(GTA_E_BADARG, "no output requested");
    const int esz = esz_of(d);
    if (bad_operand(a0, a0_stride, esz) || bad_operand(b0, b0_stride, esz) ||
        (n_pairs == 2 && (bad_operand(a1, a1_stride, esz) || bad_operand(b1, b1_stride, esz))))
        return fail(GTA_E_BADARG, "null, misaligned or negatively strided operand");
    if (int rc = check_slabs(d)) return rc;
    const bool euclid = (d->flags & GTA_FLAG_EUCLID) != 0;
    if (d->d_se3 % (euclid ? 3 : 4) || d->d_so2 % 2 || d->d_t2 % 3) return fail(GTA_E_LAYOUT, "se3 / so2 / t2 slab not a whole number of groups");
    if ((view_sums && d->d_se3 == 0) || (so2_sums && d->d_so2 == 0) || (t2_sums && d->d_t2 == 0))
        return fail(GTA_E_BADARG, "sums requested for an empty slab");
    if (((uintptr_t)view_sums | (uintptr_t)so2_sums | (uintptr_t)t2_sums) % 4) return fail(GTA_E_BADARG, "misaligned output");
    const int64_t need = (int64_t)d->B * N * chunks * 16 * (int64_t)sizeof(float);
    if (view_sums && (!workspace || (uintptr_t)workspace % 4 || workspace_bytes < need))
        return fail(GTA_E_BADARG, "view sums need a workspace of gta_rep_grad_workspace_bytes");
    GtaRepGradParams p;
    p.a[0] = a0; p.b[0] = b0;
    p.a[1] = n_pairs == 2 ? a1 : a0; p.b[1] = n_pairs == 2 ? b1 : b0;
    for (int i = 0; i < 3; ++i) {
        p.as[0][i] = a0_stride[i]; p.bs[0][i] = b0_stride[i];
        p.as[1][i] = n_pairs == 2 ? a1_stride[i] : a0_stride[i];
        p.bs[1][i] = n_pairs == 2 ? b1_stride[i] : b0_stride[i];
    }
    p.npairs = n_pairs;
    p.B = d->B; p.H = d->H; p.T = T; p.N = N; p.P = T / N;
    p.tpb = tpb; p.chunks = (int)chunks;
    p.off_se3 = d->d_triv;
    p.n_se3 = view_sums ? d->d_se3 / (euclid ? 3 : 4) : 0;
    p.off_so2 = d->d_triv + d->d_se3 + d->d_so3;
    p.n_so2 = so2_sums ? d->d_so2 / 2 : 0;
    p.off_t2 = p.off_so2 + d->d_so2;
    p.n_t2 = t2_sums ? d->d_t2 / 3 : 0;
    p.part = (float*)workspace; p.view_out = view_sums; p.so2_out = so2_sums; p.t2_out = t2_sums;
    p.lens = varlen ? lens : nullptr;
    p.live = masked ? live : nullptr;
    return launch_status(gta_repgrad_dispatch(p, esz, euclid, (hipStream_t)stream), "grid too large");
}

extern "C" int gta_rep_grad_sums(const GtaAttnDesc* d, int32_t side, int32_t n_pairs,
                                 const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                                 const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                                 float* view_sums, float* so2_sums, float* t2_sums,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    return rep_grad_call(d, side, n_pairs, a0, a0_stride, b0, b0_stride, a1, a1_stride, b1, b1_stride, false, nullptr, false, nullptr,
                         view_sums, so2_sums, t2_sums, workspace, workspace_bytes, stream);
}

extern "C" int gta_rep_grad_sums_varlen(const GtaAttnDesc* d, int32_t side, int32_t n_pairs,
                                        const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                                        const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                                        const int32_t* lens, float* view_sums, float* so2_sums, float* t2_sums,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    return rep_grad_call(d, side, n_pairs, a0, a0_stride, b0, b0_stride, a1, a1_stride, b1, b1_stride, true, lens, false, nullptr,
                         view_sums, so2_sums, t2_sums, workspace, workspace_bytes, stream);
}

extern "C" int gta_rep_grad_sums_masked(const GtaAttnDesc* d, int32_t side, int32_t n_pairs,
                                        const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                                        const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                                        const uint8_t* live, float* view_sums, float* so2_sums, float* t2_sums,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    return rep_grad_call(d, side, n_pairs, a0, a0_stride, b0, b0_stride, a1, a1_stride, b1, b1_stride, false, nullptr, true, live,
                         view_sums, so2_sums, t2_sums, workspace, workspace_bytes, stream);
}
