/*
 * gta_hip.h -- C ABI of libgta_hip.so: MI355X (gfx950) kernels for GTA attention.
 *
 * The reference (autonomousvision/gta) has no FFI: its seam for this path is the Python
 * function ``multihead_geometric_transform_attention`` (source/utils/gta.py:92-279) called
 * from ``Attention.forward`` (source/layers.py:409-430) and the rep builders
 * ``pre_compute_reps`` (source/encoder.py:183-265, source/decoder.py:247-353).  The entry
 * points below are what a ctypes binding of those call sites needs.
 *
 * Conventions
 *   - plain C, raw DEVICE pointers, no torch types; the caller allocates every buffer, the
 *     library owns nothing and keeps no state; every call is asynchronous on `stream`
 *     (a hipStream_t passed as void*) and re-entrant.
 *   - return 0 on success, a negative GTA_E_* code otherwise; nothing throws, nothing is
 *     printed.  gta_strerror() names a code.
 *   - tokens are view-major (t = view * tokens_per_view + p), gta.py:160-162.
 *   - per-head channels are laid out [triv | se3 | so3 | so2 | t2], gta.py:115-122.
 */
#ifndef GTA_HIP_H
#define GTA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTA_ABI_VERSION 2   /* r05: flag bit 12 is GTA_FLAG_ITEM_CXX, 8/16-byte alignment rules of the rep builders, dtype-dependent workspace size */

/* element types of q/k/v/out (all four share one type per call) */
#define GTA_DTYPE_F32  0
#define GTA_DTYPE_BF16 1

/* flags of GtaAttnDesc.flags */
#define GTA_FLAG_V_TRANSFORM   (1u << 0) /* gta.py: v_transform=True (default)                 */
#define GTA_FLAG_EUCLID        (1u << 1) /* gta.py:146-156 + layers.py:213-224 (not fused yet) */
#define GTA_FLAG_PRETRANSFORMED (1u << 2) /* q,k,v already carry rho; only rho_q^-1 on output   */
#define GTA_FLAG_FUSED_KV      (1u << 3) /* force the single-kernel path (rho_k inside the loop)  */
#define GTA_FLAG_PREP_ONLY     (1u << 5) /* two-stage plan: run only the K/V pre-pass (fills workspace) */
#define GTA_FLAG_KV_READY      (1u << 4) /* workspace already holds K'/V' for these k,v,reps:     */
                                         /* skip the pre-pass (several query sets, one key set)   */
#define GTA_FLAG_PERSIST       (1u << 9) /* tuning: persistent grid (resident workgroups walk the query tiles) instead of one workgroup per tile; */
                                         /* chosen automatically for launches of 1..2 rounds of resident workgroups (short sequences) */
#define GTA_FLAG_FP32_PRODUCTS (1u << 10) /* fp32 inputs: split-bf16 (hi+lo) operands, three MFMAs per product: fp32-class */
                                         /* results for the reference's mixed_prec: False configs, 3x the MFMAs; with a workspace   */
                                         /* at padded dh <= 64 the two-stage plan (hi and lo images: twice the image bytes; such a    */
                                         /* workspace is NOT what gta_attn_bwd's kv_images wants), the single-kernel plan otherwise   */
                                         /* (gta_attn_fwd_workspace_bytes then returns 0)                                              */
#define GTA_FLAG_ROWS32        (1u << 11) /* tuning: keep the 32-rows-per-wave attention kernel (gta_fwd2.hip) where the     */
                                          /* 64-rows-per-wave one (gta_fwd64.hip: dh = 96, whole ring turns of key tiles) would run */
#define GTA_FLAG_ITEM_CXX      (1u << 12) /* tuning / diagnostics: keep the 64-rows-per-wave kernel's compiler-scheduled item prologue and epilogue  */
                                          /* where the generated item stream (gen_item64.py) would run; same results bit for bit               */
#define GTA_FLAG_BWD_KEYS32    (1u << 13) /* tuning / diagnostics (gta_attn_bwd): keep the 32-keys-per-wave dK/dV kernel where the generated    */
                                          /* 64-per-wave streams (gen_bwd64.py: bf16, dh = 96, MSN layout, >= 128 blocks of 256 keys / rows) would run        */
#define GTA_FLAG_BWD_KEYS64    (1u << 14) /* tuning / diagnostics (gta_attn_bwd): run that stream at bf16, dh = 96 whatever the number of blocks    */
#define GTA_FLAG_BWD_SPLIT     (1u << 15) /* tuning / diagnostics (gta_attn_bwd): the dQ and dK/dV kernels as two launches (per-kernel times under a profiler)     */
                                          /* where one joint launch would run; same results bit for bit                                                         */
#define GTA_FLAG_FWD2_GENERIC  (1u << 6) /* tuning / diagnostics (r06): keep gta_fwd2_kernel where the dh = 64 instance of gta_fwd_cl.hip (gta_fwdc_kernel) would run */
#define GTA_FLAG_NO_DMA        (1u << 8) /* debug: stage K/V tiles through VGPRs, not LDS-DMA  */

/* error codes */
#define GTA_OK              0
#define GTA_E_BADARG       -1   /* null pointer / non-positive size / bad dtype                 */
#define GTA_E_LAYOUT       -2   /* f_dims do not add up to dh, or a slab is mis-sized           */
#define GTA_E_UNSUPPORTED  -3   /* valid request this build has no kernel for (says which in    */
                                /* gta_strerror); never silently falls back                     */
#define GTA_E_LAUNCH       -4   /* HIP launch error                                             */
#define GTA_E_NODEVICE     -5

/* Per-view rep record produced by gta_build_view_reps and consumed by the attention kernels.
 * One record of GTA_VREP_STRIDE floats per (batch, view):
 *   [ 0:16)  "inv" matrix  = extrinsic E           (reference: extras['inv_se3rep_q'], encoder.py:236)
 *   [16:32)  "rep" matrix  = inverse(E)            (reference: extras['se3rep_q/k'],  encoder.py:219,235)
 *   [32:41)  D^1(R), R = inverse(E)[:3,:3]         (reference: extras['so3rep_*'][0], encoder.py:247-259)
 *   [41:66)  D^2(R)                                (reference: extras['so3rep_*'][1])
 * all row-major, fp32.  trans_coeff is NOT folded in (it is a per-layer parameter). */
#define GTA_VREP_STRIDE 72
#define GTA_VREP_INV    0
#define GTA_VREP_REP    16
#define GTA_VREP_D1     32
#define GTA_VREP_D2     41

#define GTA_MAX_VIEWS   16   /* per side, fused kernels */

typedef struct GtaAttnDesc {
    int32_t abi_version;      /* GTA_ABI_VERSION                                              */
    int32_t dtype;            /* GTA_DTYPE_*                                                  */
    int32_t B, H;             /* batch, heads                                                 */
    int32_t Tq, Tk;           /* tokens (all views) on the query / key side                   */
    int32_t Nq, Nk;           /* views per side; Tq % Nq == 0, Tk % Nk == 0 (gta.py:160-162)  */
    int32_t dh;               /* channels per head = d_triv+d_se3+d_so3+d_so2+d_t2            */
    int32_t d_triv, d_se3, d_so3, d_so2, d_t2;   /* f_dims (gta.py:115-122)                  */
    int32_t so3_degree;       /* L: so3 sub-blocks of 3,5,..,2L+1 channels (gta.py:174-198)   */
    uint32_t flags;           /* GTA_FLAG_*                                                   */
    float   scale;            /* dim_head ** -0.5 (layers.py:181)                             */
    int32_t _pad;
    /* element strides of (batch, head, token); the channel stride is 1.  q/k/v may be views
     * into a packed [B, T, 3*H*dh] projection (layers.py:389,394-395) -- no copy needed.     */
    int64_t q_stride[3], k_stride[3], v_stride[3], o_stride[3];
} GtaAttnDesc;

/* -------------------------------------------------------------------------------------------
 * Rep builders  (replace encoder.py:183-265 / decoder.py:247-353, gta.py:47-69, wigner_d.py:16-58)
 * ------------------------------------------------------------------------------------------- */

/* extrinsics [n_views,4,4] fp32 (extras['input_transforms'] / ['target_transforms'], flattened
 * over batch) -> vrep [n_views, GTA_VREP_STRIDE].  so3_degree in {0,1,2}.  The Wigner-D path is
 * the reference's ZYZ-Euler formula D = Z(g3) J Z(g2) J Z(g1) incl. its 1e-5 gimbal masks
 * (wigner_d.py:28-49); J is a restatement of the absent J_dense.pt (parity unpinned there). */
int gta_build_view_reps(const float* extrinsics, int32_t n_views, int32_t so3_degree,
                        float* vrep, void* stream);

/* coord [n_tokens,2] fp32 in [0,1) (extras['input_coord'] / ['target_coord'] flattened) ->
 * cs [n_tokens, 2*nfreqs, 2] = (cos, sin) of theta_{t, c=2f+d} = max_freq_d * 2pi * coord_d *
 * 2^(f+1-F)  (make_SO2mats, gta.py:47-69; block order c = 2f+d from gta.py:68 + encoder.py:195).
 * Alignment: coord 8 bytes, cs 16 bytes (the kernel moves a token's coordinate pair and a frequency's two (cos, sin) pairs in one
 * access each); anything else returns GTA_E_BADARG. */
int gta_build_so2_table(const float* coord, int32_t n_tokens, int32_t nfreqs,
                        float max_freq_h, float max_freq_w, int32_t shared_freqs,
                        float* cs, void* stream);

/* Both of the above in ONE launch (they are independent and launch-latency sized): what
 * pre_compute_reps (source/encoder.py:183-265) does for a gta_so3-style config in one call.
 * Arguments (and alignment requirements) as for gta_build_view_reps followed by those of gta_build_so2_table. */
int gta_build_reps(const float* extrinsics, int32_t n_views, int32_t so3_degree, float* vrep,
                   const float* coord, int32_t n_tokens, int32_t nfreqs, float max_freq_h,
                   float max_freq_w, int32_t shared_freqs, float* cs, void* stream);

/* -------------------------------------------------------------------------------------------
 * Fused forward  (replaces gta.py:92-279 + AttnFn, layers.py:202-211)
 *   q [B,H,Tq,dh], k,v [B,H,Tk,dh] through the strides in desc; out like q.
 *   vrep_q [B,Nq,GTA_VREP_STRIDE], vrep_k [B,Nk,...] (may be NULL when d_se3 = d_so3 = 0)
 *   cs_q [B,Tq,d_so2/2,2], cs_k [B,Tk,d_so2/2,2]      (may be NULL when d_so2 = 0)
 *   trans_coeff: device pointer to the layer's scalar parameter (layers.py:191) or NULL (=1)
 *   tau:         device pointer to the softmax temperature (layers.py:195-200) or NULL (=1)
 *   lse [B,H,Tq] fp32 out (natural-log sum-exp of the scaled logits; needed by backward), or NULL
 * ------------------------------------------------------------------------------------------- */
int gta_attn_fwd(const GtaAttnDesc* desc,
                 const void* q, const void* k, const void* v,
                 const float* vrep_q, const float* vrep_k,
                 const float* cs_q, const float* cs_k,
                 const float* trans_coeff, const float* tau,
                 void* out, float* lse,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* Two execution plans, same results:
 *   workspace == NULL (or GTA_FLAG_FUSED_KV): ONE kernel; rho_k is applied to each K/V tile inside
 *       the attention loop (re-done once per 128-row query tile).
 *   workspace of >= gta_attn_fwd_workspace_bytes(desc) bytes: a K/V pre-pass writes K' = rho_k K,
 *       V' = rho_k V once as bf16 tile images into the workspace, then a lean attention kernel
 *       streams them.  The workspace content stays valid for other query sets against the same
 *       keys (GTA_FLAG_KV_READY) and is what the backward consumes.
 *   Size: [K'/V' images | per-tile key norms] depend on (B, H, Tk, dh) only.  For bf16 inputs at dh in (64, 96] the workspace ends
 *       with B * Nq * 24 KiB of query-side operand tiles (rewritten by every call), so the size ALSO depends on the query side's
 *       number of views: a workspace kept for GTA_FLAG_KV_READY calls must be sized for the largest Nq it will see (query the size
 *       with that Nq; a too-small buffer returns GTA_E_BADARG).  The size depends on desc->flags: GTA_FLAG_FP32_PRODUCTS doubles the
 *       images where that mode has a two-stage plan (fp32 inputs, padded dh <= 64) and makes the size 0 where it has none. */
int64_t gta_attn_fwd_workspace_bytes(const GtaAttnDesc* desc);

/* -------------------------------------------------------------------------------------------
 * Backward  (replaces PyTorch autograd over gta.py:92-279 + layers.py:202-211)
 *   inputs : q, k, v (as given to the forward; strides from desc), out and lse from the forward,
 *            dout [B,H,Tq,dh] with element strides dout_stride[3] (b,h,t), reps as in the forward.
 *   kv_images: the forward's workspace (K'/V' tile images) or NULL -> recomputed here.
 *   plan     : Q''/dO~ pre-pass -> dQ kernel -> dK/dV kernel, each recomputing S and dP from the images (14 GEMM-units).
 *              Deterministic (no atomics: fixed-order reductions).
 *   outputs: dq, dk, dv with element strides dqkv_stride[9] = dq(b,h,t), dk(b,h,t), dv(b,h,t);
 *            dtrans_coeff [1] fp32 (d loss / d trans_coeff, layers.py:191; written, not accumulated) or NULL;
 *            dtau [1] fp32 (d loss / d tau of TemperatureAdjsutableSoftmax, layers.py:135-143,195-200) or
 *            NULL.  The logits are z = scale q'.k' / tau, so dL/dtau = -(1/tau) sum_ij dz_ij z_ij
 *            = -(1/tau) sum_i <q'_i, dq'_i> = -(1/tau) sum_i <q_i, dq_i>  (rho_q is linear): it falls out of
 *            the dQ kernel's epilogue, no extra pass over the tiles.
 *   No gradient is produced for the reps/poses here: gta_rep_grad_sums is the separate pass that serves them.
 *   GTA_FLAG_FP32_PRODUCTS (r06; fp32 inputs, dh <= 64; other sizes: GTA_E_UNSUPPORTED -> gta_rep_apply + gta_attn_bwd_plain_f32): the fp32-faithful
 *            backward on the matrix cores -- every product of the five contractions as three bf16 MFMAs over hi / lo operand images (the
 *            arithmetic of the forward under the same flag); kv_images must then be the workspace of a forward run WITH the flag (four
 *            images per tile) or NULL; the workspace is twice as large (gta_attn_bwd_workspace_bytes depends on desc->flags); dtau is formed
 *            in the dQ walk as sum_ij dS_ij (S_ij - m_i), m_i = sum_j P_ij S_ij (centred per row: DESIGN.md section 4.6).
 * ------------------------------------------------------------------------------------------- */
int64_t gta_attn_bwd_workspace_bytes(const GtaAttnDesc* desc);
int gta_attn_bwd(const GtaAttnDesc* desc,
                 const void* q, const void* k, const void* v, const void* out, const void* dout,
                 const float* lse,
                 const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                 const float* trans_coeff, const float* tau,
                 const void* kv_images,
                 void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                 float* dtrans_coeff, float* dtau,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* Backward with per-scene prefixes (gta_attention's key_views_backward): the backward of gta_attn_fwd_varlen.
 *   key_lens: [B] int32 on the device, valid key TOKENS per scene, as in the forward (clamped to 1..Tk).  dk / dv rows at or past the prefix
 *       are written as zeros; k, v, cs_k rows there are never loaded; the padded key tiles are neither built nor walked.
 *   q_lens:   [B] int32 on the device or NULL (every query row is live), clamped to 1..Tq.  Query rows at or past the prefix take no part:
 *       their q, out, dout, lse and cs_q are never loaded, they add nothing to dk, dv, dtrans_coeff or dtau, and their dq rows are zeros
 *       (self-attention over padded views, where those rows hold anything).
 *   kv_images: the workspace of a gta_attn_fwd_varlen call under the same key_lens, or NULL -> rebuilt here by the VARLEN pre-pass.
 *   Kernels: VARLEN instances of the compiled pre-pass / dQ / dK,dV kernels as three launches, for bf16 and fp32 inputs at every head size; the
 *       generated 64-row streams are never selected (GTA_FLAG_BWD_KEYS64 is ignored).  dq, dk, dv of scene b are bit for bit those of
 *       gta_attn_bwd (GTA_FLAG_BWD_KEYS32) on that scene alone with its keys (and, with q_lens, its queries) cut to the prefixes.
 *   gta_attn_bwd_varlen_supported: what gta_attn_fwd_varlen_supported answers -- GTA_E_UNSUPPORTED with the reason in gta_strerror() for
 *       GTA_FLAG_FP32_PRODUCTS, GTA_FLAG_FUSED_KV, GTA_FLAG_PRETRANSFORMED and for layouts without a fused kernel.
 *   workspace: >= gta_attn_bwd_workspace_bytes(desc).  Every other argument, check and error code: as in gta_attn_bwd.  The gradients of the
 *       reps / poses under the same prefixes: gta_rep_grad_sums_varlen. */
int gta_attn_bwd_varlen_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_varlen(const GtaAttnDesc* desc,
                        const void* q, const void* k, const void* v, const void* out, const void* dout,
                        const float* lse,
                        const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                        const float* trans_coeff, const float* tau,
                        const int32_t* key_lens, const int32_t* q_lens,
                        const void* kv_images,
                        void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                        float* dtrans_coeff, float* dtau,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Backward over any per-scene subset of the key tokens (gta_attention's key_mask with key_mask_backward): the backward of
 * gta_attn_fwd_gather.  It is gta_attn_bwd_varlen without q_lens (this entry has no query-side mask -- gta_attn_bwd_qmask has --: every query row is live and must hold finite
 * values) whose dK/dV walk runs in GATHER instances: the walk over the compacted K'/V' images is the VARLEN walk, and the epilogue reads the
 * token of a compacted row from key_idx -- that token gives the view record, the cs_k row, the raw K / V row of the dtrans_coeff term and the
 * row of dk / dv that is written.  The dQ walk and the q-side pre-pass are the VARLEN kernels as they are.
 *   key_idx:  [B, Tk] int32 on the device; NULL: GTA_E_BADARG, with kv_images too (the scatter reads it).  For THIS entry every row must be a
 *       permutation of [0, Tk): the key_lens[b] valid tokens first, then the masked ones (what the Python layer's key_index_tensors builds).
 *       Positions at or past key_lens[b] are read here: dk / dv rows of the tokens they name are written as zeros, and nothing of those
 *       tokens (k, v, cs_k) is loaded.  Then every row of dk and dv is written exactly once.  A row that is not a permutation leaves the
 *       gradient rows of the tokens it does not name unwritten; values are clamped into [0, Tk) as in the forward, so no value moves a load
 *       or a store out of the scene's rows.  (The forward entry's contract -- entries at or past key_lens[b] are never read -- is unchanged.)
 *   key_lens: as in gta_attn_fwd_gather; NULL: GTA_E_BADARG.
 *   kv_images: the workspace of a gta_attn_fwd_gather call under the same key_idx / key_lens, or NULL -> rebuilt here by the GATHER pre-pass.
 *   vrep_k records of views no valid token belongs to are loaded with the others and enter no result (they may hold NaN).
 *   Kernels: three launches for bf16 and fp32 inputs at every head size; the generated 64-row streams are never selected, and
 *       GTA_FLAG_FP32_PRODUCTS is refused.  Under a mask of whole leading views every output is bit for bit that of gta_attn_bwd_varlen
 *       with the same key_lens and q_lens = NULL.
 *   gta_attn_bwd_gather_supported: what gta_attn_bwd_varlen_supported answers.
 *   workspace: >= gta_attn_bwd_workspace_bytes(desc).  Every other argument, check and error code: as in gta_attn_bwd_varlen.  No gradients of
 *       the reps / poses under a mask yet. */
int gta_attn_bwd_gather_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_gather(const GtaAttnDesc* desc,
                        const void* q, const void* k, const void* v, const void* out, const void* dout,
                        const float* lse,
                        const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                        const float* trans_coeff, const float* tau,
                        const int32_t* key_idx, const int32_t* key_lens,
                        const void* kv_images,
                        void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                        float* dtrans_coeff, float* dtau,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Backward of the PAIR (out, lse) (gta_attention's return_lse under grad): gta_attn_bwd with the gradient of the log-sum-exp.
 *   dlse: [B,H,Tq] fp32, contiguous, non-NULL (GTA_E_BADARG) -- d loss / d lse per query row, lse as the forward wrote it (natural log).
 *   The exact gradient of the logits is dS_ij = P_ij (dP_ij - D_i + dlse_i): the q-side pre-pass runs in instances that store -(D - dlse)
 *       where gta_attn_bwd's store -D, and every dQ / dK,dV kernel -- compiled pair, generated 64-row streams, X3 walks -- is the one
 *       gta_attn_bwd launches for the same desc.  An all-zero dlse gives dq, dk, dv, dtrans_coeff and dtau bit for bit those of gta_attn_bwd.
 *       Under GTA_FLAG_FP32_PRODUCTS the centred dtau of the X3 dQ walk accounts for sum_j dS_ij = dlse_i.
 *   gta_attn_bwd_dlse_supported: 0 where gta_attn_bwd serves desc, else its error with the reason in gta_strerror() (layouts without a
 *       fused kernel, GTA_FLAG_PRETRANSFORMED, GTA_FLAG_FP32_PRODUCTS outside fp32 inputs at dh <= 64).  With per-scene prefixes or masks: the gta_attn_bwd_*_dlse entries below.
 *   Every other argument, check, workspace size and error code: as in gta_attn_bwd. */
int gta_attn_bwd_dlse_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_dlse(const GtaAttnDesc* desc,
                      const void* q, const void* k, const void* v, const void* out, const void* dout,
                      const float* lse, const float* dlse,
                      const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                      const float* trans_coeff, const float* tau,
                      const void* kv_images,
                      void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                      float* dtrans_coeff, float* dtau,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * Merge of partial attentions (gta_attention_merge): n in 1..8 attentions (out_i, lse_i) of the SAME queries over DISJOINT key sets
 * combine into the attention over the union.  With a_i = softmax_i(lse_i) per query row:
 *     out = sum_i a_i out_i,   lse = logsumexp_i(lse_i);      dout_i = a_i dout,   dlse_i = a_i (dlse + <dout, out_i - out>).
 *   dtype: GTA_DTYPE_* of every out / dout operand; B, H, Tq, dh: their [B,H,Tq,dh] shape, dh % 8 == 0 and <= 128 (else GTA_E_UNSUPPORTED).
 *   outs, lses (and douts, dlses): HOST arrays of n DEVICE pointers; *_stride: host arrays of the (batch, head, token) element strides, three
 *       per operand ([n][3] for the arrays); the channel stride is 1.  out-like operands: 16-byte aligned base and rows (GTA_E_BADARG);
 *       lse-like operands are [B,H,Tq] fp32 views with any strides.  The host arrays are read during the call only.
 *   Arithmetic in fp32, one rounding to dtype.  A partial whose lse_i is -inf on a row (no key) is selected out, not multiplied: its out_i
 *       row enters no arithmetic (it may hold NaN; it must be readable memory), its dout_i row and dlse_i are exact zeros; a row with every lse_i = -inf gives out = 0, lse = -inf.
 *       n = 1 returns its input bit for bit.
 *   gta_attn_merge_bwd: dout like out, dlse [B,H,Tq] fp32 through dlse_stride or NULL (= 0); douts / dlses are written, not accumulated.
 *   Kernels (gta_merge.hip): HBM-bound streams, one 16-byte unit per lane, rows in the memory order of [B,Tq,H,dh] tensors, no LDS, no
 *       workspace.  No operand may alias an output.
 * ------------------------------------------------------------------------------------------- */
int gta_attn_merge(int32_t dtype, int32_t n, int32_t B, int32_t H, int32_t Tq, int32_t dh,
                   const void* const* outs, const int64_t* outs_stride, const float* const* lses, const int64_t* lses_stride,
                   void* out, const int64_t* out_stride, float* lse, const int64_t* lse_stride, void* stream);
int gta_attn_merge_bwd(int32_t dtype, int32_t n, int32_t B, int32_t H, int32_t Tq, int32_t dh,
                       const void* const* outs, const int64_t* outs_stride, const float* const* lses, const int64_t* lses_stride,
                       const void* dout, const int64_t* dout_stride, const float* dlse, const int64_t* dlse_stride,
                       void* const* douts, const int64_t* douts_stride, float* const* dlses, const int64_t* dlses_stride,
                       void* stream);

/* -------------------------------------------------------------------------------------------
 * Generic path for the reference's ablations (any f_dims layout): t2 slab (gta.py:221-238,272-274),
 * euclid similarity (GTA_FLAG_EUCLID; gta.py:146-156,251-253 + EuclidAttnFn layers.py:213-224),
 * so3 of degree 1, unaligned slabs.  Usage: q' = apply(mode 0), k' = apply(mode 1)
 * (+ key_bias under euclid), v' = apply(mode 1), o~ = gta_attn_fwd_plain(q',k',v',key_bias),
 * o = apply(mode 2) -- or, for a forward without gradient at dh % 8 == 0, the single entry gta_attn_fwd_staged below.
 *   x, y: [B,H,T,dh] through x_stride/y_stride (b,h,t), dtype from desc; T,N = Tq,Nq (modes 0,2) or Tk,Nk.
 *   coord [B,T,2]: the token coordinates of the t2 slab (make_T2mats, gta.py:72-89) or NULL.
 *   key_bias (mode 1, or NULL): [B,H,bias_pitch] <- -0.5 * bias_scale * |y|^2 per token.
 * ------------------------------------------------------------------------------------------- */
int gta_rep_apply(const GtaAttnDesc* desc, int32_t mode, const void* x, const int64_t* x_stride,
                  const float* vrep, const float* cs, const float* coord, const float* trans_coeff,
                  void* y, const int64_t* y_stride, float* key_bias, float bias_scale, int64_t bias_pitch,
                  void* stream);

/* Adjoint of gta_rep_apply(mode): dx = M^T dy (what autograd produces for gta.py:134-238 on the generic path).
 *   x: the tensor gta_rep_apply(mode) was given; dy, dx: [B,H,T,dh] through their strides.
 *   dtc_rows [B,H,T] fp32 or NULL: this row's contribution to d loss / d trans_coeff (sum them in a fixed order).
 *   dkey_bias [B,H,bias_pitch] or NULL (mode 1 under euclid): gradient w.r.t. the key bias the forward call wrote;
 *   folded in as dy - bias_scale * dkey_bias * y.  Rows whose slabs carry no bias term (so3/so2/t2) ignore it. */
int gta_rep_apply_bwd(const GtaAttnDesc* desc, int32_t mode, const void* x, const int64_t* x_stride,
                      const void* dy, const int64_t* dy_stride, const float* vrep, const float* cs,
                      const float* coord, const float* trans_coeff, const float* dkey_bias, float bias_scale,
                      int64_t bias_pitch, void* dx, const int64_t* dx_stride, float* dtc_rows, void* stream);

/* Staged generic forward: the five calls above as ONE entry -- a K/V pre-pass that writes K' and V' as bf16 tile images (and, under
 * GTA_FLAG_EUCLID, the per-key bias -0.5 * scale * |k'|^2 in fp32, from the fp32 k') plus one attention kernel that applies rho_q in
 * its prologue and rho_q^-1 in its epilogue, per row in LDS; no q', k', v' or o~ tensor is written (gta_fwd_gen.hip).  For every layout
 * of the generic path with dh % 8 == 0 and dh <= 128, bf16 or fp32 inputs, the default arithmetic (operands rounded to bf16 once,
 * after rho; fp32 accumulation and softmax).  Forward only: a gradient goes through the five calls and their adjoints.
 *   gta_attn_fwd_staged_supported: 0, or GTA_E_LAYOUT for slabs that do not add up / are mis-sized, or GTA_E_UNSUPPORTED with the
 *       reason in gta_strerror(): dh % 8 != 0, dh > 128, GTA_FLAG_FP32_PRODUCTS, GTA_FLAG_PRETRANSFORMED (those keep the five calls).
 *   workspace: >= gta_attn_fwd_staged_workspace_bytes(desc) bytes (0 when unsupported), 256-byte aligned, [images | bias]; it depends
 *       on B, H, Tk and dh only, so one workspace serves every query set against the same keys.  GTA_FLAG_KV_READY skips the pre-pass
 *       and trusts the workspace, GTA_FLAG_PREP_ONLY runs the pre-pass alone -- exactly as in gta_attn_fwd.
 *   coord_q [B,Tq,2], coord_k [B,Tk,2]: the t2 tables gta_rep_apply takes (NULL without a t2 slab); the other operands, the argument
 *       checks and the error codes are those of gta_attn_fwd.  lse (or NULL): log sum_k exp((scale q'.k' + bias_k) / tau) per query
 *       row -- the convention of gta_attn_fwd_plain with that key bias (the row-constant -scale |q'|^2 / 2 of the euclid similarity
 *       is not in it).
 * gta_attn_fwd_supported() keeps answering GTA_E_UNSUPPORTED for these layouts: that entry names the chunk-wise fused kernels. */
int     gta_attn_fwd_staged_supported(const GtaAttnDesc* desc);
int64_t gta_attn_fwd_staged_workspace_bytes(const GtaAttnDesc* desc);
int gta_attn_fwd_staged(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                        const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                        const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau,
                        void* out, float* lse, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-scene key prefixes (gta_attention's key_views): scene b attends over its first key_lens[b] key tokens only -- with view-major
 * tokens, over its first key_lens[b] / Pk views.  key_lens: [B] int32 on the device, in TOKENS, each in 1..Tk (the kernels clamp to that
 * range; the Python layer validates on the host).  K, V and the key-side tables keep their [B, Tk, ...] / [B, Nk, ...] shapes; what lies at
 * or past the prefix is never used, so it may hold anything, NaN and Inf included: rows of k, v, cs_k, coord_k there are not loaded; the
 * vrep_k records of padded views are loaded with the others (they must be readable memory) and enter no result.
 * out and lse of scene b are those of the same call on that scene alone with its key side cut to the prefix -- bit for bit where that
 * call runs the same kernel family -- and the tiles past the prefix are neither built nor streamed.  Forward only.
 *   gta_attn_fwd_varlen: the two-stage plan of gta_attn_fwd with the VARLEN instances of its pre-pass and of the 32-rows-per-wave attention kernel, gta_fwd2_kernel -- always that
 *       kernel, whatever gta_attn_fwd would pick for the shape.  *_supported: what gta_attn_fwd_supported answers, and GTA_E_UNSUPPORTED
 *       with the reason in gta_strerror() for GTA_FLAG_FUSED_KV, GTA_FLAG_FP32_PRODUCTS and GTA_FLAG_PRETRANSFORMED.
 *   gta_attn_fwd_staged_varlen: the same for gta_attn_fwd_staged (any layout with dh % 8 == 0); *_supported: gta_attn_fwd_staged_supported.
 *   workspace: required (NULL: GTA_E_BADARG), sized by gta_attn_fwd_workspace_bytes / gta_attn_fwd_staged_workspace_bytes -- by Tk, not by
 *       the prefixes; the images of scene b occupy the first ceil(key_lens[b] / 64) tiles of its slot.  GTA_FLAG_PREP_ONLY and
 *       GTA_FLAG_KV_READY as in the entries without key_lens; a GTA_FLAG_KV_READY call must come with the key_lens the images were built under.
 *   key_lens == NULL: GTA_E_BADARG.  Every other argument, check and error code: as in gta_attn_fwd / gta_attn_fwd_staged. */
int gta_attn_fwd_varlen_supported(const GtaAttnDesc* desc);
int gta_attn_fwd_varlen(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                        const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                        const float* trans_coeff, const float* tau, const int32_t* key_lens, void* out, float* lse,
                        void* workspace, int64_t workspace_bytes, void* stream);
int gta_attn_fwd_staged_varlen_supported(const GtaAttnDesc* desc);
int gta_attn_fwd_staged_varlen(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                               const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                               const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau,
                               const int32_t* key_lens, void* out, float* lse, void* workspace, int64_t workspace_bytes, void* stream);

/* Any per-scene subset of the key tokens (gta_attention's key_mask): scene b attends over the key_lens[b] tokens
 * key_idx[b, 0 .. key_lens[b]) names, in any order (softmax attention does not depend on the order of its keys).  The pre-pass compacts
 * them: image row r of tile j of scene b is built from token key_idx[b, 64 j + r], with that token's K / V row, cs_k row and view record;
 * the attention step is the VARLEN gta_fwd2_kernel of gta_attn_fwd_varlen under the same key_lens, and what that entry says of its
 * workspace (sized by Tk, the first ceil(key_lens[b] / 64) tiles of a scene's slot written, the rest untouched) holds here.
 *   key_idx: [B, Tk] int32 on the device, token numbers in [0, Tk) (the kernel clamps into that range, so no value moves a load out of the
 *       scene's rows; the Python layer builds them from a mask).  Entries at or past key_lens[b] are never read.  Tokens no index names are
 *       never loaded: their k, v and cs_k rows may hold anything, NaN and Inf included.  NULL: GTA_E_BADARG, unless GTA_FLAG_KV_READY is set
 *       -- the images are there already and key_idx is not read.
 *   key_lens: as in gta_attn_fwd_varlen (NULL: GTA_E_BADARG); a GTA_FLAG_KV_READY call must come with the key_lens the images were built under.
 *   gta_attn_fwd_gather_supported: what gta_attn_fwd_varlen_supported answers.  Forward only; fused layouts only.
 *   Every other argument, check and error code: as in gta_attn_fwd_varlen. */
int gta_attn_fwd_gather_supported(const GtaAttnDesc* desc);
int gta_attn_fwd_gather(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                        const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                        const float* trans_coeff, const float* tau, const int32_t* key_idx, const int32_t* key_lens, void* out, float* lse,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* The same on the staged generic layouts (gta_attention's key_mask with key_mask_generic): gta_attn_fwd_staged_varlen whose pre-pass runs in
 * its GATHER instances.  Image row r of tile j of scene b is built from token tok = key_idx[b, 64 j + r]: its K / V rows, the view record of
 * view tok / P, its cs_k and coord_k rows; under GTA_FLAG_EUCLID its bias -0.5 scale |k'|^2 is stored at the COMPACTED position 64 j + r of
 * (b, h), where the attention step streams it.  Rows at or past key_lens[b] in the last written tile are zero rows with bias 0.0; the tiles
 * past it are not written.  The attention step is the VARLEN gta_gen_attn_kernel as it is.
 *   key_idx, key_lens: as in gta_attn_fwd_gather (either NULL: GTA_E_BADARG; key_idx may be NULL under GTA_FLAG_KV_READY, which does not
 *       read it).  Tokens no index names are never loaded: their k, v, cs_k and coord_k rows may hold anything, NaN and Inf included; the
 *       vrep_k record of a view without a named token is never read.
 *   gta_attn_fwd_staged_gather_supported: what gta_attn_fwd_staged_supported answers.  Forward only.
 *   Every other argument, check and error code: as in gta_attn_fwd_staged_varlen. */
int gta_attn_fwd_staged_gather_supported(const GtaAttnDesc* desc);
int gta_attn_fwd_staged_gather(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                               const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                               const float* coord_q, const float* coord_k, const float* trans_coeff, const float* tau,
                               const int32_t* key_idx, const int32_t* key_lens, void* out, float* lse,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* A query-side mask beside the key mask (gta_attention's query_mask): gta_attn_fwd_gather whose attention step runs in the QMASK twins of the
 * VARLEN gta_fwd2_kernel instances (every layout, head size and input type those exist for; one workgroup per work item).
 *   q_live: [B, Tq] uint8 on the device (the storage of a bool tensor), non-zero = the query row is live.  NULL: GTA_E_BADARG.
 *   A row (b, t) is live iff q_live[b, t] is set.  A dead row is never used: its q row, its cs_q row and the vrep_q record of a view without a
 *       live row may hold anything, NaN and Inf included (the rows are loaded -- they must be readable memory -- and struck behind rho_q;
 *       vrep_q records are loaded with the others and must be readable memory too).  A dead row is written as zeros: out = +0.0 in every
 *       channel and lse = +0.0, so a later gta_attn_merge of such rows stays finite.  A scene may have no live row.
 *   A 128-row work item without a live row stores those zeros and ends before it requests a key tile or loads a query row; in a live item
 *       a dead row is computed as the row q' = 0 (to the wave-wide decisions of the lazy softmax it is the row a zero q row gives: the live
 *       rows' out and lse are bit for bit those of gta_attn_fwd_gather on the same data with the dead q rows set to zero).
 *   GTA_FLAG_PREP_ONLY: GTA_E_BADARG (the pre-pass knows no query mask: gta_attn_fwd_gather builds the images).  GTA_FLAG_KV_READY: as in
 *       gta_attn_fwd_gather.
 *   gta_attn_fwd_qmask_supported: what gta_attn_fwd_gather_supported answers.
 *   Every other argument, check and error code: as in gta_attn_fwd_gather. */
int gta_attn_fwd_qmask_supported(const GtaAttnDesc* desc);
int gta_attn_fwd_qmask(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                       const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                       const float* trans_coeff, const float* tau, const int32_t* key_idx, const int32_t* key_lens,
                       const uint8_t* q_live, void* out, float* lse,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* The backward of gta_attn_fwd_qmask (gta_attention's query_mask with key_mask_backward): gta_attn_bwd_gather with a query-side mask.  The
 * q-side pre-pass and the dQ walk run in QMASK instances; the dK/dV walk is the GATHER one as it is, under q_lens.
 *   q_live: as in gta_attn_fwd_qmask; NULL: GTA_E_BADARG.
 *   q_lens: [B] int32 on the device, 1 + the index of scene b's last live row (0 for a scene without one; the kernels clamp it to 1), or
 *       NULL = Tq.  It lets the dK/dV walk skip the query tiles behind the last live row; a larger value costs time, not correctness.
 *   A row (b, t) is live iff t < q_lens[b] and q_live[b, t] is set.  A dead row is never used: its q, cs_q, out, dout and lse entries may hold
 *       anything, NaN and Inf included, and so may the vrep_q record of a view without a live row (records are loaded with the others and
 *       must be readable memory).  Its dq row is written as +0.0 in every channel, and it adds nothing to dk, dv, dtrans_coeff or dtau: its
 *       rows of the Q'' / dO~ images are zero and its statistics (-1e30, 0), so P = 0 and dS = 0 for it in both walks.  A 128-row block of
 *       the dQ walk without a live row stores zeros and ends.  Every output is bit for bit that of gta_attn_bwd_gather on the same data with
 *       the dead rows of q and dout set to zero (dq at the live rows).
 *   gta_attn_bwd_qmask_supported: what gta_attn_bwd_gather_supported answers.
 *   Every other argument, check and error code: as in gta_attn_bwd_gather. */
int gta_attn_bwd_qmask_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_qmask(const GtaAttnDesc* desc,
                       const void* q, const void* k, const void* v, const void* out, const void* dout,
                       const float* lse,
                       const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                       const float* trans_coeff, const float* tau,
                       const int32_t* key_idx, const int32_t* key_lens, const uint8_t* q_live, const int32_t* q_lens,
                       const void* kv_images,
                       void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                       float* dtrans_coeff, float* dtau,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* The masked backwards of the PAIR (out, lse) (gta_attention's masked_lse_backward): gta_attn_bwd_varlen, gta_attn_bwd_gather and
 * gta_attn_bwd_qmask with the gradient of the log-sum-exp, as gta_attn_bwd_dlse relates to gta_attn_bwd.
 *   dlse: [B,H,Tq] fp32, contiguous, non-NULL (GTA_E_BADARG, "null dlse") -- d loss / d lse per query row.  The q-side pre-pass runs in the
 *       DLSE twin of the base entry's instance: a live row stores -(D - dlse) where the base stores -D; the Q'' / dO~ images, the lse half of
 *       the statistics and every walk are the base entry's.  An all-zero dlse gives every output bit for bit that of the base entry.
 *   A dead row -- at or past q_lens[b], or with its byte of q_live clear -- stores (-1e30, 0) as in the base entry, and its dlse is never
 *       loaded: like its dout it may hold anything, NaN and Inf included (gta_attn_merge_bwd writes dlse_i = a_i (dlse + <dout, out_i - out>)
 *       on exactly those rows).
 *   *_dlse_supported: what the base entry's query answers.  Every other argument, check, workspace size and error code: as in the base entry. */
int gta_attn_bwd_varlen_dlse_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_varlen_dlse(const GtaAttnDesc* desc,
                             const void* q, const void* k, const void* v, const void* out, const void* dout,
                             const float* lse, const float* dlse,
                             const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                             const float* trans_coeff, const float* tau,
                             const int32_t* key_lens, const int32_t* q_lens,
                             const void* kv_images,
                             void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                             float* dtrans_coeff, float* dtau,
                             void* workspace, int64_t workspace_bytes, void* stream);
int gta_attn_bwd_gather_dlse_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_gather_dlse(const GtaAttnDesc* desc,
                             const void* q, const void* k, const void* v, const void* out, const void* dout,
                             const float* lse, const float* dlse,
                             const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                             const float* trans_coeff, const float* tau,
                             const int32_t* key_idx, const int32_t* key_lens,
                             const void* kv_images,
                             void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                             float* dtrans_coeff, float* dtau,
                             void* workspace, int64_t workspace_bytes, void* stream);
int gta_attn_bwd_qmask_dlse_supported(const GtaAttnDesc* desc);
int gta_attn_bwd_qmask_dlse(const GtaAttnDesc* desc,
                            const void* q, const void* k, const void* v, const void* out, const void* dout,
                            const float* lse, const float* dlse,
                            const float* vrep_q, const float* vrep_k, const float* cs_q, const float* cs_k,
                            const float* trans_coeff, const float* tau,
                            const int32_t* key_idx, const int32_t* key_lens, const uint8_t* q_live, const int32_t* q_lens,
                            const void* kv_images,
                            void* dq, void* dk, void* dv, const int64_t* dqkv_stride, const int64_t* dout_stride,
                            float* dtrans_coeff, float* dtau,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* What the masked entries above read, built from the masks in one launch (gta_maskidx.hip; gta_amd.mask_index): one 256-thread workgroup
 * per (scene, side), no workspace, no atomics (every output element has one writer), nothing read back by the host.
 *   key_mask: [B, Tk] uint8 on the device (the storage of a contiguous bool tensor), non-zero = the key token is live; or NULL.
 *   query_mask: [B, Tq] uint8 on the device, non-zero = the query row is live; or NULL.  It may be key_mask itself (then Tq = Tk).  It is
 *       what the entries above take as q_live, as it is: nothing is written for it but q_lens.
 *   key_idx: [B, Tk] int32, written whole: row b is a permutation of [0, Tk), scene b's live tokens in ascending order, then its masked
 *       tokens in ascending order (the indices of a stable sort of the negated mask).  gta_attn_bwd_gather walks the whole row.
 *   key_lens: [B] int32, the number of live tokens of scene b, unclamped: 0 for a scene without one (the attention kernels clamp to 1).
 *   k_live: [B, Tk] uint8 or NULL: key_mask as 0 / 1 bytes, with token 0 of a scene without a live token set (the token such a scene
 *       attends over under the clamp; what gta_rep_grad_sums_masked takes as `live` on the key side).
 *   q_lens: [B] int32: 1 + the index of scene b's last live query row, 0 for a scene without one.
 *   Checked before anything touches the device, each GTA_E_BADARG with a gta_strerror text that names the argument: B < 1; both masks
 *       NULL; a given mask with T < 1 (Tk / Tq of an absent side is not read); key_mask without key_idx or key_lens; query_mask without
 *       q_lens.  The outputs of an absent side are not touched. */
int gta_mask_index(const uint8_t* key_mask, int32_t B, int32_t Tk,
                   int32_t* key_idx, int32_t* key_lens, uint8_t* k_live,
                   const uint8_t* query_mask, int32_t Tq, int32_t* q_lens,
                   void* stream);

/* -------------------------------------------------------------------------------------------
 * Gradients of the reps: camera poses and patch coordinates (what autograd over gta.py:134-279 gives the reference's
 * se3rep / inv_se3rep / so2rep / t2rep tensors; the Wigner-D blocks stay detached, gta.py:194-197,267).  A pass after the
 * backward, run only when a table needs a gradient: segmented outer-product sums
 *     S = sum a b^T    over heads, the channel groups of a slab and (se3) the tokens of a view,
 * of n_pairs (1 or 2) pairs (a, b) of [B,H,T,dh] tensors of desc->dtype through their (b,h,t) element strides (channel stride 1);
 * T, N = Tq, Nq (side 0) or Tk, Nk (side 1).  Outputs (fp32, row-major, written -- not accumulated; NULL = not wanted, and then its
 * slab's channels are not read):
 *   view_sums [B, N, 4, 4]        se3 slab, 4-channel groups; under GTA_FLAG_EUCLID 3-channel groups with b homogenised by a
 *                                 constant 1 (rows 0..2, columns 0..3; row 3 is zero);
 *   so2_sums  [B, T, d_so2/2, 2, 2] per token and so2 block;
 *   t2_sums   [B, T, 3, 3]        per token, over the t2 slab's 3-channel groups.
 * The small-matrix algebra that turns the sums into d(table) is the caller's (gta_amd/repgrad.py).
 * view_sums need a workspace of >= gta_rep_grad_workspace_bytes(desc, side) bytes (per-workgroup partials; a negative return is
 * an error code).  Deterministic: no float atomics, fixed-order reductions.  Only desc->{abi_version, dtype, B, H, Tq/Tk, Nq/Nk,
 * dh, d_*, flags & GTA_FLAG_EUCLID} are read.
 * ------------------------------------------------------------------------------------------- */
int64_t gta_rep_grad_workspace_bytes(const GtaAttnDesc* desc, int32_t side);
int gta_rep_grad_sums(const GtaAttnDesc* desc, int32_t side, int32_t n_pairs,
                      const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                      const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                      float* view_sums, float* so2_sums, float* t2_sums,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* The sums with per-scene prefixes (the pass after gta_attn_bwd_varlen): gta_rep_grad_sums over the rows of the prefix alone.
 *   lens: [B] int32 on the device, valid TOKENS of this side per scene (key_lens for side 1, q_lens for side 0), clamped to 1..T as in
 *       gta_attn_bwd_varlen; NULL: GTA_E_BADARG.  A row (b, h, t) with t >= lens[b] is dead: none of its operands is loaded, in either
 *       pair (it may hold anything, NaN and Inf included), and it adds exact zero to every sum.  The Python layer passes whole views.
 *   Every requested output is written whole: per-token sums of dead tokens and the view sums of wholly dead views are +0.0 (all bits
 *       zero).  A workgroup whose tokens all lie at or past the prefix loads nothing: padded views are skipped, not summed and dropped.
 *   Live entries are bit for bit those of gta_rep_grad_sums on the same buffers (the VARLEN twin of the instance it selects: the same
 *       thread-to-row map, pair and group order, tree, head order and finish order).
 *   Workspace (gta_rep_grad_workspace_bytes serves both entries), every other argument, check and error code: as in gta_rep_grad_sums. */
int gta_rep_grad_sums_varlen(const GtaAttnDesc* desc, int32_t side, int32_t n_pairs,
                             const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                             const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                             const int32_t* lens, float* view_sums, float* so2_sums, float* t2_sums,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* The sums under a per-token mask (the pass after gta_attn_bwd_gather / gta_attn_bwd_qmask): gta_rep_grad_sums over the live rows alone.
 *   live: [B, T] uint8 on the device, one byte per token of this side, non-zero = live; NULL: GTA_E_BADARG.
 *   Never-read: a row (b, h, t) with live[b * T + t] == 0 is dead: none of its operands is loaded, in either pair (it may hold anything,
 *       NaN and Inf included), and it adds exact zero to every sum.
 *   Dead-zero: every requested output is written whole: per-token sums of dead tokens and the view sums of views without a live token
 *       are +0.0 (all bits zero).  A scene without a live token is legal: everything it owns is +0.0.
 *   Live-equal: every output word is bit for bit that of gta_rep_grad_sums on the same operands with the dead rows set to zero (the MASKED
 *       twin of the instance it selects: the same thread-to-row map, pair and group order, tree, head order and finish order); under
 *       a mask that is a prefix of every scene it is the word of gta_rep_grad_sums_varlen with those counts.
 *   Dead workgroups: a workgroup (256 / H tokens of one view) none of whose tokens is live loads nothing, writes +0.0 to what it owns and
 *       returns.  That is decided uniformly, by one OR over the whole workgroup -- never from its first token: a workgroup whose first
 *       token is dead and a later one live is a live workgroup.
 *   Workspace (gta_rep_grad_workspace_bytes serves all three entries), every other argument, check and error code: as in
 *       gta_rep_grad_sums. */
int gta_rep_grad_sums_masked(const GtaAttnDesc* desc, int32_t side, int32_t n_pairs,
                             const void* a0, const int64_t* a0_stride, const void* b0, const int64_t* b0_stride,
                             const void* a1, const int64_t* a1_stride, const void* b1, const int64_t* b1_stride,
                             const uint8_t* live, float* view_sums, float* so2_sums, float* t2_sums,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* softmax((scale * q k^T + key_bias) / tau) v with no rep at all (the fused kernel on an identity layout).
 * key_bias: [B,H,bias_pitch] fp32, added to scale*q.k BEFORE the division by tau; bias_pitch a multiple of 64 >= Tk; or NULL.
 * Only desc->{dtype,B,H,Tq,Tk,dh,scale,*_stride} are read. */
int gta_attn_fwd_plain(const GtaAttnDesc* desc, const void* q, const void* k, const void* v,
                       const float* key_bias, int64_t bias_pitch, const float* tau,
                       void* out, float* lse, void* stream);

/* -------------------------------------------------------------------------------------------
 * fp32-FAITHFUL backward of plain attention (identity layout, fp32 tensors): the gradient leg of the accuracy mode for the
 * reference's `mixed_prec: False` configs (runs/clevrtr/GTA/gta/config.yaml:55).  q', k', v' (pre-transformed by gta_rep_apply),
 * o~ and lse from gta_attn_fwd_plain (GTA_FLAG_FP32_PRODUCTS), do~ from gta_rep_apply_bwd(mode 2) -> dq', dk', dv' for
 * gta_rep_apply_bwd(modes 0 / 1).  Exact fp32 products and accumulation (v_mfma_f32_32x32x2_f32 = an fmaf chain), 1/16 of the bf16
 * matrix rate: accuracy, not speed.  desc: dtype F32, dh % 8 == 0 (<= 128), strides of q / k / v / out in elements (multiples of
 * 4); dout_stride[3], dqkv_stride[9] as in gta_attn_bwd; workspace >= gta_attn_bwd_plain_f32_workspace_bytes (B H Tq floats).
 * ------------------------------------------------------------------------------------------- */
int64_t gta_attn_bwd_plain_f32_workspace_bytes(const GtaAttnDesc* desc);
int gta_attn_bwd_plain_f32(const GtaAttnDesc* desc, const void* q, const void* k, const void* v, const void* out,
                           const void* dout, const int64_t* dout_stride, const float* lse, const float* tau,
                           void* dq, void* dk, void* dv, const int64_t* dqkv_stride, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* 0 when gta_attn_fwd has a fused kernel for this desc, else the error it would return. */
int gta_attn_fwd_supported(const GtaAttnDesc* desc);

/* bytes of LDS / number of workgroups the fused forward uses for desc (diagnostics). */
int gta_attn_fwd_launch_info(const GtaAttnDesc* desc, int32_t* lds_bytes, int32_t* n_workgroups,
                             int32_t* threads_per_wg);

/* Profiling hooks (diagnostics; bench.py and tools/ use them, no product path does):
 *   gta_debug_time_next_attention_kernel: the next attention-kernel launch made by THIS thread through gta_attn_fwd is
 *     bracketed by the two events through the dispatch packet itself (hipExtLaunchKernelGGL), i.e. without the marker
 *     packets of hipEventRecord that push neighbouring kernels apart.  One-shot.
 *   gta_debug_event_*: thin wrappers so a ctypes caller needs no second HIP binding.
 *   gta_debug_profile_next_attention_kernel: device buffer [capacity_items][8] of uint64 (or NULL): the NEXT attention kernel launched
 *       by THIS thread through gta_attn_fwd writes, per work item, [0] / [4] = s_memtime at its start / end (shader cycles) and
 *       [5] / [6] = s_memrealtime (100 MHz) -- kernel cycles and the granted shader clock of a launch follow from them; gta_fwd2_kernel
 *       also writes [1] = HW_ID | XCC_ID << 32 of the item's first wave (which CU it ran on: tools/wg_timeline.py); -DGTA_ABLATE
 *       builds write per-phase stamps to [1], [2], [3], [7] instead.  One-shot and thread-local; a launch with more work items than capacity_items writes nothing.
 *   gta_debug_attention_kernel: name of the attention kernel a workspace call of gta_attn_fwd launches for desc, its number of
 *       work items and query rows per item ("" if desc is not supported). */
void gta_debug_time_next_attention_kernel(void* start_event, void* stop_event);
void* gta_debug_event_create(void);
void gta_debug_event_destroy(void* event);
float gta_debug_event_elapsed_ms(void* start_event, void* stop_event);
void gta_debug_profile_next_attention_kernel(void* device_buffer, int64_t capacity_items);
const char* gta_debug_attention_kernel(const GtaAttnDesc* desc, int32_t* n_items, int32_t* rows_per_item);

const char* gta_strerror(int code);
int gta_abi_version(void);
int gta_sizeof_attn_desc(void);   /* sizeof(GtaAttnDesc) as compiled: binding self-check */

#ifdef __cplusplus
}
#endif
#endif /* GTA_HIP_H */
