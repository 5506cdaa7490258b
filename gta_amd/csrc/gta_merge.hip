// gta_merge.hip -- merge of n partial attentions of the same queries over disjoint key sets (gta_attn_merge, gta_attn_merge_bwd).
//
// With a_i = softmax_i(lse_i) per query row:   out = sum_i a_i out_i,   lse = logsumexp_i(lse_i),
// and for the pair (dout, dlse):               dout_i = a_i dout,       dlse_i = a_i (dlse + <dout, out_i - out>).
//
// Both kernels are memory streams: n + 1 (forward) / 2n + 1 (backward) row operands, a few flops per byte (measured:
// profiles/lse_merge/README.md).
//   * one 16-byte unit per lane; a row of dh channels is U = dh * esz / 16 units, held by a lane group of G = the next power of two >= U
//     lanes (lanes U..G-1 idle: at dh = 96, 12 of 16 for bf16 and 24 of 32 for fp32), 256 / G rows per workgroup and step;
//   * rows are walked in MEMORY order of the [B,Tq,H,dh] tensors the attention kernels write (row index = (b Tq + t) H + h): consecutive
//     rows of a contiguous operand are one stream; any other (b, h, t) strides are served, at whatever coalescing they leave;
//   * grid-stride over rows, no LDS; the backward's row dot <dout, out_i - out> is reduced inside the lane group with log2 G exchanges;
//   * pointers and strides of the partials are kernel arguments, indexed by unrolled (constant) i < 8 only: scalar loads, no scratch;
//   * arithmetic in fp32, one rounding to the operands' dtype.  A partial whose lse_i is -inf on a row (an empty key set; also one whose
//     weight underflows to 0) is SELECTED out: its out_i row enters no arithmetic, so it may hold anything, NaN included (the row is still
//     loaded, with every other operand of the step and before the weights are known: one memory round trip per step, not two); its dout_i
//     row and dlse_i are exact zeros.  A row whose lse_i are all -inf gives out = 0, lse = -inf and zero gradients.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gta_common.h"
#include "gta_merge_params.h"
#include "../../include/gta_hip.h"

namespace {

template <int ESZ>
GTA_DEV void unit_load(const char* src, float* x) {        // 16 bytes -> 16 / ESZ floats
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(src);
    if constexpr (ESZ == 2) {
        unpack8(w, x);
    } else {
        x[0] = __uint_as_float(w.x); x[1] = __uint_as_float(w.y); x[2] = __uint_as_float(w.z); x[3] = __uint_as_float(w.w);
    }
}
template <int ESZ>
GTA_DEV void unit_store(char* dst, const float* x) {
    u32x4_t w;
    if constexpr (ESZ == 2) {
        w = pack8(x);
    } else {
        w.x = __float_as_uint(x[0]); w.y = __float_as_uint(x[1]); w.z = __float_as_uint(x[2]); w.w = __float_as_uint(x[3]);
    }
    *reinterpret_cast<u32x4_t*>(dst) = w;
}

// the lane's place in a step: row g of the workgroup's 256 >> lg rows, unit u of the row's G = 1 << lg (U of them real)
struct MergeMap {
    int U, lg, u, g, rpb;
};
template <int ESZ>
GTA_DEV MergeMap merge_map(int dh) {
    MergeMap m;
    m.U = dh * ESZ / 16;
    m.lg = m.U > 1 ? 32 - __builtin_clz((unsigned)(m.U - 1)) : 0;
    m.u = threadIdx.x & ((1 << m.lg) - 1);
    m.g = threadIdx.x >> m.lg;
    m.rpb = 256 >> m.lg;
    return m;
}
GTA_DEV long row_off(const long* st, int b, int h, int t) { return (long)b * st[0] + (long)h * st[1] + (long)t * st[2]; }

#define GTA_NEG_INF (-__builtin_inff())

// weights of a row from its n log-sum-exps: w_i = exp(lse_i - max) (0 where lse_i = -inf), their sum s and the maximum m
#define GTA_MERGE_WEIGHTS(P, ROW_OK)                                                                    \
    float l[GTA_MERGE_MAX], w[GTA_MERGE_MAX], m = GTA_NEG_INF, s = 0.f;                                 \
    _Pragma("unroll") for (int i = 0; i < GTA_MERGE_MAX; ++i) {                                         \
        l[i] = GTA_NEG_INF;                                                                             \
        if (i < (P).n) {                                                                                \
            if (ROW_OK) l[i] = (P).lses[i][row_off((P).lses_st[i], b, h, t)];                           \
            m = fmaxf(m, l[i]);                                                                         \
        }                                                                                               \
    }                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < GTA_MERGE_MAX; ++i) {                                         \
        w[i] = (i < (P).n && l[i] != GTA_NEG_INF) ? __expf(l[i] - m) : 0.f;                             \
        s += w[i];                                                                                      \
    }                                                                                                   \
    const float inv_s = s > 0.f ? 1.0f / s : 0.f;

template <int ESZ>
__global__ __launch_bounds__(256) void gta_merge_kernel(const GtaMergeParams p) {
    constexpr int E = 16 / ESZ;
    const MergeMap mp = merge_map<ESZ>(p.dh);
    const long R = (long)p.B * p.Tq * p.H;
    for (long r0 = (long)blockIdx.x * mp.rpb; r0 < R; r0 += (long)gridDim.x * mp.rpb) {
        const bool row_ok = r0 + mp.g < R;
        if (!(row_ok && mp.u < mp.U)) continue;
        const int r = (int)(r0 + mp.g);
        const int h = r % p.H, bt = r / p.H, t = bt % p.Tq, b = bt / p.Tq;
        // the row units of every partial first, then the log-sum-exps (independent loads: all in flight together), then the arithmetic
        float x[GTA_MERGE_MAX][E];
#pragma unroll
        for (int i = 0; i < GTA_MERGE_MAX; ++i)
            if (i < p.n) unit_load<ESZ>((const char*)p.outs[i] + row_off(p.outs_st[i], b, h, t) * ESZ + mp.u * 16, x[i]);
        GTA_MERGE_WEIGHTS(p, true)
        float acc[E];
        bool first = true;
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = 0.f;
#pragma unroll
        for (int i = 0; i < GTA_MERGE_MAX; ++i)
            if (i < p.n && w[i] > 0.f) {
                const float a = w[i] * inv_s;
                // (the first live partial starts the sum as a product: a lone partial comes back bit for bit, -0 included)
#pragma unroll
                for (int c = 0; c < E; ++c) acc[c] = first ? a * x[i][c] : __builtin_fmaf(a, x[i][c], acc[c]);
                first = false;
            }
        unit_store<ESZ>((char*)p.out + row_off(p.out_st, b, h, t) * ESZ + mp.u * 16, acc);
        if (mp.u == 0) p.lse[row_off(p.lse_st, b, h, t)] = s > 0.f ? (s == 1.0f ? m : m + __logf(s)) : GTA_NEG_INF;
    }
}

template <int ESZ>
__global__ __launch_bounds__(256) void gta_merge_bwd_kernel(const GtaMergeBwdParams p) {
    constexpr int E = 16 / ESZ;
    const MergeMap mp = merge_map<ESZ>(p.dh);
    const long R = (long)p.B * p.Tq * p.H;
    // (every lane of the workgroup takes every step: the lane-group exchanges below are executed by all 64 lanes of a wave)
    for (long r0 = (long)blockIdx.x * mp.rpb; r0 < R; r0 += (long)gridDim.x * mp.rpb) {
        const bool row_ok = r0 + mp.g < R;
        const bool act = row_ok && mp.u < mp.U;
        const int r = row_ok ? (int)(r0 + mp.g) : (int)(R - 1);
        const int h = r % p.H, bt = r / p.H, t = bt % p.Tq, b = bt / p.Tq;
        float dO[E], o[E], x[GTA_MERGE_MAX][E];
#pragma unroll
        for (int c = 0; c < E; ++c) { dO[c] = 0.f; o[c] = 0.f; }
        if (act) unit_load<ESZ>((const char*)p.dout + row_off(p.dout_st, b, h, t) * ESZ + mp.u * 16, dO);
#pragma unroll
        for (int i = 0; i < GTA_MERGE_MAX; ++i) {
#pragma unroll
            for (int c = 0; c < E; ++c) x[i][c] = 0.f;
            if (i < p.n && act) unit_load<ESZ>((const char*)p.outs[i] + row_off(p.outs_st[i], b, h, t) * ESZ + mp.u * 16, x[i]);
        }
        const float g_lse = (p.dlse && row_ok) ? p.dlse[row_off(p.dlse_st, b, h, t)] : 0.f;
        GTA_MERGE_WEIGHTS(p, row_ok)
#pragma unroll
        for (int i = 0; i < GTA_MERGE_MAX; ++i)          // a partial without keys on this row: whatever its row holds (NaN) is dropped here
            if (!(w[i] > 0.f)) {
#pragma unroll
                for (int c = 0; c < E; ++c) x[i][c] = 0.f;
            }
#pragma unroll
        for (int i = 0; i < GTA_MERGE_MAX; ++i)
            if (i < p.n) {
                const float a = w[i] * inv_s;
#pragma unroll
                for (int c = 0; c < E; ++c) o[c] = __builtin_fmaf(a, x[i][c], o[c]);
            }
#pragma unroll
        for (int i = 0; i < GTA_MERGE_MAX; ++i)
            if (i < p.n) {                                   // (uniform over the grid)
                const float a = w[i] * inv_s;
                float dot = 0.f;
#pragma unroll
                for (int c = 0; c < E; ++c) dot = __builtin_fmaf(dO[c], x[i][c] - o[c], dot);
                for (int off = (1 << mp.lg) >> 1; off; off >>= 1) dot += __shfl_xor(dot, off);
                if (act) {
                    float d[E];
#pragma unroll
                    for (int c = 0; c < E; ++c) d[c] = w[i] > 0.f ? a * dO[c] : 0.f;
                    unit_store<ESZ>((char*)p.douts[i] + row_off(p.douts_st[i], b, h, t) * ESZ + mp.u * 16, d);
                    if (mp.u == 0) p.dlses[i][row_off(p.dlses_st[i], b, h, t)] = w[i] > 0.f ? a * (g_lse + dot) : 0.f;
                }
            }
    }
}

// rows fit an int (the kernels divide the row index); 256 >> lg rows per workgroup and step, at most 8 workgroups per CU of work in flight
// (the cap of 2048 workgroups sizes the rows of test_merge_past_the_grid_cap, tests/test_gpu_lse_merge.py)
template <class P>
long merge_grid(const P& p, int esz) {
    const long R = (long)p.B * p.Tq * p.H;
    if (R > 0x7fffffffL - 256) return -1;
    const int U = p.dh * esz / 16;
    int G = 1;
    while (G < U) G <<= 1;
    const long rpb = 256 / G, blocks = (R + rpb - 1) / rpb;
    return blocks < 2048 ? blocks : 2048;
}

}  // namespace

int gta_merge_dispatch(const GtaMergeParams& p, int esz, hipStream_t stream) {
    const long grid = merge_grid(p, esz);
    if (grid < 0) return GTA_E_UNSUPPORTED;
    if (esz == 2) hipLaunchKernelGGL((gta_merge_kernel<2>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((gta_merge_kernel<4>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? GTA_OK : GTA_E_LAUNCH;
}

int gta_merge_bwd_dispatch(const GtaMergeBwdParams& p, int esz, hipStream_t stream) {
    const long grid = merge_grid(p, esz);
    if (grid < 0) return GTA_E_UNSUPPORTED;
    if (esz == 2) hipLaunchKernelGGL((gta_merge_bwd_kernel<2>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((gta_merge_bwd_kernel<4>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? GTA_OK : GTA_E_LAUNCH;
}
