// gta_repgrad.hip -- gradients of the rep tables (camera poses, patch coordinates): a pass after the attention backward that only
// runs when a table requires a gradient.  Segmented outer-product sums  S = sum a b^T  over the channel groups of the se3 / so2 / t2
// slabs of up to two (a, b) pairs of [B,H,T,dh] tensors (strided rows, unit channel stride), accumulated in fp32 and reduced
//   per view  (se3: 4x4; euclid: 3x4 with b homogenised by a constant 1)  over heads, the view's tokens and the slab's groups,
//   per token (so2: 2x2 per block; t2: 3x3)                                over heads (and the t2 slab's groups).
// gta_amd/repgrad.py maps the sums to d vrep / d cs / d coord.  One thread per (token, head) row, a workgroup
// holds 256 / H tokens of one view, so the per-view sums are split over P * H / 256 workgroups (1280 at the headline shape, 160 views).
// Only the channels of the requested slabs are read.  No float atomics: per-token sums are finished inside the workgroup in head order,
// per-view sums leave one partial per workgroup and gta_repgrad_finish_kernel adds them in workgroup order -- two runs, same bits.
// With per-scene prefixes (gta_rep_grad_sums_varlen, batches that mix view counts) the VARLEN twins skip what lies past a scene's prefix.
// With a per-token liveness byte (gta_rep_grad_sums_masked, key / query masks) the MASKED twins skip every dead row, wherever it lies.
#include "gta_common.h"
#include "gta_repgrad_params.h"
#include "../../include/gta_hip.h"

namespace {

constexpr int NT = GTA_REPGRAD_THREADS;
constexpr int SO2_PASS = 8;                   // so2 blocks whose per-row sums share the LDS at a time (8 x 4 x 256 floats = 32 KiB)

template <int ESZ> GTA_DEV float ld(const char* p, int i) {
    if (ESZ == 4) return reinterpret_cast<const float*>(p)[i];
    return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
}

// channels [ch, ch + 8) of a row as fp32: one 16-byte load for bf16, two for fp32 (VEC instances: 8-channel aligned slabs and rows)
template <int ESZ> GTA_DEV void ld8(const char* p, int ch, float* x) {
    if (ESZ == 2) {
        unpack8(*reinterpret_cast<const u32x4_t*>(p + ch * 2), x);
    } else {
        const float4 a = *reinterpret_cast<const float4*>(p + ch * 4), b = *reinterpret_cast<const float4*>(p + ch * 4 + 16);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    }
}

// sum of red[k][tl * H + h] over the heads h of token tl, in head order
GTA_DEV float head_sum(const float* red, int k, int tl, int H) {
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += red[k * NT + tl * H + h];
    return s;
}

// VARLEN (gta_rep_grad_sums_varlen): a row at or past its scene's prefix p.lens[b] is dead -- never loaded, exact zero in every sum; a
// workgroup wholly past the prefix writes +0.0 to its partial and to its per-token outputs and returns (uniform over the workgroup).
// What is live runs the statements of the instance without VARLEN in the same order: the same bits.
// MASKED (gta_rep_grad_sums_masked; the instances with the trailing `const uint8_t*`): a row is live when its token's byte of p.live
// [B, T] is non-zero -- the same never-read / exact-zero rule per row.  A workgroup is dead when NONE of its ntok tokens is live, decided
// by one OR over the workgroup (a ballot per wave, the four words through the LDS): its first token says nothing about the others.
template <int ESZ, bool EUCLID, bool VEC, bool VARLEN = false, typename... LIVE>
__global__ __launch_bounds__(NT) void gta_repgrad_kernel(const GtaRepGradParams p) {
    constexpr bool MASKED = sizeof...(LIVE) == 1;
    static_assert(sizeof...(LIVE) <= 1 && !(MASKED && VARLEN), "a launch has prefixes or a mask, not both");
    __shared__ float red[SO2_PASS * 4 * NT];
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    const int vb = wg / p.chunks, c = wg % p.chunks;          // vb = b * N + n
    const int b = vb / p.N, n = vb % p.N;
    const int h = tid % p.H, tl = tid / p.H;
    const int t0 = n * p.P + c * p.tpb;                        // first token of the workgroup
    const int ntok = min(p.tpb, p.P - c * p.tpb);
    int nlive = ntok;                                          // tokens of the workgroup whose rows are loaded
    if (VARLEN) {
        const int len = min(max(p.lens[b], 1), p.T);           // valid tokens of scene b, clamped to 1..T
        if (t0 >= len) {                                       // a dead workgroup: nothing loaded, every word it owns is +0.0
            if (p.n_se3 > 0 && tid < 16) p.part[(long)wg * 16 + tid] = 0.f;
            for (int e = tid; e < ntok * p.n_so2 * 4; e += NT) p.so2_out[(long)(b * p.T + t0) * p.n_so2 * 4 + e] = 0.f;
            if (p.n_t2 > 0)
                for (int e = tid; e < ntok * 9; e += NT) p.t2_out[(long)(b * p.T + t0) * 9 + e] = 0.f;
            return;
        }
        nlive = min(ntok, len - t0);                           // a workgroup that straddles the prefix: its tail adds zeros
    }
    bool live = tl < nlive;
    if (MASKED) {
        live = tl < ntok && p.live[(long)b * p.T + t0 + tl] != 0;
        uint32_t* any = reinterpret_cast<uint32_t*>(red);
        const unsigned long long wave_live = __ballot(live);
        if (tid % 64 == 0) any[tid / 64] = wave_live != 0ull;
        __syncthreads();
        uint32_t wg_live = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) wg_live |= any[w];
        if (!wg_live) {                                        // a dead workgroup (uniform): nothing loaded, every word it owns is +0.0
            if (p.n_se3 > 0 && tid < 16) p.part[(long)wg * 16 + tid] = 0.f;
            for (int e = tid; e < ntok * p.n_so2 * 4; e += NT) p.so2_out[(long)(b * p.T + t0) * p.n_so2 * 4 + e] = 0.f;
            if (p.n_t2 > 0)
                for (int e = tid; e < ntok * 9; e += NT) p.t2_out[(long)(b * p.T + t0) * 9 + e] = 0.f;
            return;
        }
        __syncthreads();                                       // (red is the reduction array from here on)
    }
    const int t = t0 + (live ? tl : 0);
    const char* ar[2];
    const char* br[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ar[i] = (const char*)p.a[i] + ((long)b * p.as[i][0] + (long)h * p.as[i][1] + (long)t * p.as[i][2]) * ESZ;
        br[i] = (const char*)p.b[i] + ((long)b * p.bs[i][0] + (long)h * p.bs[i][1] + (long)t * p.bs[i][2]) * ESZ;
    }

    if (p.n_se3 > 0) {                                         // per-view 4x4 (3x4) sums -> one partial per workgroup
        constexpr int W = EUCLID ? 3 : 4;
        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        if (live && VEC && !EUCLID) {                          // two 4-channel groups per 16-byte load
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                if (pr >= p.npairs) break;
                for (int g = 0; g < p.n_se3; g += 2) {
                    float x[8], y[8];
                    ld8<ESZ>(ar[pr], p.off_se3 + g * 4, x);
                    ld8<ESZ>(br[pr], p.off_se3 + g * 4, y);
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[i * 4 + j] += x[4 * u + i] * y[4 * u + j];
                }
            }
        } else if (live) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                if (pr >= p.npairs) break;
                for (int g = 0; g < p.n_se3; ++g) {
                    const int ch = p.off_se3 + g * W;
                    float x[4], y[4];
#pragma unroll
                    for (int i = 0; i < W; ++i) { x[i] = ld<ESZ>(ar[pr], ch + i); y[i] = ld<ESZ>(br[pr], ch + i); }
                    if (EUCLID) { x[3] = 0.f; y[3] = 1.f; }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i * 4 + j] += x[i] * y[j];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) red[k * NT + tid] = acc[k];
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int k = 0; k < 16; ++k) red[k * NT + tid] += red[k * NT + tid + s];
            }
            __syncthreads();
        }
        if (tid < 16) p.part[(long)wg * 16 + tid] = red[tid * NT];
        __syncthreads();
    }

    for (int f0 = 0; f0 < p.n_so2; f0 += SO2_PASS) {          // per-token 2x2 sums of each so2 block, SO2_PASS blocks at a time
        const int nf = min(SO2_PASS, p.n_so2 - f0);
        if (VEC) {                                             // four blocks per 16-byte load (n_so2 % 4 == 0)
#pragma unroll
            for (int u = 0; u < SO2_PASS / 4; ++u) {
                if (4 * u < nf) {
                    float s[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[i] = 0.f;
                    if (live) {
                        const int ch = p.off_so2 + 2 * (f0 + 4 * u);
#pragma unroll
                        for (int pr = 0; pr < 2; ++pr) {
                            if (pr < p.npairs) {
                                float x[8], y[8];
                                ld8<ESZ>(ar[pr], ch, x);
                                ld8<ESZ>(br[pr], ch, y);
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    s[4 * j + 0] += x[2 * j] * y[2 * j];     s[4 * j + 1] += x[2 * j] * y[2 * j + 1];
                                    s[4 * j + 2] += x[2 * j + 1] * y[2 * j]; s[4 * j + 3] += x[2 * j + 1] * y[2 * j + 1];
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) red[(16 * u + i) * NT + tid] = s[i];
                }
            }
        } else {
#pragma unroll
            for (int f = 0; f < SO2_PASS; ++f) {
                if (f < nf) {
                    float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
                    if (live) {
                        const int ch = p.off_so2 + 2 * (f0 + f);
#pragma unroll
                        for (int pr = 0; pr < 2; ++pr) {
                            if (pr < p.npairs) {
                                const float x0 = ld<ESZ>(ar[pr], ch), x1 = ld<ESZ>(ar[pr], ch + 1);
                                const float y0 = ld<ESZ>(br[pr], ch), y1 = ld<ESZ>(br[pr], ch + 1);
                                s00 += x0 * y0; s01 += x0 * y1; s10 += x1 * y0; s11 += x1 * y1;
                            }
                        }
                    }
                    red[(f * 4 + 0) * NT + tid] = s00;
                    red[(f * 4 + 1) * NT + tid] = s01;
                    red[(f * 4 + 2) * NT + tid] = s10;
                    red[(f * 4 + 3) * NT + tid] = s11;
                }
            }
        }
        __syncthreads();
        const int m = ntok * nf * 4;
        for (int e = tid; e < m; e += NT) {
            const int tk = e / (nf * 4), r = e % (nf * 4);
            p.so2_out[((long)(b * p.T + t0 + tk) * p.n_so2 + f0) * 4 + r] = head_sum(red, r, tk, p.H);
        }
        __syncthreads();
    }

    if (p.n_t2 > 0) {                                          // per-token 3x3 sums over the t2 slab's groups
        float acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = 0.f;
        if (live) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                if (pr >= p.npairs) break;
                for (int g = 0; g < p.n_t2; ++g) {
                    const int ch = p.off_t2 + 3 * g;
                    float x[3], y[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) { x[i] = ld<ESZ>(ar[pr], ch + i); y[i] = ld<ESZ>(br[pr], ch + i); }
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) acc[i * 3 + j] += x[i] * y[j];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) red[k * NT + tid] = acc[k];
        __syncthreads();
        const int m = ntok * 9;
        for (int e = tid; e < m; e += NT) {
            const int tk = e / 9, k = e % 9;
            p.t2_out[(long)(b * p.T + t0 + tk) * 9 + k] = head_sum(red, k, tk, p.H);
        }
    }
}

// per-view sums: the workgroups' partials of each view added in workgroup order
__global__ __launch_bounds__(256) void gta_repgrad_finish_kernel(const GtaRepGradParams p) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)p.B * p.N * 16) return;
    const long vb = e / 16;
    const int k = (int)(e % 16);
    float s = 0.f;
    for (int c = 0; c < p.chunks; ++c) s += p.part[(vb * p.chunks + c) * 16 + k];
    p.view_out[e] = s;
}

// the 16-byte form: every operand row 16-byte aligned, se3 / so2 slabs that start and end on 8-channel boundaries (every BASELINE layout)
bool vec_ok(const GtaRepGradParams& p, int esz, bool euclid) {
    for (int i = 0; i < p.npairs; ++i) {
        const void* ptr[2] = {p.a[i], p.b[i]};
        const long* st[2] = {p.as[i], p.bs[i]};
        for (int j = 0; j < 2; ++j) {
            if ((uintptr_t)ptr[j] % 16) return false;
            for (int d = 0; d < 3; ++d)
                if ((st[j][d] * esz) % 16) return false;
        }
    }
    if (p.n_se3 > 0 && (euclid || p.off_se3 % 8 || p.n_se3 % 2)) return false;
    if (p.n_so2 > 0 && (p.off_so2 % 8 || p.n_so2 % 4)) return false;
    return true;
}

// the VARLEN twin of each instance below, selected the same way
void launch_varlen(const GtaRepGradParams& p, int esz, bool euclid, dim3 grid, dim3 block, hipStream_t stream) {
    if (vec_ok(p, esz, euclid)) {
        if (esz == 2) hipLaunchKernelGGL((gta_repgrad_kernel<2, false, true, true>), grid, block, 0, stream, p);
        else          hipLaunchKernelGGL((gta_repgrad_kernel<4, false, true, true>), grid, block, 0, stream, p);
    } else if (esz == 2) {
        if (euclid) hipLaunchKernelGGL((gta_repgrad_kernel<2, true, false, true>), grid, block, 0, stream, p);
        else        hipLaunchKernelGGL((gta_repgrad_kernel<2, false, false, true>), grid, block, 0, stream, p);
    } else {
        if (euclid) hipLaunchKernelGGL((gta_repgrad_kernel<4, true, false, true>), grid, block, 0, stream, p);
        else        hipLaunchKernelGGL((gta_repgrad_kernel<4, false, false, true>), grid, block, 0, stream, p);
    }
}

// the MASKED twin of each instance, selected the same way
void launch_masked(const GtaRepGradParams& p, int esz, bool euclid, dim3 grid, dim3 block, hipStream_t stream) {
    using M = const uint8_t*;
    if (vec_ok(p, esz, euclid)) {
        if (esz == 2) hipLaunchKernelGGL((gta_repgrad_kernel<2, false, true, false, M>), grid, block, 0, stream, p);
        else          hipLaunchKernelGGL((gta_repgrad_kernel<4, false, true, false, M>), grid, block, 0, stream, p);
    } else if (esz == 2) {
        if (euclid) hipLaunchKernelGGL((gta_repgrad_kernel<2, true, false, false, M>), grid, block, 0, stream, p);
        else        hipLaunchKernelGGL((gta_repgrad_kernel<2, false, false, false, M>), grid, block, 0, stream, p);
    } else {
        if (euclid) hipLaunchKernelGGL((gta_repgrad_kernel<4, true, false, false, M>), grid, block, 0, stream, p);
        else        hipLaunchKernelGGL((gta_repgrad_kernel<4, false, false, false, M>), grid, block, 0, stream, p);
    }
}

}  // namespace

// p.live != nullptr selects the MASKED instances (gta_rep_grad_sums_masked refuses a NULL live before it comes here), else
// p.lens != nullptr selects the VARLEN instances (gta_rep_grad_sums_varlen refuses a NULL lens before it comes here)
int gta_repgrad_dispatch(const GtaRepGradParams& p, int esz, bool euclid, hipStream_t stream) {
    const long nwg = (long)p.B * p.N * p.chunks;
    if (nwg <= 0 || nwg > 0x7fffffffL) return GTA_E_UNSUPPORTED;
    const dim3 grid((unsigned)nwg), block(NT);
    if (p.live) {
        launch_masked(p, esz, euclid, grid, block, stream);
    } else if (p.lens) {
        launch_varlen(p, esz, euclid, grid, block, stream);
    } else if (vec_ok(p, esz, euclid)) {
        if (esz == 2) hipLaunchKernelGGL((gta_repgrad_kernel<2, false, true>), grid, block, 0, stream, p);
        else          hipLaunchKernelGGL((gta_repgrad_kernel<4, false, true>), grid, block, 0, stream, p);
    } else if (esz == 2) {
        if (euclid) hipLaunchKernelGGL((gta_repgrad_kernel<2, true, false>), grid, block, 0, stream, p);
        else        hipLaunchKernelGGL((gta_repgrad_kernel<2, false, false>), grid, block, 0, stream, p);
    } else {
        if (euclid) hipLaunchKernelGGL((gta_repgrad_kernel<4, true, false>), grid, block, 0, stream, p);
        else        hipLaunchKernelGGL((gta_repgrad_kernel<4, false, false>), grid, block, 0, stream, p);
    }
    if (p.n_se3 > 0) {
        const long n = (long)p.B * p.N * 16;
        hipLaunchKernelGGL(gta_repgrad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p);
    }
    return hipGetLastError() == hipSuccess ? GTA_OK : GTA_E_LAUNCH;
}
