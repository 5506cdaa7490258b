// gta_rep_row.h -- rho of ANY f_dims layout applied to ONE (batch, head, token) row in fp32: the per-row transform of the generic path
// (gta_apply.hip: gta_rep_apply) and of the staged generic forward (gta_fwd_gen.hip), one copy for both.
//   mode 0: q side      q' = blockdiag((E_q.m)^T | D(R_q) | R(th_q) | (T_q^-1)^T) q      (euclid: affine inv(E_q).m)
//   mode 1: k side      k' = blockdiag(inv(E_k).m | D(R_k) | R(th_k) | T_k) k  (also v)  (euclid: affine inv(E_k).m)
//   mode 2: output      o  = blockdiag(E_q.m | D(R_q)^T | R(th_q)^T | T_q^-1) o~        (euclid: affine E_q.m)
// Everything has internal linkage (anonymous namespace): each .hip is its own module.
#pragma once
#include "gta_common.h"
#include "../../include/gta_hip.h"

namespace {

struct ApplyParams {
    const void* x; void* y;
    long x_sb, x_sh, x_st, y_sb, y_sh, y_st;
    const float *vrep, *cs, *coord, *trans_coeff;
    float* key_bias; float bias_scale; long bias_pitch;
    int B, H, T, N, P;
    int d_triv, d_se3, d_so3, d_so2, d_t2, L;
    int mode, euclid, esz;
};

template <int ESZ> GTA_DEV float ld(const char* p, int i) {
    if (ESZ == 4) return reinterpret_cast<const float*>(p)[i];
    return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16);
}
template <int ESZ> GTA_DEV void st(char* p, int i, float v) {
    if (ESZ == 4) { reinterpret_cast<float*>(p)[i] = v; return; }
    reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)(pack_bf16x2(v, 0.f) & 0xffffu);
}
// a row as the bodies below see it: element ch in, element ch out -- in global memory (direct form) or as fp32 in the wave's LDS stage
template <int ESZ> struct GIn  { const char* p; GTA_DEV float operator()(int ch) const { return ld<ESZ>(p, ch); } };
template <int ESZ> struct GOut { char* p;       GTA_DEV void operator()(int ch, float v) const { st<ESZ>(p, ch, v); } };
struct LIn  { const float* p; GTA_DEV float operator()(int ch) const { return p[ch]; } };
struct LOut { float* p;       GTA_DEV void operator()(int ch, float v) const { p[ch] = v; } };

GTA_DEV void row_decode(long row, int T, int H, int& b, int& h, int& t) {
    t = (int)(row % T);
    h = (int)((row / T) % H);
    b = (int)(row / ((long)T * H));
}

// bias_t: where the row's key bias goes in its (b, h) line, when that is not its token (-1: at t) -- the compacted position under a gather
template <class In, class Out>
GTA_DEV void apply_row(const ApplyParams& p, const int b, const int h, const int t, const In X, const Out Y, const int bias_t = -1) {
    const float tc = p.trans_coeff ? *p.trans_coeff : 1.0f;
    const int n = t / p.P;
    const float* vr = p.vrep ? p.vrep + ((long)b * p.N + n) * GTA_VREP_STRIDE : nullptr;
    float sq = 0.f;
    int ch = 0;
    for (int i = 0; i < p.d_triv; ++i, ++ch) { const float v = X(ch); Y(ch, v); sq += v * v; }
    if (p.d_se3 > 0) {
        // matrix used: mode 0 non-euclid: (E.m)^T ; mode 0 euclid: inv(E).m ; mode 1: inv(E).m ; mode 2: E.m
        float M[16];
        const bool use_inv_slot = (p.mode == 2) || (p.mode == 0 && !p.euclid);     // "inv" slot holds E
        const float* src = vr + (use_inv_slot ? GTA_VREP_INV : GTA_VREP_REP);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                const float m = (r == 3) ? (c == 3 ? 1.f : 0.f) : (c == 3 ? tc : 1.f);
                const float v = src[r * 4 + c] * m;
                if (p.mode == 0 && !p.euclid) M[c * 4 + r] = v; else M[r * 4 + c] = v;
            }
        if (p.euclid) {
            for (int blk = 0; blk < p.d_se3 / 3; ++blk, ch += 3) {
                const float a = X(ch), bb = X(ch + 1), c = X(ch + 2);
                for (int r = 0; r < 3; ++r) {
                    const float v = M[r * 4] * a + M[r * 4 + 1] * bb + M[r * 4 + 2] * c + M[r * 4 + 3];   // homogenisation
                    Y(ch + r, v); sq += v * v;
                }
            }
        } else {
            for (int blk = 0; blk < p.d_se3 / 4; ++blk, ch += 4) {
                const float a = X(ch), bb = X(ch + 1), c = X(ch + 2), d = X(ch + 3);
                for (int r = 0; r < 4; ++r) {
                    const float v = M[r * 4] * a + M[r * 4 + 1] * bb + M[r * 4 + 2] * c + M[r * 4 + 3] * d;
                    Y(ch + r, v); sq += v * v;
                }
            }
        }
    }
    if (p.d_so3 > 0) {
        const int tot = p.L >= 2 ? 8 : 3;
        for (int g = 0; g < p.d_so3 / tot; ++g) {
            for (int l = 1; l <= p.L; ++l) {
                const int dim = 2 * l + 1;
                const float* D = vr + (l == 1 ? GTA_VREP_D1 : GTA_VREP_D2);
                float in[5];
                for (int i = 0; i < dim; ++i) in[i] = X(ch + i);
                for (int r = 0; r < dim; ++r) {
                    float v = 0.f;
                    for (int c = 0; c < dim; ++c) v += (p.mode == 2 ? D[c * dim + r] : D[r * dim + c]) * in[c];
                    Y(ch + r, v); sq += v * v;
                }
                ch += dim;
            }
        }
    }
    if (p.d_so2 > 0) {
        const int nblk = p.d_so2 / 2;
        const float* cs = p.cs + ((long)b * p.T + t) * 2 * nblk;
        for (int blk = 0; blk < nblk; ++blk, ch += 2) {
            const float c = cs[2 * blk], s = (p.mode == 2 ? -1.f : 1.f) * cs[2 * blk + 1];
            const float a = X(ch), bb = X(ch + 1);
            const float v0 = c * a - s * bb, v1 = s * a + c * bb;
            Y(ch, v0); Y(ch + 1, v1); sq += v0 * v0 + v1 * v1;
        }
    }
    if (p.d_t2 > 0) {
        const float cx = p.coord[((long)b * p.T + t) * 2], cy = p.coord[((long)b * p.T + t) * 2 + 1];
        for (int blk = 0; blk < p.d_t2 / 3; ++blk, ch += 3) {
            const float a = X(ch), bb = X(ch + 1), c = X(ch + 2);
            float v0, v1, v2;
            if (p.mode == 0)      { v0 = a - cx * c; v1 = bb - cy * c; v2 = c; }                   // (T^-1)^T
            else if (p.mode == 1) { v0 = a; v1 = bb; v2 = cx * a + cy * bb + c; }                  // T
            else                  { v0 = a; v1 = bb; v2 = c - cx * a - cy * bb; }                  // T^-1
            Y(ch, v0); Y(ch + 1, v1); Y(ch + 2, v2); sq += v0 * v0 + v1 * v1 + v2 * v2;
        }
    }
    if (p.key_bias) p.key_bias[((long)b * p.H + h) * p.bias_pitch + (bias_t < 0 ? t : bias_t)] = -0.5f * p.bias_scale * sq;
}

}  // namespace
