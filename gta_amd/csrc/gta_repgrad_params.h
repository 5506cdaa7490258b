// gta_repgrad_params.h -- launch record of the rep-gradient sums (gta_repgrad.hip), filled by gta_rep_grad_sums (gta_abi.cpp).
#ifndef GTA_REPGRAD_PARAMS_H
#define GTA_REPGRAD_PARAMS_H

#include <hip/hip_runtime.h>

struct GtaRepGradParams {
    const void* a[2];                 // pair i: sum a b^T per channel group; pair 1 unused when npairs == 1
    const void* b[2];
    long as[2][3], bs[2][3];          // element strides (batch, head, token); channel stride 1
    int npairs;
    int B, H, T, N, P;                // P = T / N tokens per view
    int tpb, chunks;                  // tokens per workgroup (256 / H), workgroups per view
    int off_se3, n_se3;               // first channel, 4-channel (euclid: 3-channel) groups; n_se3 = 0: no view sums
    int off_so2, n_so2;               // first channel, 2-channel blocks; 0: no per-token so2 sums
    int off_t2, n_t2;                 // first channel, 3-channel groups; 0: no per-token t2 sums
    float* part;                      // [B*N][chunks][16] per-workgroup partial view sums
    float* view_out;                  // [B*N][16]
    float* so2_out;                   // [B*T][n_so2][4]
    float* t2_out;                    // [B*T][9]
    const int32_t* lens;              // [B] valid tokens of this side per scene (clamped to 1..T): the VARLEN instances; nullptr: every row is live
    const uint8_t* live;              // [B, T] one byte per token of this side, non-zero = live: the MASKED instances; nullptr: not masked
};

constexpr int GTA_REPGRAD_THREADS = 256;

// tokens per workgroup of a launch: H heads of tpb tokens fill a workgroup's 256 threads (0: H unsupported)
inline int gta_repgrad_tpb(int H) { return H > 0 && H <= GTA_REPGRAD_THREADS ? GTA_REPGRAD_THREADS / H : 0; }

int gta_repgrad_dispatch(const GtaRepGradParams& p, int esz, bool euclid, hipStream_t stream);

#endif
