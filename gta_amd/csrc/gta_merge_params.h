// gta_merge_params.h -- argument blocks of the merge kernels (gta_merge.hip), shared with gta_abi.cpp.
// The pointers and (b, h, t) element strides of the n <= GTA_MERGE_MAX partial attentions travel in the block itself: the kernels index them
// with compile-time constants only (unrolled loops), so they are scalar loads from the kernel arguments -- no table in memory, no scratch.
#ifndef GTA_MERGE_PARAMS_H
#define GTA_MERGE_PARAMS_H

#define GTA_MERGE_MAX 8

struct GtaMergeParams {
    const void* outs[GTA_MERGE_MAX];          // [B,H,Tq,dh] views, channel stride 1
    const float* lses[GTA_MERGE_MAX];         // [B,H,Tq] views
    long outs_st[GTA_MERGE_MAX][3], lses_st[GTA_MERGE_MAX][3];
    void* out;
    float* lse;
    long out_st[3], lse_st[3];
    int n, B, H, Tq, dh;
};

struct GtaMergeBwdParams {
    const void* outs[GTA_MERGE_MAX];
    const float* lses[GTA_MERGE_MAX];
    void* douts[GTA_MERGE_MAX];
    float* dlses[GTA_MERGE_MAX];
    long outs_st[GTA_MERGE_MAX][3], lses_st[GTA_MERGE_MAX][3], douts_st[GTA_MERGE_MAX][3], dlses_st[GTA_MERGE_MAX][3];
    const void* dout;
    const float* dlse;                        // or null
    long dout_st[3], dlse_st[3];
    int n, B, H, Tq, dh;
};

#endif
