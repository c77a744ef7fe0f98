// skin_act.h -- what the kernels of skinning.hip and skinloss.hip share: the row widths of the logit kinds, the moves of a
// block's contiguous slab of rows between global memory and LDS (slab.h, by row), and the bone-weight activations (the kinematic-tree
// softmax and F.softmax) with their reverses.  The spec of the activations is at the top of skinning.hip.  Every
// translation unit that includes this is built without FMA contraction (build.py STRICT).
#pragma once
#include "common.h"
#include "slab.h"

#define SKIN_THREADS 256

template <int KIND>
struct SkinKind {
    static constexpr int C = KIND == GS_SKIN_HIERARCHICAL ? 25 : 24;  // row width
};

// rows [row0, row0 + n) of a (., C) fp32 array <-> LDS (slab.h; row0 is a multiple of SKIN_THREADS: 16-byte aligned)
template <int C>
__device__ __forceinline__ void skin_slab_load(const float* __restrict__ g, int row0, int n, float* __restrict__ lds) {
    slab_load<SKIN_THREADS>(g + (size_t)row0 * C, n * C, lds);
}
template <int C>
__device__ __forceinline__ void skin_slab_store(float* __restrict__ g, int row0, int n, const float* __restrict__ lds) {
    slab_store<SKIN_THREADS>(g + (size_t)row0 * C, n * C, lds);
}
template <int C>
__device__ __forceinline__ void row_from_lds(const float* __restrict__ lds, int t, float* x) {
    if (C % 4 == 0) {
        const float4* l4 = reinterpret_cast<const float4*>(lds + t * C);
#pragma unroll
        for (int k = 0; k < C / 4; k++) {
            const float4 v = l4[k];
            x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) x[k] = lds[t * C + k];
    }
}

__device__ __forceinline__ float skin_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int K>
__device__ __forceinline__ void softmax_fwd(const float* x, float* y) {
    float m = x[0];
#pragma unroll
    for (int k = 1; k < K; k++) m = fmaxf(m, x[k]);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) {
        y[k] = expf(x[k] - m);
        s += y[k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) y[k] = y[k] / s;
}
template <int K>
__device__ __forceinline__ void softmax_bwd(const float* y, const float* dy, float* dx) {
    float d = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) d += y[k] * dy[k];
#pragma unroll
    for (int k = 0; k < K; k++) dx[k] = y[k] * (dy[k] - d);
}

// the split steps of the hierarchy: (parent, child) before step 5, then after it; the child's logit is the gate
#define HS_SPLITS_A(X) X(0, 1, 4) X(1, 2, 5) X(2, 3, 6) X(3, 4, 7) X(4, 5, 8) X(5, 6, 9) X(6, 7, 10) X(7, 8, 11)
#define HS_SPLITS_B(X) X(8, 12, 15) X(9, 13, 16) X(10, 14, 17) X(11, 16, 18) X(12, 17, 19) X(13, 18, 20) X(14, 19, 21) \
    X(15, 20, 22) X(16, 21, 23)
#define HS_NSPLIT 17

// forward of the hierarchy; v (optional): v[k] = the parent's value before split k, v[HS_NSPLIT] = p9 before step 5
__device__ __forceinline__ void hier_forward(const float* x, float* p, const float* s, const float* sm1, const float* sm2,
                                             float* v) {
#pragma unroll
    for (int i = 0; i < 3; i++) p[1 + i] = s[0] * sm1[i];
    p[0] = 1.0f - s[0];
#define HS_FWD(k, P, C)                      \
    {                                        \
        const float v_ = p[P];               \
        if (v) v[k] = v_;                    \
        p[C] = v_ * s[C];                    \
        p[P] = v_ * (1.0f - s[C]);           \
    }
    HS_SPLITS_A(HS_FWD)
    {
        const float v9 = p[9];
        if (v) v[HS_NSPLIT] = v9;
        const float e = v9 * s[24];
#pragma unroll
        for (int i = 0; i < 3; i++) p[12 + i] = e * sm2[i];
        p[9] = v9 * (1.0f - s[24]);
    }
    HS_SPLITS_B(HS_FWD)
#undef HS_FWD
}

__device__ __forceinline__ void hier_gates(const float* x, float* s, float* sm1, float* sm2) {
#pragma unroll
    for (int k = 0; k < 25; k++) s[k] = skin_sigmoid(x[k]);  // (s1..3, s12..14 are never read: the compiler drops them)
    softmax_fwd<3>(x + 1, sm1);
    softmax_fwd<3>(x + 12, sm2);
}

// reverse of hier_forward: dx (25) from x (25) and dW (24)
__device__ __forceinline__ void hier_backward(const float* x, const float* dW, float* dx) {
    float s[25], sm1[3], sm2[3], p[24], v[HS_NSPLIT + 1];
    hier_gates(x, s, sm1, sm2);
    hier_forward(x, p, s, sm1, sm2, v);
    float dp[24], ds[25];
#pragma unroll
    for (int j = 0; j < 24; j++) dp[j] = dW[j];
#pragma unroll
    for (int k = 0; k < 25; k++) ds[k] = 0.0f;
#define HS_BWD(k, P, C)                                          \
    {                                                            \
        ds[C] = v[k] * (dp[C] - dp[P]);                          \
        dp[P] = dp[C] * s[C] + dp[P] * (1.0f - s[C]);            \
    }
    // the splits after step 5, last first
    HS_BWD(16, 21, 23) HS_BWD(15, 20, 22) HS_BWD(14, 19, 21) HS_BWD(13, 18, 20) HS_BWD(12, 17, 19) HS_BWD(11, 16, 18)
    HS_BWD(10, 14, 17) HS_BWD(9, 13, 16) HS_BWD(8, 12, 15)
    {
        const float v9 = v[HS_NSPLIT], e = v9 * s[24];
        float de = 0.0f, dsm[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            de += dp[12 + i] * sm2[i];
            dsm[i] = dp[12 + i] * e;
        }
        ds[24] = v9 * (de - dp[9]);
        dp[9] = de * s[24] + dp[9] * (1.0f - s[24]);
        softmax_bwd<3>(sm2, dsm, dx + 12);
    }
    HS_BWD(7, 8, 11) HS_BWD(6, 7, 10) HS_BWD(5, 6, 9) HS_BWD(4, 5, 8) HS_BWD(3, 4, 7) HS_BWD(2, 3, 6) HS_BWD(1, 2, 5)
    HS_BWD(0, 1, 4)
#undef HS_BWD
    {
        float dsm[3];
        float d0 = -dp[0];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            d0 += dp[1 + i] * sm1[i];
            dsm[i] = dp[1 + i] * s[0];
        }
        ds[0] = d0;
        softmax_bwd<3>(sm1, dsm, dx + 1);
    }
    // sigmoid' = s (1 - s) for every gate; dx 1..3 and 12..14 came from the softmaxes
    dx[0] = ds[0] * (1.0f - s[0]) * s[0];
#pragma unroll
    for (int k = 4; k < 25; k++)
        if (k < 12 || k > 14) dx[k] = ds[k] * (1.0f - s[k]) * s[k];
}

template <int KIND>
__device__ __forceinline__ void weights_fwd(const float* x, float* W) {
    if (KIND == GS_SKIN_HIERARCHICAL) {
        float s[25], sm1[3], sm2[3];
        hier_gates(x, s, sm1, sm2);
        hier_forward(x, W, s, sm1, sm2, nullptr);
    } else if (KIND == GS_SKIN_SOFTMAX) {
        softmax_fwd<24>(x, W);
    } else {
#pragma unroll
        for (int j = 0; j < 24; j++) W[j] = x[j];
    }
}
template <int KIND>
__device__ __forceinline__ void weights_bwd(const float* x, const float* W, const float* dW, float* dx) {
    if (KIND == GS_SKIN_HIERARCHICAL) {
        hier_backward(x, dW, dx);
    } else if (KIND == GS_SKIN_SOFTMAX) {
        softmax_bwd<24>(W, dW, dx);
    } else {
#pragma unroll
        for (int j = 0; j < 24; j++) dx[j] = dW[j];
    }
}
