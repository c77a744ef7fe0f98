// slab.h -- a workgroup's contiguous slab of rows between global memory and LDS (internal): `total` floats from `g`, the
// slab's first float (16-byte aligned, as is `lds`), moved by T threads with 16-byte accesses and a scalar tail of
// total mod 4 floats.  The caller puts its barriers around them.
#pragma once
#include <hip/hip_runtime.h>

template <int T>
__device__ __forceinline__ void slab_load(const float* __restrict__ g, int total, float* __restrict__ lds) {
    const int n4 = total >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* l4 = reinterpret_cast<float4*>(lds);
    for (int k = threadIdx.x; k < n4; k += T) l4[k] = g4[k];
    for (int k = 4 * n4 + threadIdx.x; k < total; k += T) lds[k] = g[k];
}
template <int T>
__device__ __forceinline__ void slab_store(float* __restrict__ g, int total, const float* __restrict__ lds) {
    const int n4 = total >> 2;
    float4* g4 = reinterpret_cast<float4*>(g);
    const float4* l4 = reinterpret_cast<const float4*>(lds);
    for (int k = threadIdx.x; k < n4; k += T) g4[k] = l4[k];
    for (int k = 4 * n4 + threadIdx.x; k < total; k += T) g[k] = lds[k];
}
