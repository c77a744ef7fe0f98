// blend.h -- the per-(pixel, Gaussian) evaluation shared by the forward and backward render
// kernels (they must take identical skip decisions), per-(tile, Gaussian) staging, and wave64
// reduction helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LOG2E_F 1.4426950408889634f

// ---------------------------------------------------------------------------------------------
// Ownership: a 16x16 tile is four 8x8 QUADRANTS, quadrant q sits at (8 * (q & 1), 8 * (q >> 1)); one
// wave64 per quadrant, lane l <-> pixel (l & 7, l >> 3) in the forward.
// ---------------------------------------------------------------------------------------------

// A staged (quadrant, Gaussian) entry: 48 bytes in LDS, read at a wave-uniform address.
//   a = (x, y, A2, B2)   centre in pixels; conic pre-scaled into the log2 domain:
//                        power2 = A2 dx^2 + C2 dy^2 + B2 dx dy = log2(e) * power
//   b = (C2, opacity, thr, compacted index + 1)
//   c = (r, g, b, position in the tile's list (1-based))
struct Staged {
    float4 a, b, c;
};

// Builds the staged entry of a splat record (r0, r1, r2 as written by the preprocess kernel) for ONE
// 8x8 quadrant with origin (QX0, QY0) and returns whether the Gaussian can reach the quadrant at
// all (the forward kernel runs one wave per quadrant and compacts on this flag).  `thr`: alpha >= 1/255
// <=> opacity * 2^power2 >= 1/255 <=> power2 >= -log2(255 opacity), kept 1e-3 relaxed.
// EXACT ellipse-vs-rectangle test: the minimum over the quadrant's pixel-centre rectangle of the
// quadratic form q(d) = A dx^2 + 2 B dx dy + C dy^2 (convex, so either the centre lies inside, or the
// minimum sits on one of the four edges, where it is a clamped 1-D parabola) against
// 2 tau = 2 ln(255 opacity) (+ slack).  alpha >= 1/255 <=> q <= 2 ln(255 opacity); the test keeps a
// 1e-3 (log2) slack plus a relative 1e-4, so every pair it drops would fail the per-pixel alpha test.
//
// The test holds NO division (it runs once per list entry and quadrant wave, in front of a loop bound by VALU issue; a
// correctly rounded quotient is ~11 instructions, and the exact form had five of them):
//   * the parabola's vertex on an edge is ys = clamp(k xf, y0, y1) with k = -B / c: ONE approximate reciprocal
//     (v_rcp_f32, 1 ulp) per orientation, shared by the orientation's two edges.  An inexact ys does not leave the edge;
//     it moves the evaluated point by d = |ys| e along it (e ~ 3 x 2^-23: the reciprocal and two roundings) and RAISES the
//     value, by exactly c d^2 = (c ys^2) e^2 -- second order.  Against the minimum itself, xf^2 det / c at an unclamped
//     vertex, that is (B^2 / det) e^2 <= (A C / det) e^2 < 2.7e5 x 1.3e-13 = 4e-8 relative (A C / det < 2.7e5 is what
//     `rel < 0.5` below demands): three orders of magnitude inside the 1e-4 relative slack.  A clamped vertex is y0 or y1
//     itself (v_med3_f32 is exact);
//   * the decision is one compare of the minimum against a limit that depends on the Gaussian alone:
//     qmin (1 - rel) - 1e-3 <= 2 tau  <=>  qmin <= (2 tau + 1e-3) / (1 - rel)   (0.5 < 1 - rel <= 1),
//     lim = (2 tau + 1e-3) rcp(1 - rel) (1 + 2^-20).  The last factor pays for what the rewrite rounds differently: two
//     approximate reciprocals (rcp(det) enters through rel < 0.5 scaled by 1.9e-6, rcp(1 - rel) in full: 2^-23) and three
//     products (3 x 2^-24) -- under 2^-21 in all, so lim is never below the exact quotient, and 2^-20 = 1e-6 is a
//     hundredth of the relative slack that is there to be used up.
// NaN (0 x inf from a subnormal C) fails `qmin > lim` and keeps the entry.
// min over y in [y0, y1] of axx + b2x y + c y^2, the edge at xf:  axx = a xf^2, b2x = 2 B xf, kx = -(B / c) xf
__device__ __forceinline__ float edge_min(float axx, float b2x, float c, float kx, float y0, float y1) {
    const float ys = __builtin_amdgcn_fmed3f(kx, y0, y1);
    return axx + (b2x + c * ys) * ys;
}
__device__ __forceinline__ bool stage_entry_quad(const float4 r0, const float4 r1, const float4 r2, int QX0, int QY0,
                                                 Staged& s) {
    const float gx = r0.x, gy = r0.y, A = r0.z, B = r0.w, C = r1.x, o = r1.y;
    const float thr = -__log2f(255.f * o) - 1e-3f;
    bool hit = false;
    if (thr <= 0.f) {
        hit = true;
        if (A > 0.f && C > 0.f) {
            const float two_tau = (-2.f / LOG2E_F) * thr;
            // rectangle of pixel centres relative to the Gaussian centre
            const float x0 = (float)QX0 - gx, x1 = x0 + 7.f;
            const float y0 = (float)QY0 - gy, y1 = y0 + 7.f;
            const bool inside = (x0 <= 0.f) && (x1 >= 0.f) && (y0 <= 0.f) && (y1 >= 0.f);
            const float b2 = 2.f * B;
            const float ky = -B * __builtin_amdgcn_rcpf(C), kx = -B * __builtin_amdgcn_rcpf(A);  // vertex slopes: y = ky x, x = kx y
            const float axx0 = A * x0 * x0, axx1 = A * x1 * x1, cyy0 = C * y0 * y0, cyy1 = C * y1 * y1;
            const float qmin = fminf(fminf(edge_min(axx0, b2 * x0, C, ky * x0, y0, y1), edge_min(axx1, b2 * x1, C, ky * x1, y0, y1)),
                                     fminf(edge_min(cyy0, b2 * y0, A, kx * y0, x0, x1), edge_min(cyy1, b2 * y1, A, kx * y1, x0, x1)));
            // relative slack: 1e-4, plus the rounding of a form whose terms cancel (long thin Gaussians): ~2^-24 A C / det
            // per operation (gs_math.h: snug_half_widths); when the bound says nothing the entry is kept
            const float AC = A * C;
            const float detc = AC - B * B;
            const float rel = 1e-4f + AC * __builtin_amdgcn_rcpf(detc) * 1.9073486e-6f;
            const float lim = (two_tau + 1e-3f) * __builtin_amdgcn_rcpf(1.0f - rel) * 1.00000095f;  // (1 + 2^-20)
            hit = inside || !(detc > 0.f) || !(rel < 0.5f) || !(qmin > lim);
        }
    }
    s.a = make_float4(gx, gy, (-0.5f * LOG2E_F) * A, -LOG2E_F * B);
    s.b = make_float4((-0.5f * LOG2E_F) * C, o, thr, 0.f);
    s.c = make_float4(r1.z, r1.w, r2.x, 0.f);
    return hit;
}

// the staged form alone (no footprint test): for a walk of a quadrant's recorded compacted list, whose entries are hits
__device__ __forceinline__ void stage_entry_convert(const float4 r0, const float4 r1, const float4 r2, Staged& s) {
    s.a = make_float4(r0.x, r0.y, (-0.5f * LOG2E_F) * r0.z, -LOG2E_F * r0.w);
    s.b = make_float4((-0.5f * LOG2E_F) * r1.x, r1.y, 0.f, 0.f);
    s.c = make_float4(r1.z, r1.w, r2.x, 0.f);
}

// The inner loop's marks (render_fwd.hip: blend / step): where a pair is blended, the loop's LDS address register is
// kept -- for the even entries of a run the entry's own address, for the odd ones the address 48 bytes past it.  So
// entry j of the batch (staged at sp0 + 48 j) leaves sp0 + 48 j in mark_e or sp0 + 48 (j + 1) in mark_o, and the last
// blended entry of the batch, as a 1-based index into it, is max(mark_e + 48, mark_o) - sp0 over 48: ONE decode for
// both marks (48-byte entries: x / 48 = x * 43691 >> 21 for x < 2^15).  "No entry yet" is the pair of marks that decodes to 0.
__device__ __forceinline__ uint32_t mark_none_even(uint32_t sp0) { return sp0 - 48u; }
__device__ __forceinline__ uint32_t mark_none_odd(uint32_t sp0) { return sp0; }
__device__ __forceinline__ uint32_t marks_last_entry(uint32_t mark_e, uint32_t mark_o, uint32_t sp0) {
    const uint32_t d = max(mark_e - sp0 + 48u, mark_o - sp0);  // (both >= 0: marks only ever move up from "none")
    return (d * 43691u) >> 21;
}

// ---- DPP helpers (cross-lane moves without LDS) ----
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_get(float v) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return wave_max(v); }  // (common.h: DPP ladder)
