// second_colors.hip -- the colour gradient of a SECOND image rendered from the same geometry (gs_backward_with_second with
// GsSecondImage.dL_dcolors set): dL_dcolors2[i, c] = sum over pixels of alpha_i T_i dL_dpix2[c].
//
// The one-pass backward of both images (render_bwd.hip) gives the gradients of everything the two images SHARE -- alpha
// and T -- and the first image's colour gradient.  What it leaves out is the second image's own colour gradient, which
// depends on no gradient state at all: the weight alpha T of a (pixel, Gaussian) pair is what the FORWARD composited
// with.  So this is a forward-shaped walk of the tile lists, with no state of the render kernels' quadrant / chunk
// machinery (recorded quadrant lists, checkpoints, row marks):
//
//  1. second_colors_tile_kernel<true>: one workgroup per 16x16 tile (heaviest tiles first: the forward's launch order),
//     one thread per pixel, wave q on the 8x8 quadrant q of blend.h.  The tile's range of the point list is staged through
//     LDS SC_BATCH entries at a time, front to back (as pair_stats_kernel in debug_stats.hip walks it), in the log2-domain
//     form of blend.h (A2, B2, C2; alpha = min(0.99, opacity 2^power2)).  The thread that stages an entry also runs
//     blend.h's exact footprint test against the four quadrants (stage_entry_quad: a quadrant it drops holds no pixel with
//     alpha >= 1/255 -- the forward never blends there), and every wave compacts the batch's entries that reach ITS
//     quadrant (ballot + prefix count) before it walks them, the next entry's LDS reads issued ahead of the current one's
//     arithmetic.  alpha is evaluated with the very expression of the render kernels, so the power2 <= 0 and alpha >= 1/255
//     decisions are theirs bit for bit.  A pixel walks up to its own n_contrib -- the position of its last contributor,
//     which is how the backward render kernel bounds its walk, too: the forward's T (1 - alpha) < 1e-4 decision is not taken
//     again.  Per entry the 64 pixels' alpha T g_c are summed with the DPP ladder of common.h (a fixed order; skipped
//     where no lane of the wave blends the entry, and for a channel whose gradient is zero over the whole quadrant -- two
//     of three for the inverse-depth image) and, once per batch, across the four waves in wave order by the thread that
//     owns the entry, which writes ONE 16-byte row per (tile, Gaussian) pair -- in full, zeros included -- at the pair's
//     Gaussian-major slot: first_pair + (ty - miny) w + (tx - minx) for the tile (tx, ty) of the Gaussian's rectangle (the
//     pair numbering behind gradient_row in common.h; one slot per pair, not four).  Every pair of the frame sits in
//     exactly one tile list, so every slot below the frame's pair count is written exactly once.
//  2. second_colors_reduce_kernel: four lanes per Gaussian add up its contiguous span of rows [first_pair, first_pair +
//     tiles_touched) in index order (lane j: rows j, j + 4, ...), fold with two quad-permute DPP adds and write the
//     Gaussian's row of the (P, 3) output; zeros for a Gaussian that is culled or touches no tile.
//
// FEW, LONG LISTS (images of up to 2048 tiles, or GsFwdArgs.long_lists: common.h, few_long_lists_mode -- a trained avatar
// has ~150 tiles of 2000-7000 entries): one workgroup per tile would walk them alone, one dependent step after the other,
// on a chip that is otherwise idle.  There every tile's list is cut into K equal CHUNKS (a multiple of SC_BATCH entries; K
// = 16, or the largest power of two the workspace holds), one workgroup per (tile, chunk), and a launch in front,
// second_colors_tile_kernel<false>, leaves per (tile, chunk, pixel) the product of (1 - alpha) over the chunk: a chunk's
// workgroup starts from T = the product of the chunks before it, multiplied in order.  (T is then a differently
// associated product of the same factors as the forward's: fp32 rounding, the same on every run.)
//
// No atomics, no memset node, no host wait: the sums are taken in one order (bitwise reproducible) and all launches are
// kernel nodes under stream capture.  Workspace: the ROWS region of the backward scratch (4 D x 32 bytes: 16 D bytes of rows,
// behind them the chunk products), which is free once the per-Gaussian backward (its last reader) has been enqueued on the
// stream.
//
// LDS per workgroup: 7 KB of staged entries, 1 KB of quadrant masks, 2 KB of per-wave compacted indices, 12 KB of per-wave
// partial sums (seven workgroups per CU fit).  Staged entries are read at a wave-uniform address (a broadcast: no bank
// conflicts); masks, indices and partial sums by consecutive lanes at consecutive words.
#include "common.h"
#include "blend.h"

#define SC_BATCH 256     // list entries staged per trip (one per thread)
#define SC_MAX_CHUNKS 16 // chunks per tile where the lists are few and long

// SUMS = false: the per-pixel product of (1 - alpha) over chunk c < K - 1 of every tile -> prod[tile][c][pixel];
// SUMS = true: the rows.  K = 1: whole lists, no products.
template <bool SUMS>
__global__ __launch_bounds__(256) void second_colors_tile_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ point_list,
                                                                 const uint2* __restrict__ ranges, const uint32_t* __restrict__ order,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 const float* __restrict__ dL_dpix2, int W, int H, int gx, int ntiles,
                                                                 uint32_t D, const PairCount pc, int K, float* __restrict__ prod,
                                                                 float4* __restrict__ rows) {
    __shared__ float4 s0[SC_BATCH];           // x, y, A2, B2
    __shared__ float2 s1[SC_BATCH];           // C2, opacity
    __shared__ uint32_t sslot[SC_BATCH];      // the pair's row
    __shared__ uint32_t shit[SC_BATCH];       // bit q: the entry can reach quadrant q
    __shared__ uint16_t widx[4][SC_BATCH];    // per wave: the batch's entries that reach its quadrant, in list order
    __shared__ float part[3][4][SC_BATCH];    // [channel][wave][entry]: the wave's sum of alpha T g_c
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int KC = SUMS ? K : K - 1;          // chunks per tile this launch works on
    const int chunk = (int)blockIdx.x % KC;
    const int tile = (int)(order[(int)blockIdx.x / KC] & 0x7FFFFFFFu);  // heaviest tiles first; bit 31: the forward's mark
    if (tile >= ntiles) return;               // (never for a launch order the forward wrote)
    // (workgroup-uniform) a frame whose pairs did not fit the state rendered empty: nothing to walk, the sum writes zeros
    if (*pc.dev > (unsigned long long)pc.cap) return;
    const uint2 r = ranges[tile];
    const uint32_t n = r.y - r.x;
    const uint32_t L = ((n + (uint32_t)K - 1) / (uint32_t)K + SC_BATCH - 1) / SC_BATCH * SC_BATCH;  // entries per chunk
    const uint32_t begin = (uint32_t)chunk * L;
    if (SUMS ? begin >= n : begin + L >= n) return;  // (workgroup-uniform) no such chunk / no chunk behind it to start from its product
    const uint32_t end = min(n, begin + L);
    const uint32_t tx = (uint32_t)(tile % gx), ty = (uint32_t)(tile / gx);
    const int qx0 = (int)tx * TILE + 8 * (q & 1), qy0 = (int)ty * TILE + 8 * (q >> 1);  // the wave's quadrant (blend.h)
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t HW = (size_t)H * W, pid = (size_t)py * W + px;
    const uint32_t last = inside ? n_contrib[pid] : 0u;  // 1-based position of the pixel's last contributor
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (SUMS && inside) { g0 = dL_dpix2[pid]; g1 = dL_dpix2[HW + pid]; g2 = dL_dpix2[2 * HW + pid]; }
    // (wave-uniform) channels with a gradient somewhere in the quadrant: the others' sums are the zeros already there
    const bool ch0 = __ballot(g0 != 0.f) != 0ull, ch1 = __ballot(g1 != 0.f) != 0ull, ch2 = __ballot(g2 != 0.f) != 0ull;
    const uint32_t wmax = wave_max(last);  // entries beyond it meet no pixel of this wave
    const float pxf = (float)px, pyf = (float)py;
    const size_t prod_at = ((size_t)tile * (size_t)(K - 1)) * 256 + (size_t)tid;
    float T = 1.0f;
    if (SUMS)
        for (int c = 0; c < chunk; c++) T *= prod[prod_at + (size_t)c * 256];  // T in front of the chunk
    for (uint32_t base = begin; base < end; base += SC_BATCH) {
        const uint32_t m = min((uint32_t)SC_BATCH, end - base);
        __syncthreads();  // (the previous batch's entries and partial sums have been read)
        uint32_t hits = 0u;
        if ((uint32_t)tid < m) {
            const uint32_t id = point_list[r.x + base + tid];
            const float4 p0 = rec[(size_t)id * 3], p1 = rec[(size_t)id * 3 + 1], p2 = rec[(size_t)id * 3 + 2];
            s0[tid] = make_float4(p0.x, p0.y, (-0.5f * LOG2E_F) * p0.z, -LOG2E_F * p0.w);
            s1[tid] = make_float2((-0.5f * LOG2E_F) * p1.x, p1.y);
            if (SUMS) {
                const uint32_t off = __float_as_uint(p2.y), rmin = __float_as_uint(p2.z), rsz = __float_as_uint(p2.w);
                sslot[tid] = off + (ty - (rmin >> 16)) * (rsz & 0xFFFFu) + (tx - (rmin & 0xFFFFu));
            }
            Staged unused;
#pragma unroll
            for (int qq = 0; qq < 4; qq++)
                hits |= stage_entry_quad(p0, p1, p2, (int)tx * TILE + 8 * (qq & 1), (int)ty * TILE + 8 * (qq >> 1), unused) ? (1u << qq) : 0u;
        }
        shit[tid] = hits;
        if (SUMS) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int w = 0; w < 4; w++) part[c][w][tid] = 0.f;
        }
        __syncthreads();
        // this wave's entries of the batch: those that reach its quadrant, up to the last one any of its pixels meets
        const uint32_t mw = min(m, wmax > base ? wmax - base : 0u);  // (wave-uniform)
        uint32_t cnt = 0;
        for (uint32_t e0 = 0; e0 < mw; e0 += 64) {
            const uint32_t e = e0 + (uint32_t)lane;
            const bool hit = e < mw && ((shit[e] >> q) & 1u) != 0u;
            const unsigned long long b = __ballot(hit);
            if (hit) widx[q][cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] = (uint16_t)e;
            cnt += (uint32_t)__popcll(b);
        }
        __builtin_amdgcn_wave_barrier();  // (the indices are read by other lanes of the wave than wrote them)
        if (cnt > 0) {
            // (indices and entries are the same in every lane: broadcast reads; entry j + 1 and index j + 2 are on their way
            // while entry j is evaluated)
            uint32_t k1 = widx[q][0];
            float4 a1 = s0[k1];
            float2 b1 = s1[k1];
            uint32_t k2 = widx[q][min(1u, cnt - 1)];
            for (uint32_t j = 0; j < cnt; j++) {
                const uint32_t k = k1;
                const float4 a = a1;
                const float2 b = b1;
                k1 = k2;
                a1 = s0[k1];
                b1 = s1[k1];
                k2 = widx[q][min(j + 2, cnt - 1)];
                const float dx = a.x - pxf, dy = a.y - pyf;
                // A2 dx^2 + B2 dx dy + C2 dy^2, evaluated exactly as the render kernels do
                const float power2 = __builtin_fmaf(a.z * dx, dx, __builtin_fmaf(a.w, dx, b.x * dy) * dy);
                const float G = __builtin_amdgcn_exp2f(power2);
                const float al = fminf(0.99f, b.y * G);
                const bool valid = (power2 <= 0.0f) && (base + k < last) && (al >= (1.0f / 255.0f));
                const float alpha = valid ? al : 0.f;
                if (SUMS) {
                    if (__ballot(valid) != 0ull) {  // (wave-uniform; otherwise nothing is blended here: the zeros stand)
                        const float wgt = alpha * T;
                        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
                        if (ch0) c0 = wave_scan_incl(wgt * g0);  // (lane 63: the wave's sum, in wave_sum's order)
                        if (ch1) c1 = wave_scan_incl(wgt * g1);
                        if (ch2) c2 = wave_scan_incl(wgt * g2);
                        if (lane == 63) {
                            part[0][q][k] = c0;
                            part[1][q][k] = c1;
                            part[2][q][k] = c2;
                        }
                    }
                }
                T *= 1.f - alpha;
            }
        }
        if (SUMS) {
            __syncthreads();
            if ((uint32_t)tid < m) {
                // the four waves' sums in wave order
                const float v0 = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
                const float v1 = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
                const float v2 = ((part[2][0][tid] + part[2][1][tid]) + part[2][2][tid]) + part[2][3][tid];
                const uint32_t slot = sslot[tid];
                if (slot < D) rows[slot] = make_float4(v0, v1, v2, 0.f);  // (always true for a consistent state: the scratch is carved for D pairs)
            }
        }
    }
    if (!SUMS) prod[prod_at + (size_t)chunk * 256] = T;
}

__global__ __launch_bounds__(256) void second_colors_reduce_kernel(int P, const int32_t* __restrict__ radii, const float4* __restrict__ rec,
                                                                   const uint32_t* __restrict__ tiles, const float4* __restrict__ rows,
                                                                   uint32_t D, const PairCount pc, float* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t >> 2, j = t & 3;
    float f[3] = {0.f, 0.f, 0.f};
    // A frame whose pairs did not fit the state (a captured graph replayed on a scene that has outgrown its capacity) rendered
    // empty: its tile lists are empty and NO row was written, while the records still number the real scene's pairs.  Such a
    // frame gets zeros, as every other gradient of it is zero.  D == 0: no rows either
    const bool fits = D > 0u && *pc.dev <= (unsigned long long)pc.cap;
    if (fits && i < P && radii[i] > 0) {
        const uint32_t off = __float_as_uint(rec[(size_t)i * 3 + 2].y), tt = tiles[i];
        if ((unsigned long long)off + tt <= (unsigned long long)D) {  // (always, when the frame fits: its count is at most D)
            for (uint32_t k = (uint32_t)j; k < tt; k += 4u) {
                const float4 v = rows[(size_t)off + k];
                f[0] += v.x; f[1] += v.y; f[2] += v.z;
            }
        }
    }
    // fold the four lanes of the group: (l0 + l1) + (l2 + l3), every lane of the wave taking part
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = f[c];
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));  // quad_perm:[1,0,3,2]
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));  // quad_perm:[2,3,0,1]
        f[c] = v;
    }
    if (i < P && j < 3) out[(size_t)i * 3 + j] = j == 0 ? f[0] : (j == 1 ? f[1] : f[2]);
}

int launch_second_colors(const float* rec, const uint32_t* tiles, const int32_t* radii, const uint32_t* point_list,
                         const uint32_t* ranges, const uint32_t* order, const uint32_t* n_contrib, const float* dL_dpix2, int P,
                         int W, int H, int64_t D, PairCount pc, bool few_long_lists, void* workspace, size_t workspace_bytes,
                         float* dL_dcolors, int debug, hipStream_t s) {
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE, ntiles = gx * gy;
    float4* const rows = reinterpret_cast<float4*>(workspace);
    if (D > 0) {
        // chunks per tile: as many as the workspace holds products for behind the rows (none: whole lists)
        const size_t rows_bytes = align_up((size_t)D * 16, 256);
        int K = 1;
        if (few_long_lists)
            for (int k = SC_MAX_CHUNKS; k > 1 && K == 1; k >>= 1)
                if (rows_bytes + (size_t)ntiles * (size_t)(k - 1) * 1024 <= workspace_bytes) K = k;
        float* const prod = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + rows_bytes);
        if (K > 1) {
            hipLaunchKernelGGL(second_colors_tile_kernel<false>, dim3((unsigned)(ntiles * (K - 1))), dim3(256), 0, s,
                               reinterpret_cast<const float4*>(rec), point_list, reinterpret_cast<const uint2*>(ranges), order, n_contrib,
                               dL_dpix2, W, H, gx, ntiles, (uint32_t)D, pc, K, prod, rows);
            GS_LAUNCH_CHECK("second_colors_products", debug, s);
        }
        hipLaunchKernelGGL(second_colors_tile_kernel<true>, dim3((unsigned)(ntiles * K)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(rec), point_list, reinterpret_cast<const uint2*>(ranges), order, n_contrib,
                           dL_dpix2, W, H, gx, ntiles, (uint32_t)D, pc, K, prod, rows);
        GS_LAUNCH_CHECK("second_colors_tiles", debug, s);
    }
    hipLaunchKernelGGL(second_colors_reduce_kernel, dim3((unsigned)(((size_t)P * 4 + 255) / 256)), dim3(256), 0, s, P, radii,
                       reinterpret_cast<const float4*>(rec), tiles, reinterpret_cast<const float4*>(rows), (uint32_t)D, pc, dL_dcolors);
    GS_LAUNCH_CHECK("second_colors_reduce", debug, s);
    return GS_OK;
}
