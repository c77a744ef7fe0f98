// render_fwd.hip -- per-tile front-to-back alpha compositing (replaces
// upstream renderCUDA forward).
//
// CDNA4 mapping: ONE wave64 per 8x8 QUADRANT of a 16x16 tile (four waves per tile, one pixel per
// lane; 4 x tiles waves keep every SIMD 8 deep and let the dispatcher balance the heavy centre tiles).
// The tile's depth-ordered list is staged 64 entries at a time: each lane gathers one 48-byte splat
// record (next batch prefetched into registers), converts it (log2-domain conic, alpha threshold) and
// tests whether the Gaussian's alpha >= 1/255 footprint (ellipse bbox) reaches THIS quadrant; the
// entries that do are COMPACTED into LDS with a ballot prefix, so the inner loop carries no mask
// logic at all and reads each staged entry at a wave-uniform address.  The per-pixel body is
// branch-free (compute, then select).  No barrier spans more than this one wave; the early-out is
// a wave ballot.
//
// The compaction is also RECORDED for the backward pass: qlist (the quadrant's compacted Gaussian
// indices, in order), the per-pixel last contributor in compacted coordinates, and the per-quadrant
// count up to the last contributor.  The backward therefore never re-derives relevance.
#include "common.h"
#include "blend.h"
#include <type_traits>

struct FwdArgs {
    const float4* __restrict__ rec;
    const uint32_t* __restrict__ point_list;
    const uint2* __restrict__ ranges;
    const uint32_t* __restrict__ order;
    const float* __restrict__ bg;
    int W, H, gx, ntiles, xmap;
    float* __restrict__ out_color;
    float* __restrict__ final_T;
    uint32_t* __restrict__ n_contrib;
    uint32_t* __restrict__ qlist;
    uint32_t* __restrict__ ncon_c;
    uint32_t* __restrict__ qcount;
    float4* __restrict__ ckpt;
    uint32_t* __restrict__ ck_start;
    int chunks;
    // a second render of the same geometry (gs_forward_shared): the first render's per-quadrant counts and n_contrib --
    // the quadrants' recorded compacted lists (qlist) are walked instead of the tiles' lists
    const uint32_t* __restrict__ src_qcount;
    const uint32_t* __restrict__ src_n_contrib;
    // ... and, if not null, a word that is ZERO when that second render's colours are all (1, 1, 1): the render then
    // leaves at once -- second_ones_kernel writes the image, 1 - T, from the first render's state
    const unsigned long long* __restrict__ not_ones;
    // the side job of this launch (null: none): ROW_UNWRITTEN into every mark word of the backward's gradient rows
    // (BinLayout::marks) -- this kernel is bound by its VALU stream, the stores ride along; *marks_flag := MARKS_CLEAN
    uint4* __restrict__ marks;
    size_t mark_quads;
    uint32_t* __restrict__ marks_flag;
    // (a second render) the image state's word that says "this image IS 1 - T of the first render": this launch -- the one
    // that decides between compositing and leaving the speculative 1 - T image (common.h: second_ones_body) -- sets it
    uint32_t* __restrict__ all_ones;
    // fused L1 loss (GsFwdArgs.l1_target; null: off): the target image and one partial sum of |out_color - target| per
    // quadrant, written by the quadrant's wave(s) from the colours they hold at the end of their walk
    const float* __restrict__ l1_target;
    float* __restrict__ l1_part;
};
__device__ __forceinline__ void forward_side_fill(const FwdArgs& A) {
    if (!A.marks) {  // not this launch's job; a state word it owns must not keep what an earlier use of the memory left there
        if (A.marks_flag && blockIdx.x == 0 && threadIdx.x == 0) *A.marks_flag = 0u;
        return;
    }
    const uint4 ones = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < A.mark_quads; k += (size_t)gridDim.x * blockDim.x)
        store_stream(&A.marks[k], ones);
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.marks_flag = MARKS_CLEAN;  // (read by a later launch: the backward's)
}

// between two phases of ONE wave that exchange data through LDS (a wave's LDS operations execute in order)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (compile-time ordering only: nothing waits on the global loads in flight)
    __builtin_amdgcn_wave_barrier();
}

// workgroup barrier for data exchanged through LDS only: waits for this wave's LDS operations, not for its global ones
// (__syncthreads() also drains vmcnt: the prefetched records in flight and the qlist store of the batch)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One wave, one quadrant (tile, q), one entry per step.  `srec`: LDS for 66 staged entries (64 + the two the pipelined
// loop may read past a batch).
template <bool FQ>
__device__ __forceinline__ void render_quadrant_1(const FwdArgs& A, const int tile, const int q, float4* __restrict__ srec) {
    const float4* __restrict__ rec = A.rec;
    const uint32_t* __restrict__ point_list = A.point_list;
    const float* __restrict__ bg = A.bg;
    const int W = A.W, H = A.H, gx = A.gx, chunks = A.chunks;
    float* __restrict__ out_color = A.out_color;
    float* __restrict__ final_T = A.final_T;
    uint32_t* __restrict__ n_contrib = A.n_contrib;
    uint32_t* __restrict__ qlist = A.qlist;
    uint32_t* __restrict__ ncon_c = A.ncon_c;
    uint32_t* __restrict__ qcount = A.qcount;
    float4* __restrict__ ckpt = A.ckpt;
    uint32_t* __restrict__ ck_start = A.ck_start;
    const int tx = tile % gx, ty = tile / gx;
    const int lane = threadIdx.x & 63;
    const int QX0 = tx * TILE + 8 * (q & 1), QY0 = ty * TILE + 8 * (q >> 1);
    const int px = QX0 + (lane & 7), py = QY0 + (lane >> 3);
    const float pxf = (float)px, pyf = (float)py;
    const bool inside = px < W && py < H;
    const uint2 range = A.ranges[tile];
    const int n_tile = (int)(range.y - range.x);
    const uint32_t qbase = 4u * range.x + (uint32_t)q * (uint32_t)n_tile;  // this quadrant's slice of qlist / gradient rows
    // what is walked: the tile's list, or (FQ) the quadrant's own compacted list as the first render recorded it -- up to
    // its last contributor: the colours do not change which entries contribute
    const int n = FQ ? (int)A.src_qcount[tile * 4 + q] : n_tile;
    const uint32_t* __restrict__ list = FQ ? qlist + qbase : point_list + range.x;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));

    // A pixel is "alive" while T > 0.  The sign of T doubles as the done flag: when a contribution
    // would push T below 1e-4 the pixel is frozen as T := -T, which keeps final_T and makes every later
    // test fail by itself.  All per-pixel decisions are VALU compares + selects (v_cmp -> vcc ->
    // v_cndmask): no scalar mask arithmetic in the inner loop -- the CU's single scalar unit was the
    // bottleneck of the mask-based version.
    float T = inside ? 1.0f : -1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f;
    // the fused L1 loss's target values of this pixel: requested NOW (a load at the wave's end is a stall of a whole
    // memory latency with nothing left to hide it behind: + 11 us on the launch at config 3 when it was there)
    float gt0 = 0.f, gt1 = 0.f, gt2 = 0.f;
    if (A.l1_target && inside) {
        const size_t HW = (size_t)H * W, pid = (size_t)py * W + px;
        gt0 = A.l1_target[pid]; gt1 = A.l1_target[HW + pid]; gt2 = A.l1_target[2 * HW + pid];
    }
    uint32_t last = 0, last_k = 0;
    uint32_t kcount = 0;  // wave-uniform: compacted entries staged so far
    int nck = 0;                   // checkpoints written so far (chunks of the backward begun, less one)
    bool live = __ballot(T > 0.f) != 0ull;  // wave-uniform

    float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
    // Prefetch two deep: the list index of the batch after next, the record of the next batch -- a record load depends
    // on its index load, and the two in a row (two trips to the L2 or beyond) are longer than a batch of few hits takes
    uint32_t pid_g = 0, pid_n = 0;
    if (live && lane < n) {
        pid_g = list[lane];
        p0 = rec[(size_t)pid_g * 3];
        p1 = rec[(size_t)pid_g * 3 + 1];
        p2 = rec[(size_t)pid_g * 3 + 2];
    }
    if (live && 64 + lane < n) pid_n = list[64 + lane];
    for (int base = 0; base < n && live; base += 64) {
        asm volatile("" : "+v"(pid_n));  // (waited for here, not behind this batch's qlist store: render_quadrant_4)
        Staged s;
        bool hit;
        if (FQ) {
            stage_entry_convert(p0, p1, p2, s);
            hit = base + lane < n;
        } else {
            hit = stage_entry_quad(p0, p1, p2, QX0, QY0, s) && (base + lane < n);
        }
        const unsigned long long bal = __ballot(hit);
        const int cnt = __popcll(bal);
        wave_lds_sync();
        if (hit) {
            const int slot = __popcll(bal & lt_mask);
            const uint32_t k = kcount + (uint32_t)slot;  // compacted index of this entry
            s.c.w = __uint_as_float((uint32_t)(base + lane + 1));  // position in the tile's list (1-based)
            srec[slot * 3] = s.a;
            srec[slot * 3 + 1] = s.b;
            srec[slot * 3 + 2] = s.c;
            if (!FQ) qlist[qbase + k] = pid_g;  // record the compaction for the backward
        }
        wave_lds_sync();
        kcount += (uint32_t)cnt;
        if (base + 64 + lane < n) {
            pid_g = pid_n;
            p0 = rec[(size_t)pid_g * 3];
            p1 = rec[(size_t)pid_g * 3 + 1];
            p2 = rec[(size_t)pid_g * 3 + 2];
            if (base + 128 + lane < n) pid_n = list[base + 128 + lane];
        }
        // The staged entries are read at a wave-uniform address.  Keeping that address in a VGPR the
        // compiler cannot prove uniform (vzero) makes it one v_add per entry + immediate offsets; proven
        // uniform, it is rebuilt from SGPRs with a v_mov per dword and a dozen scalar adds per entry, and
        // the CU's single scalar unit becomes the bottleneck.
        // (Held as the 32-bit LDS address itself: the loop advances it inside an asm statement, below.)
        uint32_t sp = (uint32_t)(uintptr_t)srec + vzero;
        const uint32_t kbase = kcount - (uint32_t)cnt;  // compacted index of this batch's first entry
        // One entry against the 64 pixels.  `a`, `b`, `c` = the three staged quads of the entry.
        // `mark`: set to the loop's LDS address register where the pair is blended -- the entry's index in the batch is
        // read back from it after the loop (a select between two VGPRs; selecting the wave-uniform index itself costs a
        // v_mov per entry on top, an SGPR cannot be the second source next to vcc)
        auto blend = [&](const float4 a, const float2 b, const float4 c, uint32_t& mark) {
            const float dx = a.x - pxf, dy = a.y - pyf;
            // A2 dx^2 + B2 dx dy + C2 dy^2, evaluated exactly as the backward does
            const float power2 = __builtin_fmaf(a.z * dx, dx, __builtin_fmaf(a.w, dx, b.x * dy) * dy);
            const float G = __builtin_amdgcn_exp2f(power2);
            const float al = fminf(0.99f, b.y * G);
            const bool valid = power2 <= 0.0f && al >= (1.0f / 255.0f);
            const float a2 = valid ? al : 0.f;                    // alpha, or 0 if the pair is rejected
            const float test_T = T * (1.f - a2);                  // == T for a rejected pair, < 0 for a frozen pixel
            const bool pass = test_T >= 0.0001f;
            const float wT = a2 * T;
            const float w = pass ? wT : 0.f;                      // > 0 exactly when the pair is blended
            T = pass ? test_T : -fabsf(T);                        // freeze: keeps |T| = final_T
            C0 += c.x * w;
            C1 += c.y * w;
            C2 += c.z * w;
            // blended <=> w > 0 <=> valid and pass (pass implies T > 0): the AND of two lane masks the loop already has,
            // one scalar instruction instead of a third compare
            mark = (valid && pass) ? sp : mark;
        };
        // The loop is software-pipelined by hand, two entries per trip: the LDS reads of the NEXT entry are issued
        // before the current one is evaluated.  With eight waves per SIMD the LDS latency hides behind the other waves
        // anyway; a lone wave on its SIMD paid the ~100 cycles of every entry's reads in full.  (Reads one entry past the
        // batch: srec has a 65th.)
        typedef float lds_v4 __attribute__((ext_vector_type(4)));
        typedef float lds_v2 __attribute__((ext_vector_type(2)));
        auto ld4 = [&](int o) {
            const lds_v4 v = *(const __attribute__((address_space(3))) lds_v4*)(sp + o);
            return make_float4(v.x, v.y, v.z, v.w);
        };
        auto ld_a = [&](int o) { return ld4(o); };
        auto ld_b = [&](int o) {
            const lds_v2 v = *(const __attribute__((address_space(3))) lds_v2*)(sp + o + 16);
            return make_float2(v.x, v.y);
        };
        auto ld_c = [&](int o) {
            const float4 c = ld4(o + 32);
            // keep the whole 16 bytes of `c` one ds_read_b128 (4 LDS cycles): only r, g, b are used in the loop, and
            // the 12-byte ds_read_b96 the compiler would pick takes 8 -- with it the loop needs 14 LDS cycles per entry
            // and wave, 56 per four SIMDs against 52 cycles of VALU issue: the kernel was LDS-bound
            asm volatile("" ::"v"(c.w));
            return c;
        };
        // ... and the pin of the trip's last read advances `sp` to the next pair of entries, in place: as an ordinary
        // add the compiler issued it early, held old and new address in two registers and paid a copy per trip.  (`mark`:
        // the select of the even entry, which takes the old address, stands in front of the add.)
        auto ld_c_advance = [&](int o, uint32_t& mark) {
            const float4 c = ld4(o + 32);
            asm volatile("v_add_u32 %0, 0x60, %0" : "+v"(sp), "+v"(mark) : "v"(c.w));
            return c;
        };
        // even entries of a run are evaluated with sp at their own address, odd ones with sp 48 bytes past theirs
        const uint32_t sp0 = sp;
        uint32_t mark_e = mark_none_even(sp0), mark_o = mark_none_odd(sp0);  // (blend.h: marks_last_entry)
        // entries [j0, j1) of the batch (sp stands at entry j0, and at entry j1 afterwards)
        auto run = [&](const int j0, const int j1) {
            float4 a0 = ld_a(0), c0 = ld_c(0);
            float2 b0 = ld_b(0);
            int j = j0;
            for (; j + 1 < j1; j += 2) {
                const float4 a1 = ld_a(48), c1 = ld_c(48);
                const float2 b1 = ld_b(48);
                blend(a0, b0, c0, mark_e);
                a0 = ld_a(96); b0 = ld_b(96); c0 = ld_c_advance(96, mark_e);
                blend(a1, b1, c1, mark_o);
            }
            if (j < j1) {
                blend(a0, b0, c0, mark_e);
                sp += 48;
            }
        };
        // A chunk of the backward starts at every compacted index c BWD_CH, 0 < c < chunks (common.h, BWD_CH) -- at the
        // index itself, wherever it falls in a batch, so that the chunks do not depend on how the list is cut into
        // batches (the tile's list, or the recorded quadrant list for a second render of the same geometry: the same
        // gradient bits).  At most one such index per batch (64 <= BWD_CH): the batch runs in two parts around it.
        int jc = cnt;
        if (chunks > 1) {
            const uint32_t r = (BWD_CH - (kbase & (BWD_CH - 1u))) & (BWD_CH - 1u);
            if (r < (uint32_t)cnt && kbase + r > 0u && kbase + r < (uint32_t)chunks * BWD_CH) jc = (int)r;
        }
        run(0, jc);
        if (jc < cnt) {
            nck = (int)((kbase + (uint32_t)jc) / BWD_CH);  // (this is checkpoint nck - 1: they come in order)
            ckpt[((size_t)(tile * 4 + q) * (size_t)(chunks - 1) + (size_t)(nck - 1)) * 64 + lane] = make_float4(fabsf(T), C0, C1, C2);
            if (lane == 0) ck_start[(size_t)(tile * 4 + q) * (size_t)chunks + nck] = kbase + (uint32_t)jc;
            run(jc, cnt);
        }
        // the last blended entry of the batch, 1-based (0: none), and with it the pixel's last contributor so far as a
        // compacted index and as a position in the TILE's list (n_contrib: looked up once per batch)
        const uint32_t jl = marks_last_entry(mark_e, mark_o, sp0);
        if (jl) {
            last_k = kbase + jl;
            last = __float_as_uint(srec[(jl - 1u) * 3 + 2].w);
        }
        live = __ballot(T > 0.f) != 0ull;  // every pixel of the quadrant frozen: stop
    }
    {
        const uint32_t nm = wave_max_u32(last_k);
        if (lane == 0) qcount[tile * 4 + q] = nm;  // the backward's loop bound / work estimate for this quadrant
        // chunks of the backward that never began
        if (chunks > 1 && lane > nck && lane < chunks) ck_start[(size_t)(tile * 4 + q) * (size_t)chunks + lane] = 0xFFFFFFFFu;
    }
    float l1 = 0.f;
    if (inside) {
        const size_t HW = (size_t)H * W;
        const size_t pid = (size_t)py * W + px;
        const float Tf = fabsf(T);
        final_T[pid] = Tf;
        n_contrib[pid] = FQ ? A.src_n_contrib[pid] : last;
        ncon_c[pid] = last_k;
        const float o0 = C0 + Tf * bg[0], o1 = C1 + Tf * bg[1], o2 = C2 + Tf * bg[2];
        out_color[pid] = o0;
        out_color[HW + pid] = o1;
        out_color[2 * HW + pid] = o2;
        l1 = (fabsf(o0 - gt0) + fabsf(o1 - gt1)) + fabsf(o2 - gt2);
    }
    if (A.l1_target) {  // (wave-uniform) the quadrant's share of the fused L1 loss, summed in the DPP ladder's fixed order
        l1 = wave_sum(l1);
        if (lane == 0) A.l1_part[tile * 4 + q] = l1;
    }
}

template <bool FQ>
__device__ __forceinline__ void render_fwd_body(const FwdArgs& A, float4* __restrict__ srec) {
    int slot, q;
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.all_ones) *A.all_ones = (A.not_ones && *A.not_ones == 0ull) ? 1u : 0u;
    const int b = (int)blockIdx.x;
    const bool composite = !(FQ && A.not_ones && *A.not_ones == 0ull);
    render_block_map(b, A.xmap, &slot, &q);
    if (slot < A.ntiles && composite) {
        const uint32_t ov = A.order[slot];  // heaviest tiles first (tile_order_kernel)
        render_quadrant_1<FQ>(A, (int)(ov & 0x7FFFFFFFu), q, srec);
    }
    // The side job BEHIND the wave's own work (same-box A/B, config 3, whole step: no side job 617.3 us; here 611.5 us;
    // between the wave's first gathers and its loop 624.9 us -- the stores queue in front of every wave's second batch)
    forward_side_fill(A);
}

template <bool FQ>
__global__ __launch_bounds__(64, 8) void render_fwd_kernel(const FwdArgs A) {  // (eight waves per SIMD: at most 64 VGPRs)
    __shared__ float4 srec[66 * 3];
    render_fwd_body<FQ>(A, srec);
}

// ---------------------------------------------------------------------------------------------------------------
// The forward for SMALL images (up to FWD4_MAX_TILES tiles), where one wave per quadrant leaves most of the chip idle
// and the frame time is the longest quadrant's chain of dependent steps (a trained avatar at 512 x 512: 150 tiles with
// lists of 2000-7000 entries, a quadrant wave alone on its SIMD for 0.3 ms).  FOUR waves per quadrant, one workgroup:
// every wave owns 16 pixels (two rows of the quadrant) and evaluates FOUR consecutive entries per step -- lane 4 p + e
// holds pixel p against entry j + e.  The four alphas are independent; what is sequential per pixel -- transmittance,
// the 1e-4 stop, the last contributor -- runs down the four lanes of the pixel's quad with quad-permute DPP in exactly
// the operation order of the one-entry-per-step kernel (T bit-identical; the colour sums associate differently:
// per-lane partial sums, added up at the end).  A step costs ~45 VALU instructions for 4 x 16 pairs against 4 x 26 for
// four dependent steps of 64 pairs: 1.7 x the work per pair, less than half the dependent chain; the staging pass takes
// 256 entries of the tile's list at a time (a quarter of the batches).  Same outputs and side records (qlist, ncon_c,
// qcount, checkpoints) as render_fwd_kernel.
// ---------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float qperm(float v) {
    // (every lane of a quad permute has a source: `old` is never kept; passing v itself spares the v_mov that sets it)
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t qperm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
// v * (value of `t` in the lane before, lane 0 of a quad: its own) as ONE instruction: the quad permute rides in the multiply
// (left to the compiler, which folds the v_mov_dpp into the multiply and keeps the two wait states a DPP read of a value
// just written needs; hand-written asm would have to carry its own s_nop)
__device__ __forceinline__ float mul_qprev(float t, float v) {
    const int i = __builtin_bit_cast(int, t);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x90, 0xF, 0xF, false)) * v;
}
#define QP_PREV 0x90   // quad_perm [0,0,1,2]: the lane before (lane 0 of the quad: itself)
#define QP_PAIR 0x44   // quad_perm [0,1,0,1]
#define QP_X1 0xB1     // quad_perm [1,0,3,2]
#define QP_X2 0x4E     // quad_perm [2,3,0,1]
#define QP_LAST 0xFF   // quad_perm [3,3,3,3]
#define FWD4_BATCH 256

// Four waves, one quadrant (tile, q), four entries per step.  `srec`: LDS for FWD4_BATCH + 12 staged entries (a batch's
// compacted entries and four all-zero ones behind them); s_cnt / s_flag / s_lastk: four words each.
template <bool FQ>
__device__ __forceinline__ void render_quadrant_4(const FwdArgs& A, const int tile, const int q, float4* __restrict__ srec,
                                                  uint32_t* __restrict__ s_cnt, uint32_t* __restrict__ s_flag,
                                                  uint32_t* __restrict__ s_lastk) {
    const float4* __restrict__ rec = A.rec;
    const uint32_t* __restrict__ point_list = A.point_list;
    const uint2* __restrict__ ranges = A.ranges;
    const float* __restrict__ bg = A.bg;
    const int W = A.W, H = A.H, gx = A.gx, chunks = A.chunks;
    float* __restrict__ out_color = A.out_color;
    float* __restrict__ final_T = A.final_T;
    uint32_t* __restrict__ n_contrib = A.n_contrib;
    uint32_t* __restrict__ qlist = A.qlist;
    uint32_t* __restrict__ ncon_c = A.ncon_c;
    uint32_t* __restrict__ qcount = A.qcount;
    float4* __restrict__ ckpt = A.ckpt;
    uint32_t* __restrict__ ck_start = A.ck_start;
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int p = lane >> 2, e = lane & 3;  // pixel of this wave (two rows of eight), entry slot of the step
    const bool e0 = e == 0;
    const uint32_t e0_mask = e0 ? 0xFFFFFFFFu : 0u;
    const int QX0 = tx * TILE + 8 * (q & 1), QY0 = ty * TILE + 8 * (q >> 1);
    const int px = QX0 + (p & 7), py = QY0 + 2 * wv + (p >> 3);
    const float pxf = (float)px, pyf = (float)py;
    const bool inside = px < W && py < H;
    const int pix_q = 16 * wv + p;  // the pixel's index in the quadrant, (py - QY0) * 8 + (px - QX0)
    const uint2 range = ranges[tile];
    const int n_tile = (int)(range.y - range.x);
    const uint32_t qbase = 4u * range.x + (uint32_t)q * (uint32_t)n_tile;
    const int n = FQ ? (int)A.src_qcount[tile * 4 + q] : n_tile;  // (render_quadrant_1)
    const uint32_t* __restrict__ list = FQ ? qlist + qbase : point_list + range.x;
    const size_t quad = (size_t)(tile * 4 + q);
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    // Transmittance as TWO values (round 4; until then one, frozen as -T like render_fwd_kernel's): Tc, the running product
    // T (1 - a) (1 - a') ... over EVERY entry evaluated so far, in list order -- it only ever decreases, so "the pixel is done"
    // (an entry took it below 1e-4) is simply Tc < 1e-4, for good, and every later entry fails the test by itself -- and Tf,
    // the value after the last entry that passed: final_T.  The sequential part of a step is then three multiplies (each
    // with its quad permute folded in) instead of three rounds of permute + multiply + select, and the pass / freeze
    // bookkeeping hangs off the chain instead of sitting on it.  The same multiplications in the same order as before: T,
    // final_T, n_contrib, the recorded lists and the colours are bit for bit what the frozen-sign form produced.
    float Tc = inside ? 1.0f : 0.0f, Tf = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f;  // C: this lane's share of the pixel's colour
    float gt0 = 0.f, gt1 = 0.f, gt2 = 0.f;  // the fused L1 loss's target values of this pixel, requested up front (render_quadrant_1)
    if (A.l1_target && inside && e0) {
        const size_t HW = (size_t)H * W, pid = (size_t)py * W + px;
        gt0 = A.l1_target[pid]; gt1 = A.l1_target[HW + pid]; gt2 = A.l1_target[2 * HW + pid];
    }
    uint32_t last = 0, last_k = 0;
    uint32_t kcount = 0;
    int nck = 0;
    bool live = QX0 < W && QY0 < H;  // (workgroup-uniform) the quadrant has a pixel inside the image

#ifdef FWD4_PROF
    // variant build only (tools/fwd4_prof.py): cycles of thread 0 per phase, printed for the heaviest tile's quadrant 0
    unsigned long long pf_t0 = __builtin_readcyclecounter(), pf_stage = 0, pf_loop = 0, pf_tail = 0, pf_mark = 0;
    uint32_t pf_batches = 0, pf_steps = 0;
#define PF_MARK() (pf_mark = __builtin_readcyclecounter())
#define PF_ADD(x) do { const unsigned long long pf_n = __builtin_readcyclecounter(); x += pf_n - pf_mark; pf_mark = pf_n; } while (0)
#else
#define PF_MARK() ((void)0)
#define PF_ADD(x) ((void)0)
#endif
    float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
    uint32_t pid_g = 0, pid_n = 0;  // (two deep, as in render_quadrant_1)
    if (live && tid < n) {
        pid_g = list[tid];
        p0 = rec[(size_t)pid_g * 3];
        p1 = rec[(size_t)pid_g * 3 + 1];
        p2 = rec[(size_t)pid_g * 3 + 2];
    }
    if (live && FWD4_BATCH + tid < n) pid_n = list[FWD4_BATCH + tid];
    for (int base = 0; base < n && live; base += FWD4_BATCH) {
        // (the index fetched two batches ahead is waited for HERE, where everything older has long arrived: left pending,
        // the compiler waits for it -- vmcnt(0), i.e. for this batch's qlist store too -- right before the next prefetch)
        asm volatile("" : "+v"(pid_n));
        PF_MARK();
        Staged s;
        bool hit;
        if (FQ) {
            stage_entry_convert(p0, p1, p2, s);
            hit = base + tid < n;
        } else {
            hit = stage_entry_quad(p0, p1, p2, QX0, QY0, s) && (base + tid < n);
        }
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(bal);
        lds_barrier();  // (the previous batch's readers of srec are done, too)
        const uint32_t n0 = s_cnt[0], n1 = s_cnt[1], n2 = s_cnt[2], n3 = s_cnt[3];
        const int cnt = (int)(n0 + n1 + n2 + n3);
        const uint32_t woff = wv == 0 ? 0u : (wv == 1 ? n0 : (wv == 2 ? n0 + n1 : n0 + n1 + n2));
        // Entry k of the quadrant's compacted list is always evaluated by lane k mod 4 of the quads, however the list is cut
        // into batches: the per-lane colour sums are then the same whether the walk goes over the tile's list (256 list
        // entries per batch) or over the recorded quadrant list (256 hits per batch: a second render of the same
        // geometry) -- bit-identical images.  The batch is staged behind `lead` = kcount mod 4 all-zero entries.
        const uint32_t lead = kcount & 3u;
        if (hit) {
            const uint32_t sl = woff + (uint32_t)__popcll(bal & lt_mask);
            s.c.w = __uint_as_float((uint32_t)(base + tid + 1));  // position in the tile's list (1-based)
            srec[(lead + sl) * 3] = s.a;
            srec[(lead + sl) * 3 + 1] = s.b;
            srec[(lead + sl) * 3 + 2] = s.c;
            if (!FQ) qlist[qbase + kcount + sl] = pid_g;  // record the compaction for the backward
        }
        if (tid < 7) {  // entries of opacity 0 before (lead) and behind the batch: a step always evaluates four
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const uint32_t zs = tid < 4 ? lead + (uint32_t)cnt + (uint32_t)tid : (uint32_t)tid - 4u;
            if (tid < 4 || zs < lead) {
                srec[zs * 3] = z;
                srec[zs * 3 + 1] = z;
                srec[zs * 3 + 2] = z;
            }
        }
        lds_barrier();
        const uint32_t kbase = kcount;  // compacted index of this batch's first entry
        kcount += (uint32_t)cnt;
        if (base + FWD4_BATCH + tid < n) {
            pid_g = pid_n;
            p0 = rec[(size_t)pid_g * 3];
            p1 = rec[(size_t)pid_g * 3 + 1];
            p2 = rec[(size_t)pid_g * 3 + 2];
            if (base + 2 * FWD4_BATCH + tid < n) pid_n = list[base + 2 * FWD4_BATCH + tid];
        }
        // a chunk of the backward starts where the previous one has its BWD_CH entries (common.h, BWD_CH): at a step
        // boundary, here also in the middle of a batch (a batch holds up to 256 entries)
        auto checkpoint = [&](const uint32_t k0) {  // k0 = c BWD_CH: checkpoint c - 1
            float s0 = C0 + qperm<QP_X1>(C0), s1 = C1 + qperm<QP_X1>(C1), s2 = C2 + qperm<QP_X1>(C2);
            s0 += qperm<QP_X2>(s0);
            s1 += qperm<QP_X2>(s1);
            s2 += qperm<QP_X2>(s2);
            nck = (int)(k0 / BWD_CH);  // (they come in order)
            if (e0) ckpt[(quad * (size_t)(chunks - 1) + (size_t)(nck - 1)) * 64 + pix_q] = make_float4(Tc >= 0.0001f ? Tc : Tf, s0, s1, s2);
            if (tid == 0) ck_start[quad * (size_t)chunks + nck] = k0;
        };
        // the next chunk boundary this batch can meet (steps start at multiples of four: every c BWD_CH is a step boundary;
        // one before kbase -- lead > 0 -- was this step's boundary in the previous batch already), or none
        uint32_t ck_next = 0xFFFFFFFFu;
        if (chunks > 1) {
            const uint32_t k = (max(kbase, 1u) + BWD_CH - 1u) & ~(BWD_CH - 1u);
            if (k < (uint32_t)chunks * BWD_CH) ck_next = k;
        }
        auto ck_due = [&](const uint32_t k) {
            if (k != ck_next) return false;
            ck_next = (k + BWD_CH < (uint32_t)chunks * BWD_CH) ? k + BWD_CH : 0xFFFFFFFFu;
            return true;
        };
        PF_ADD(pf_stage);
#ifdef FWD4_PROF
        pf_batches++;
        pf_steps += (lead + (uint32_t)cnt + 3u) / 4u;
#endif
        const char* sp = reinterpret_cast<const char*>(srec) + e * 48;
        const uint32_t kstep0 = kbase - lead;              // compacted index of the batch's first step (its lead entries: done)
        const int nstaged = (int)lead + cnt;
        uint32_t idx1 = kstep0 + (uint32_t)e + 1u;         // compacted index of this lane's entry, 1-based
        // one step: the four entries a / b / c hold (one per lane of the quad) against the wave's 16 pixels
        auto step = [&](const float4 a, const float2 b, const float4 c) {
            const float dx = a.x - pxf, dy = a.y - pyf;
            const float power2 = __builtin_fmaf(a.z * dx, dx, __builtin_fmaf(a.w, dx, b.x * dy) * dy);
            const float G = __builtin_amdgcn_exp2f(power2);
            const float al = fminf(0.99f, b.y * G);
            const float a2 = (power2 <= 0.0f && al >= (1.0f / 255.0f)) ? al : 0.f;  // alpha, or 0 if the pair is rejected
            // T before this lane's entry: Tc times (1 - a2) of the lanes before it, multiplied up in list order -- three rounds
            // settle lanes 1, 2, 3; lane 0 multiplies by 1 (its own value comes back from the permute)
            const float x = 1.f - a2;
            // (a bit select, one v_bfi: written as `e0 ? 1 : ...` the compiler branches around the permute)
            const float xs = __uint_as_float((__float_as_uint(qperm<QP_PREV>(x)) & ~e0_mask) | (0x3F800000u & e0_mask));
            float tb = Tc;
#pragma unroll
            for (int r = 0; r < 3; r++) tb = mul_qprev(tb, xs);
            const float ta = tb * x;  // == tb for a rejected pair
            // Tc only decreases: an entry passes the 1e-4 test exactly when it and every entry before it do
            const bool pass = ta >= 0.0001f;
            const float w = pass ? a2 * tb : 0.f;
            C0 += c.x * w;
            C1 += c.y * w;
            C2 += c.z * w;
            last_k = (w > 0.f) ? idx1 : last_k;
            idx1 += 4u;
            // final_T so far: the value after the last entry that passed (the passing lanes of a step are a prefix of the
            // quad and their values decrease: the smallest one) -- off the sequential chain
            // (positive floats order like their bit patterns: integer min, no NaN canonicalisation)
            uint32_t cand = pass ? __float_as_uint(ta) : 0x7F800000u;
            cand = min(cand, qperm<QP_X1>(cand));
            cand = min(cand, qperm<QP_X2>(cand));
            Tf = cand != 0x7F800000u ? __uint_as_float(cand) : Tf;
            Tc = qperm<QP_LAST>(ta);  // the product over all four entries, in order
        };
        auto ld_a = [&](int o) { return *reinterpret_cast<const float4*>(sp + o); };
        auto ld_b = [&](int o) { return *reinterpret_cast<const float2*>(sp + o + 16); };
        auto ld_c = [&](int o) {
            const float4 c = *reinterpret_cast<const float4*>(sp + o + 32);
            asm volatile("" ::"v"(c.w));  // one ds_read_b128 (render_quadrant_1)
            return c;
        };
        // two steps per trip over two register sets: the next step's LDS reads are issued before the current one is
        // evaluated (reads up to one step past the padded batch: srec has the room; what is read there is never used)
        float4 a0 = ld_a(0), c0 = ld_c(0);
        float2 b0 = ld_b(0);
        int j = 0;
        for (; j + 4 < nstaged; j += 8) {
            if (ck_due(kstep0 + (uint32_t)j)) checkpoint(kstep0 + (uint32_t)j);  // (workgroup-uniform)
            const float4 a1 = ld_a(192), c1 = ld_c(192);
            const float2 b1 = ld_b(192);
            step(a0, b0, c0);
            if (ck_due(kstep0 + (uint32_t)j + 4u)) checkpoint(kstep0 + (uint32_t)j + 4u);
            a0 = ld_a(384); c0 = ld_c(384); b0 = ld_b(384);
            sp += 384;
            step(a1, b1, c1);
        }
        if (j < nstaged) {
            if (ck_due(kstep0 + (uint32_t)j)) checkpoint(kstep0 + (uint32_t)j);
            step(a0, b0, c0);
        }
        PF_ADD(pf_loop);
        {
            uint32_t lk = max(last_k, qperm<QP_X1>(last_k));
            lk = max(lk, qperm<QP_X2>(lk));
            last_k = lk;  // the pixel's last contributor so far
            // its position in the TILE's list (n_contrib), looked up once per batch
            if (lk > kbase) last = __float_as_uint(srec[(lk - 1u - kstep0) * 3 + 2].w);
        }
        const bool alive = __ballot(Tc >= 0.0001f) != 0ull;
        if (lane == 0) s_flag[wv] = alive ? 1u : 0u;
        lds_barrier();
        live = (s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]) != 0u;  // every pixel of the quadrant frozen: stop
        PF_ADD(pf_tail);
    }
#ifdef FWD4_PROF
    if (tid == 0 && blockIdx.x < 8)
        printf("fwd4prof block %d tile %d q %d: list %d batches %u steps %u | cycles total %llu stage %llu loop %llu tail %llu\n", (int)blockIdx.x, tile, q, n,
               pf_batches, pf_steps, (unsigned long long)(__builtin_readcyclecounter() - pf_t0), pf_stage, pf_loop, pf_tail);
#endif
    {
        const uint32_t wm = wave_max_u32(last_k);
        if (lane == 0) s_lastk[wv] = wm;
        lds_barrier();
        if (tid == 0) qcount[quad] = max(max(s_lastk[0], s_lastk[1]), max(s_lastk[2], s_lastk[3]));
        if (chunks > 1 && tid > nck && tid < chunks) ck_start[quad * (size_t)chunks + tid] = 0xFFFFFFFFu;  // never begun
    }
    float s0 = C0 + qperm<QP_X1>(C0), s1 = C1 + qperm<QP_X1>(C1), s2 = C2 + qperm<QP_X1>(C2);
    s0 += qperm<QP_X2>(s0);
    s1 += qperm<QP_X2>(s1);
    s2 += qperm<QP_X2>(s2);
    float l1 = 0.f;
    if (inside && e0) {
        const size_t HW = (size_t)H * W;
        const size_t pid = (size_t)py * W + px;
        final_T[pid] = Tf;
        n_contrib[pid] = FQ ? A.src_n_contrib[pid] : last;
        ncon_c[pid] = last_k;
        const float o0 = s0 + Tf * bg[0], o1 = s1 + Tf * bg[1], o2 = s2 + Tf * bg[2];
        out_color[pid] = o0;
        out_color[HW + pid] = o1;
        out_color[2 * HW + pid] = o2;
        l1 = (fabsf(o0 - gt0) + fabsf(o1 - gt1)) + fabsf(o2 - gt2);
    }
    if (A.l1_target) {  // (workgroup-uniform) the four waves' shares, added in wave order
        l1 = wave_sum(l1);
        lds_barrier();  // (s_lastk has been read by thread 0)
        if (lane == 0) s_lastk[wv] = __float_as_uint(l1);
        lds_barrier();
        if (tid == 0)
            A.l1_part[quad] = (__uint_as_float(s_lastk[0]) + __uint_as_float(s_lastk[1])) + (__uint_as_float(s_lastk[2]) + __uint_as_float(s_lastk[3]));
    }
}

// Small images: one workgroup of four waves per quadrant.  Quadrants of tiles whose list is long against the frame's
// total (tile_order_kernel marks them in the launch order) are rendered by all four waves, four entries per step; the
// others by the first wave alone, as on large images -- there the chip is busy anyway and the one-entry step does the
// same work in 0.6 x the instructions.
template <bool FQ>
__global__ __launch_bounds__(FWD4_BATCH) void render_fwd_small_kernel(const FwdArgs A) {
    __shared__ float4 srec[(FWD4_BATCH + 12) * 3];
    __shared__ uint32_t s_cnt[4], s_flag[4], s_lastk[4];
    int slot, q;
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.all_ones) *A.all_ones = (A.not_ones && *A.not_ones == 0ull) ? 1u : 0u;
    render_block_map((int)blockIdx.x, A.xmap, &slot, &q);
    if (slot < A.ntiles && !(FQ && A.not_ones && *A.not_ones == 0ull)) {
        const uint32_t ov = A.order[slot];  // heaviest tiles first; bit 31: all four waves (tile_order_kernel)
        if (ov >> 31) {
            render_quadrant_4<FQ>(A, (int)(ov & 0x7FFFFFFFu), q, srec, s_cnt, s_flag, s_lastk);
        } else if (threadIdx.x < 64) {
            render_quadrant_1<FQ>(A, (int)ov, q, srec);  // (no workgroup barrier inside: the other waves do the side job)
        }
    }
    forward_side_fill(A);
}

int launch_render_forward(const float* rec, const uint32_t* point_list, const uint32_t* ranges, const uint32_t* order,
                          const float* bg, int W, int H, float* out_color, float* final_T, uint32_t* n_contrib,
                          const QuadLists& ql, hipStream_t s) {
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int xmap = gs_tune_get(GS_TUNE_XCD_MAP);
    const FwdArgs A{reinterpret_cast<const float4*>(rec), point_list, reinterpret_cast<const uint2*>(ranges), order, bg, W, H, gx,
                    gx * gy, xmap, out_color, final_T, n_contrib, ql.qlist, ql.ncon_c, ql.qcount, ql.ckpt, ql.ck_start,
                    ql.ckpt ? ql.chunks : 1, ql.src_qcount, ql.src_n_contrib, ql.not_ones, ql.marks, ql.mark_quads, ql.marks_flag, ql.all_ones,
                    ql.l1_target, ql.l1_part};
    const dim3 grid(render_grid_blocks(gx * gy, xmap));
    const bool fq = ql.src_qcount != nullptr;  // a second render of the same geometry: walk the recorded quadrant lists
    // frames of few long lists (small images; GsFwdArgs.long_lists): four waves per quadrant, all used where
    // tile_order_kernel marked the tile's list as long
    if (ql.four_waves) {
        if (fq) hipLaunchKernelGGL(render_fwd_small_kernel<true>, grid, dim3(FWD4_BATCH), 0, s, A);
        else hipLaunchKernelGGL(render_fwd_small_kernel<false>, grid, dim3(FWD4_BATCH), 0, s, A);
    } else {
        if (fq) hipLaunchKernelGGL(render_fwd_kernel<true>, grid, dim3(64), 0, s, A);
        else hipLaunchKernelGGL(render_fwd_kernel<false>, grid, dim3(64), 0, s, A);
    }
    GS_LAUNCH_CHECK("render_forward", 0, s);
    if (ql.l1_target)  // the fused L1 loss: the quadrants' partial sums, added in index order, over the 3 H W elements
        return launch_loss_final(ql.l1_part, gx * gy * 4, 1.0f / (3.0f * (float)W * (float)H), ql.l1_loss, s);
    return GS_OK;
}

// The opacity render -- what a second rasterizer call with colours = 1 returns in every channel
// (gaussian_renderer/__init__.py:132-142): sum_i alpha_i T_i + T_final * bg = (1 - T_final) + T_final * bg[0].
// The forward already has T_final per pixel, so no second render is needed.
__global__ __launch_bounds__(256) void opacity_image_kernel(const float* __restrict__ final_T, const float* __restrict__ bg,
                                                            int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float Tf = final_T[i];
    out[i] = (1.0f - Tf) + Tf * bg[0];
}

int launch_opacity_image(const float* final_T, const float* bg, int W, int H, float* out, hipStream_t s) {
    const int n = W * H;
    hipLaunchKernelGGL(opacity_image_kernel, dim3((n + 255) / 256), dim3(256), 0, s, final_T, bg, n, out);
    GS_LAUNCH_CHECK("opacity_image", 0, s);
    return GS_OK;
}
