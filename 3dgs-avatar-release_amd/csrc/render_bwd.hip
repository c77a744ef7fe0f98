// render_bwd.hip -- backward of the per-tile compositing (replaces upstream
// renderCUDA backward and its 9 float atomicAdds per (pixel, Gaussian) pair).
//
// CDNA4 formulation -- GAUSSIAN-PARALLEL, no atomics at all:
//  * One wave64 per 8x8 quadrant.  The forward recorded the quadrant's compacted list (qlist) of the
//    Gaussians whose footprint reaches it, up to its last contributor.
//  * LANES ARE LIST ENTRIES, the pixels stream through them.  The wave is FOUR RINGS of 16 lanes (the
//    rows DPP row_ror:1 rotates); ring r owns 16 of the 64 pixels and all four rings hold the same 16
//    entries: entry e sits at position e mod 16 of every ring for the 16 steps e .. e+15, and at step s
//    works on the pixel at ring position s - e.  A pixel's running state (T and the not yet composited
//    part of Gtot) therefore moves one lane per step and visits the entries front to back, exactly like
//    the forward.  The pipeline is skewed, so it never drains between chunks of 16 entries ("rounds"):
//    only the first and last 15 steps of a quadrant run partly empty (a single 64-lane ring wasted 63
//    steps per quadrant, 22 % of all steps on the benchmark scene).
//    (The pixel-parallel formulation needs a 64-lane reduction of nine values per list entry; DPP
//    adds issue at half rate on gfx950 (tools/dpp_rate.hip), which made that reduction ~2/3 of the
//    kernel.)
//  * Entries never touch LDS: every lane gathers the record of its entry two chunks ahead (its list
//    word three), converts it at the round boundary, and at its own switch step (ring position == step mod 16) moves it into
//    the working set.  Per-pixel constants (dL/dpixel, position, last-contributor limit) sit in LDS, one
//    array per component, and are read at the lane's current pixel index one step ahead.
//  * Each lane keeps TWO sets of nine gradient sums, named by the parity of the chunk they belong to:
//    lanes that have switched in the current round add into one set, the others still into the other
//    (the nine FMAs issued under complementary exec masks).  A set is complete for every lane one
//    round later: it is folded over the four rings with lane swaps (no LDS), stored by all four rings
//    (ring r the dwords r and 4 + r of the entry's row) and cleared at a round start -- nothing is stored
//    or cleared under a one-lane exec mask, where an instruction costs as much as with 64 lanes.
//  * FRONT-to-back recurrence.  With g = dL/dpixel, Gtot = out_color . g (out_color already holds
//    T_final * bg) and Rem_i = Gtot - sum_{j<=i} (c_j . g) alpha_j T_j,
//        dL/dalpha_i = T_i (c_i . g) - Rem_i / (1 - alpha_i)
//    which is the reference's back-to-front recurrence (accum_rec / T division) rewritten so that T is
//    rebuilt by the same multiplications the forward did.
//  * Output: the nine raw sums of (pair, quadrant) at row gradient_row(...) (common.h), pairs in EMISSION order
//    (Gaussian-major), so the per-Gaussian kernel reads one contiguous span per Gaussian: eight sums in
//    a 32-byte row, the ninth in a dense word array the caller pre-fills with ROW_UNWRITTEN, so it also
//    tells which rows were written.
#include "common.h"
#include "blend.h"

// rotate by one lane inside every row of 16 lanes (DPP row_ror:1)
__device__ __forceinline__ float ring_ror1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xF, 0xF, true));
}
#define RING 16  // lanes per ring; a wave holds 64 / RING rings
#define RING_STRIDE 48  // words between the rings' per-pixel constants in LDS

// x[0..8] += (Gd dx, Gd dy, tdx dx, tdx dy, tdy dy, Gd, wgt gx, wgt gy, wgt gz) on the lanes of `mask`,
// y[0..8] += the same on all other lanes: the nine instructions issued twice under complementary exec
// masks.  (Written as if / else the compiler either flattens the two blocks into three selects per sum
// or indexes the sets through scratch memory.)  The caller runs with all 64 lanes on.
//
// ENTRY SWITCH, riding in the same two blocks.  Position t of every ring takes its entry of the round's chunk at step t --
// one lane per ring and step.  Moving nine values under a one-lane exec mask costs nine VALU issue slots per step (an
// instruction costs the same with 1 or 64 lanes on): here the LDS unit does it instead.  The lanes of `m1 & ~mask` (those
// that switch at the NEXT step; the accumulation is the last thing of a step that reads the entry... and it does not)
// read their new entry from its staged copy straight into the working registers (q0, q1, q2): no other lane is written.
// Round 4: the reads are issued AND waited for inside one asm statement -- in front of and behind the second set's nine
// instructions and the two ring rotations that end a step -- so the compiler never sees a point where loads into q0 / q1
// / q2 are in flight.  (Until round 3 they were issued in the first set's statement and waited for in the second's, with
// a disassembly check at build time as the only guard; same-box A/B of the one-statement form: render_bwd 1 us faster.)
typedef float bwd_f4 __attribute__((ext_vector_type(4)));
// OFF: byte offset of the slot the reads take from, relative to `lds_addr` (the lane's entry in slot 0): an immediate of
// the read, so the two slots cost neither a second address register nor a select at the round start.
template <bool SECOND, int OFF>
__device__ __forceinline__ void split_accumulate(float (&x)[9], float (&y)[9], unsigned long long mask, float Gd, float dx,
                                                 float dy, float tdx, float tdy, float wgt, float gx, float gy,
                                                 float gz, unsigned long long m1, uint32_t lds_addr, bwd_f4& q0, bwd_f4& q1,
                                                 bwd_f4& q2, float& rot0, float& rot1) {
    unsigned long long save;
    // The first statement is the X set alone; the second issues the reads, runs the Y set (and the caller's two ring
    // rotations, `rot0` / `rot1`) in their shadow and waits.  The 30-operand limit of an asm statement is what keeps the X
    // set out of it.  (SECOND: q2 = (b, r2, g2, b2), 16 bytes; otherwise only its first word is used: a 4-byte read.)
    asm volatile(
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, %[m]\n\t"
        "v_fmac_f32 %[x0], %[Gd], %[dx]\n\t"
        "v_fmac_f32 %[x1], %[Gd], %[dy]\n\t"
        "v_fmac_f32 %[x2], %[tdx], %[dx]\n\t"
        "v_fmac_f32 %[x3], %[tdx], %[dy]\n\t"
        "v_fmac_f32 %[x4], %[tdy], %[dy]\n\t"
        "v_add_f32 %[x5], %[x5], %[Gd]\n\t"
        "v_fmac_f32 %[x6], %[w], %[gx]\n\t"
        "v_fmac_f32 %[x7], %[w], %[gy]\n\t"
        "v_fmac_f32 %[x8], %[w], %[gz]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [x0] "+v"(x[0]), [x1] "+v"(x[1]), [x2] "+v"(x[2]), [x3] "+v"(x[3]), [x4] "+v"(x[4]), [x5] "+v"(x[5]), [x6] "+v"(x[6]),
          [x7] "+v"(x[7]), [x8] "+v"(x[8]), [sv] "=&s"(save)
        : [m] "s"(mask), [Gd] "v"(Gd), [dx] "v"(dx), [dy] "v"(dy), [tdx] "v"(tdx), [tdy] "v"(tdy), [w] "v"(wgt), [gx] "v"(gx),
          [gy] "v"(gy), [gz] "v"(gz)
        : "scc");
#define GS_ACC_Y                                     \
        "s_andn2_b64 exec, %[sv], %[m]\n\t"          \
        "v_fmac_f32 %[y0], %[Gd], %[dx]\n\t"         \
        "v_fmac_f32 %[y1], %[Gd], %[dy]\n\t"         \
        "v_fmac_f32 %[y2], %[tdx], %[dx]\n\t"        \
        "v_fmac_f32 %[y3], %[tdx], %[dy]\n\t"        \
        "v_fmac_f32 %[y4], %[tdy], %[dy]\n\t"        \
        "v_add_f32 %[y5], %[y5], %[Gd]\n\t"          \
        "v_fmac_f32 %[y6], %[w], %[gx]\n\t"          \
        "v_fmac_f32 %[y7], %[w], %[gy]\n\t"          \
        "v_fmac_f32 %[y8], %[w], %[gz]\n\t"          \
        "s_mov_b64 exec, %[sv]\n\t"                  \
        "v_mov_b32_dpp %[r0], %[r0] row_ror:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_mov_b32_dpp %[r1], %[r1] row_ror:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "s_waitcnt lgkmcnt(0)"
#define GS_ACC_Y_OUT [y0] "+v"(y[0]), [y1] "+v"(y[1]), [y2] "+v"(y[2]), [y3] "+v"(y[3]), [y4] "+v"(y[4]), [y5] "+v"(y[5]), \
                     [y6] "+v"(y[6]), [y7] "+v"(y[7]), [y8] "+v"(y[8]), [q0] "+v"(q0), [q1] "+v"(q1), [r0] "+v"(rot0), [r1] "+v"(rot1), \
                     [sv] "=&s"(save)
#define GS_ACC_Y_IN [m] "s"(mask), [m1] "s"(m1), [a] "v"(lds_addr), [Gd] "v"(Gd), [dx] "v"(dx), [dy] "v"(dy), [tdx] "v"(tdx), \
                    [tdy] "v"(tdy), [w] "v"(wgt), [gx] "v"(gx), [gy] "v"(gy), [gz] "v"(gz), [o0] "n"(OFF), [o1] "n"(OFF + 16), \
                    [o2] "n"(OFF + 32)
    if constexpr (SECOND) {
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_andn2_b64 exec, %[m1], %[m]\n\t"
            "ds_read_b128 %[q0], %[a] offset:%[o0]\n\t"
            "ds_read_b128 %[q1], %[a] offset:%[o1]\n\t"
            "ds_read_b128 %[q2], %[a] offset:%[o2]\n\t" GS_ACC_Y
            : GS_ACC_Y_OUT, [q2] "+v"(q2)
            : GS_ACC_Y_IN
            : "memory", "scc");
    } else {
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_andn2_b64 exec, %[m1], %[m]\n\t"
            "ds_read_b128 %[q0], %[a] offset:%[o0]\n\t"
            "ds_read_b128 %[q1], %[a] offset:%[o1]\n\t"
            "ds_read_b32 %[q2], %[a] offset:%[o2]\n\t" GS_ACC_Y
            : GS_ACC_Y_OUT, [q2] "+v"(q2.x)
            : GS_ACC_Y_IN
            : "memory", "scc");
    }
#undef GS_ACC_Y
#undef GS_ACC_Y_OUT
#undef GS_ACC_Y_IN
}

// The LAST step of a full round (t = 15): every ring position has switched, so all 64 lanes add into x and the other
// set's nine instructions would run under an empty exec mask -- they are not issued.  The switch reads of this step, which
// had no lane left in this round either, fetch what the NEXT round starts with instead: position 0 of every ring (`m0`)
// takes its entry of the next chunk from the other slot (OFF; staged at this round's start), in the shadow of the nine
// instructions and the two ring rotations, so a round start has no read and no wait of its own.  One statement, as above.
template <bool SECOND, int OFF>
__device__ __forceinline__ void last_accumulate(float (&x)[9], float Gd, float dx, float dy, float tdx, float tdy, float wgt,
                                                float gx, float gy, float gz, unsigned long long m0, uint32_t lds_addr,
                                                bwd_f4& q0, bwd_f4& q1, bwd_f4& q2, float& rot0, float& rot1) {
    unsigned long long save;
#define GS_ACC_L                                     \
        "s_mov_b64 exec, %[sv]\n\t"                  \
        "v_fmac_f32 %[x0], %[Gd], %[dx]\n\t"         \
        "v_fmac_f32 %[x1], %[Gd], %[dy]\n\t"         \
        "v_fmac_f32 %[x2], %[tdx], %[dx]\n\t"        \
        "v_fmac_f32 %[x3], %[tdx], %[dy]\n\t"        \
        "v_fmac_f32 %[x4], %[tdy], %[dy]\n\t"        \
        "v_add_f32 %[x5], %[x5], %[Gd]\n\t"          \
        "v_fmac_f32 %[x6], %[w], %[gx]\n\t"          \
        "v_fmac_f32 %[x7], %[w], %[gy]\n\t"          \
        "v_fmac_f32 %[x8], %[w], %[gz]\n\t"          \
        "v_mov_b32_dpp %[r0], %[r0] row_ror:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_mov_b32_dpp %[r1], %[r1] row_ror:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define GS_ACC_L_OUT [x0] "+v"(x[0]), [x1] "+v"(x[1]), [x2] "+v"(x[2]), [x3] "+v"(x[3]), [x4] "+v"(x[4]), [x5] "+v"(x[5]), \
                     [x6] "+v"(x[6]), [x7] "+v"(x[7]), [x8] "+v"(x[8]), [q0] "+v"(q0), [q1] "+v"(q1), [r0] "+v"(rot0), [r1] "+v"(rot1), \
                     [sv] "=&s"(save)
#define GS_ACC_L_IN [m0] "s"(m0), [a] "v"(lds_addr), [Gd] "v"(Gd), [dx] "v"(dx), [dy] "v"(dy), [tdx] "v"(tdx), [tdy] "v"(tdy), \
                    [w] "v"(wgt), [gx] "v"(gx), [gy] "v"(gy), [gz] "v"(gz), [o0] "n"(OFF), [o1] "n"(OFF + 16), [o2] "n"(OFF + 32)
    if constexpr (SECOND) {
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_mov_b64 exec, %[m0]\n\t"
            "ds_read_b128 %[q0], %[a] offset:%[o0]\n\t"
            "ds_read_b128 %[q1], %[a] offset:%[o1]\n\t"
            "ds_read_b128 %[q2], %[a] offset:%[o2]\n\t" GS_ACC_L
            "s_waitcnt lgkmcnt(0)"
            : GS_ACC_L_OUT, [q2] "+v"(q2)
            : GS_ACC_L_IN
            : "memory");
    } else {
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_mov_b64 exec, %[m0]\n\t"
            "ds_read_b128 %[q0], %[a] offset:%[o0]\n\t"
            "ds_read_b128 %[q1], %[a] offset:%[o1]\n\t"
            "ds_read_b32 %[q2], %[a] offset:%[o2]\n\t" GS_ACC_L
            "s_waitcnt lgkmcnt(0)"
            : GS_ACC_L_OUT, [q2] "+v"(q2.x)
            : GS_ACC_L_IN
            : "memory");
    }
#undef GS_ACC_L
#undef GS_ACC_L_OUT
#undef GS_ACC_L_IN
}

// The per-entry values the inner loop reads, as the three 16-byte quads they are staged with in LDS:
// q0 = (x, y, A2, B2), q1 = (C2, opacity, r, g), q2 = (b, and the entry's colour in a second image of the same geometry)
struct EntryQ {
    bwd_f4 q0, q1, q2;
};
template <int V>
struct bwd_const {  // a compile-time step index, slot offset or flag handed to a generic lambda
    static constexpr int value = V;
};
#define ENT_SLOTS 2  // chunks of 16 staged entries in LDS: the one the lanes are switching to, the one after it

// Entry switch.  Position t of every ring takes its entry of the round's chunk at step t -- one lane per ring and step.
// Moving nine values under a one-lane exec mask costs nine VALU issue slots per step (an instruction costs the same with 1
// or 64 lanes on): here the LDS unit does it instead.  The lanes of `m1 & ~m0` (those that switch at the NEXT step) read
// their new entry from its staged copy straight into the working registers; no other lane is written.  Issue and wait
// sit in one block: between two blocks the compiler would be free to copy registers whose load is still in flight.
// (The statement of its own serves position 0 in front of a wave's FIRST round only: in every later round position 0's
// entry was read by the last step of the round before, last_accumulate.)
template <bool SECOND>
__device__ __forceinline__ void switch_entry(EntryQ& e, uint32_t lds_addr, unsigned long long m0, unsigned long long m1) {
    unsigned long long save;
    if constexpr (SECOND) {
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_andn2_b64 exec, %[m1], %[m0]\n\t"
            "ds_read_b128 %[q0], %[a]\n\t"
            "ds_read_b128 %[q1], %[a] offset:16\n\t"
            "ds_read_b128 %[q2], %[a] offset:32\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            "s_waitcnt lgkmcnt(0)"
            : [q0] "+v"(e.q0), [q1] "+v"(e.q1), [q2] "+v"(e.q2), [sv] "=&s"(save)
            : [a] "v"(lds_addr), [m0] "s"(m0), [m1] "s"(m1)
            : "memory", "scc");
    } else {
        float b = e.q2.x;
        asm volatile(
            "s_mov_b64 %[sv], exec\n\t"
            "s_andn2_b64 exec, %[m1], %[m0]\n\t"
            "ds_read_b128 %[q0], %[a]\n\t"
            "ds_read_b128 %[q1], %[a] offset:16\n\t"
            "ds_read_b32 %[b], %[a] offset:32\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            "s_waitcnt lgkmcnt(0)"
            : [q0] "+v"(e.q0), [q1] "+v"(e.q1), [b] "+v"(b), [sv] "=&s"(save)
            : [a] "v"(lds_addr), [m0] "s"(m0), [m1] "s"(m1)
            : "memory", "scc");
        e.q2.x = b;
    }
}

// OPA: the image has a fourth channel whose "colour" is 1 for every Gaussian -- the opacity render the reference
// obtains with a second rasterizer call (gaussian_renderer/__init__.py:132-142) -- and dL_dopa is the gradient of
// that channel: one more term in (c . g) and in Gtot, nothing else changes.
// MODE 0: one image; 1 (OPA): + the opacity channel; 2 (SECOND): + a second image of the same geometry; 3 (SONES): + a
// second image whose colours are all (1, 1, 1) -- the reference's opacity pass (gaussian_renderer/__init__.py:132-142).
// Modes 1 and 3 run MODE 0's loop: an image of colours one enters through the pixel's starting value alone (see the set-up).  Both 2 and 3 are launched for a second image; each
// leaves at once unless the second image's `all_ones` word says it is its case (the host does not know).
#ifndef BWD_MIN_WAVES
#define BWD_MIN_WAVES 1
#endif
// A GUARD, without effect on the code as it stands: modes 0, 1 and 3 hold 75-76 VGPRs and run six waves per SIMD with or
// without it (measured level).  Builds of this kernel that happened to fit 72 registers ran SEVEN
// and were 8-10 us slower than the same code at six, so a register saved by a later change must not become a seventh
// wave unnoticed.  (-DBWD_MIN_WAVES above six raises the cap with it.)
#ifndef BWD_MAX_WAVES
#define BWD_MAX_WAVES (BWD_MIN_WAVES > 6 ? BWD_MIN_WAVES : 6)
#endif
template <int MODE>
__attribute__((amdgpu_waves_per_eu(BWD_MIN_WAVES, BWD_MAX_WAVES)))
__global__ __launch_bounds__(64, BWD_MIN_WAVES) void render_bwd_kernel(const float4* __restrict__ rec,
                                                        const uint2* __restrict__ ranges,
                                                        const uint32_t* __restrict__ order, int W, int H, int gx,
                                                        int ntiles, int xmap,
                                                        const uint32_t* __restrict__ qlist,
                                                        const uint32_t* __restrict__ ncon_c,
                                                        const uint32_t* __restrict__ qcount,
                                                        const float* __restrict__ out_color,
                                                        const float* __restrict__ dL_dpix,
                                                        const float* __restrict__ dL_dopa,
                                                        const float* __restrict__ final_T, const float* __restrict__ bg,
                                                        float4* __restrict__ qrows, uint32_t* __restrict__ q8,
                                                        const float4* __restrict__ ckpt,
                                                        const uint32_t* __restrict__ ck_start, const int chunks,
                                                        const int blocks_per_chunk, const SecondImage second,
                                                        const L1Grad l1, const float l1_inv_n) {
    constexpr bool OPA = MODE == 1, SECOND = MODE == 2, SONES = MODE == 3;
    if constexpr (SECOND) { if (*second.all_ones != 0u) return; }
    if constexpr (SONES) { if (*second.all_ones == 0u) return; }
    // per-pixel constants, one array per component (adjacent lanes read adjacent words: no bank
    // conflicts; the 32-byte records this replaces cost 8-way conflicts on every step); ring r owns the
    // 16 pixels 16 r .. 16 r + 15, each ring's 16 values stored twice in a row so a round's reads never
    // wrap, and the rings RING_STRIDE = 48 words apart: the four rings' 16-word windows then fall into four
    // different quarters of the banks (at 32 words apart rings 0 / 2 and 1 / 3 collide):  g0, g1, g2, x, y, lim
    // ... stored as PAIRS (one ds_read_b64 per pair: 2 LDS cycles for 8 bytes per lane where two ds_read_b32 take 4 -- with
    // the entry switch done by LDS reads the kernel sits close to the LDS's cycle budget): (g0, g1) (g2, x) (y, lim)
    // [+ (h0, h1) (h2, -)]
    constexpr int NP2 = SECOND ? 5 : 3;
    __shared__ float2 pix[NP2][4 * RING_STRIDE];
    // the converted entries of a chunk, staged by ring 0 at a round start for the switch reads of the NEXT round
    __shared__ bwd_f4 ent[ENT_SLOTS][RING][3];
    int slot, q;
    // chunk-major: all first chunks, heaviest tiles first, then all second chunks, ... (chunks = 1: one wave per quadrant)
    const int chunk = chunks > 1 ? (int)blockIdx.x / blocks_per_chunk : 0;
    render_block_map((int)blockIdx.x - chunk * blocks_per_chunk, xmap, &slot, &q);
    if (slot >= ntiles) return;
    const int tile = (int)(order[slot] & 0x7FFFFFFFu);  // heaviest tiles first (tile_order_kernel on the forward's counts; or the forward's own order, bit 31 = its mark)
    const int tx = tile % gx, ty = tile / gx;
    const int lane = threadIdx.x;
    const int j = lane & (RING - 1), ring = lane / RING;  // position in the ring / which ring
    const int QX0 = tx * TILE + 8 * (q & 1), QY0 = ty * TILE + 8 * (q >> 1);
    // The lane loads the pixel it STARTS with: position i of a ring starts at ring lane (16 - i) mod 16, so lane (ring, j)
    // takes ring position pi = (16 - j) mod 16, pixel `pl` of the quadrant -- T0 and gtot0 are then where the loop wants
    // them (until now every lane loaded pixel `lane` and the two were fetched with a __shfl each).
    const int pi = (RING - j) & (RING - 1), pl = ring * RING + pi;
    const int px = QX0 + (pl & 7), py = QY0 + (pl >> 3);
    const uint2 range = ranges[tile];
    const int n = (int)(range.y - range.x);
    // this wave's entries: [k0, k0 + m) of the quadrant's compacted list (the whole list when chunks = 1)
    const int m_all = (int)qcount[tile * 4 + q];
    const uint32_t ks = chunk > 0 ? ck_start[(size_t)(tile * 4 + q) * (size_t)chunks + chunk] : 0u;
    if (ks >= (uint32_t)m_all) return;  // (also: chunk never begun, ~0)
    const int k0 = (int)ks;
    const uint32_t ke = chunk + 1 < chunks ? ck_start[(size_t)(tile * 4 + q) * (size_t)chunks + chunk + 1] : 0xFFFFFFFFu;
    const int m = (int)min(ke, (uint32_t)m_all) - k0;
    if (m <= 0) return;  // (a chunk holds at least one entry: the gathers below read list word min(k, m - 1))
    const uint32_t qbase = 4u * range.x + (uint32_t)q * (uint32_t)n + (uint32_t)k0;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float gtot0, T0 = 1.0f;  // Gtot of pixel `pl` (what of it is not composited before entry k0), its transmittance there
    {
        // (g0, g1, g2, Gtot) and (x, y, lim): the pixel at position i of its ring meets compacted entry k at
        // step s = k + i, and the pair counts only while k < (its last contributor) <=> s < lim = ncon + i
        float4 c0 = zero4, c1 = make_float4((float)px, (float)py, __uint_as_float((uint32_t)pi), 0.f);
        float3 h = make_float3(0.f, 0.f, 0.f);  // (SECOND) dL/dpixel of the second image
        if (px < W && py < H) {
            const size_t HW = (size_t)H * W;
            const size_t pid = (size_t)py * W + px;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (dL_dpix) { g0 = dL_dpix[pid]; g1 = dL_dpix[HW + pid]; g2 = dL_dpix[2 * HW + pid]; }
            const float o0 = out_color[pid], o1 = out_color[HW + pid], o2 = out_color[2 * HW + pid];
            if (l1.target) {
                // the fused L1 loss (GsFwdArgs.l1_target): d mean|out - target| / d out = sign(out - target) / (3 H W), times
                // the loss's own gradient -- formed here instead of being written to and read from a gradient image
                const float sc = (l1.grad ? l1.grad[0] : 1.0f) * l1_inv_n;
                const float d0 = o0 - l1.target[pid], d1 = o1 - l1.target[HW + pid], d2 = o2 - l1.target[2 * HW + pid];
                g0 += d0 > 0.f ? sc : (d0 < 0.f ? -sc : 0.f);
                g1 += d1 > 0.f ? sc : (d1 < 0.f ? -sc : 0.f);
                g2 += d2 > 0.f ? sc : (d2 < 0.f ? -sc : 0.f);
            }
            c0 = make_float4(g0, g1, g2, o0 * g0 + o1 * g1 + o2 * g2);
            const uint32_t nc = ncon_c[pid];
            c1.z = __uint_as_float((nc > (uint32_t)k0 ? nc - (uint32_t)k0 : 0u) + (uint32_t)pi);
            // An image whose colours are all ONE -- the opacity channel o = (1 - Tf) + Tf bg, or a second render with
            // colours (1, 1, 1) -- needs nothing in the loop: its (c . g) is the same g4 for every entry, and with
            // sum_{j <= i} alpha_j T_j = 1 - T_{i+1} its share of dL/dalpha_i = T_i g4 - Rem_i / (1 - alpha_i) collapses to
            // g4 (1 - o) / (1 - alpha_i), the same constant over (1 - alpha_i) at every entry: it is SUBTRACTED FROM Gtot
            // once, here, and the recurrence carries it (also from a checkpoint: no term there).  (Until round 3: one more
            // pixel constant read and added per step, 265 against 245 us at config 3.)
            if (OPA) {
                const float Tf = final_T[pid];
                c0.w -= dL_dopa[pid] * (Tf * (1.0f - bg[0]));  // g4 (1 - o),  1 - o = Tf (1 - bg)
            }
            if (SECOND || SONES) {
                h = make_float3(second.dL_dpix[pid], second.dL_dpix[HW + pid], second.dL_dpix[2 * HW + pid]);
                if (SECOND) c0.w += second.out_color[pid] * h.x + second.out_color[HW + pid] * h.y + second.out_color[2 * HW + pid] * h.z;
                else c0.w -= (1.0f - second.out_color[pid]) * h.x + (1.0f - second.out_color[HW + pid]) * h.y + (1.0f - second.out_color[2 * HW + pid]) * h.z;
            }
            if (chunk > 0) {
                // the forward's state before entry k0: T, and the colour composited so far (the opacity channel's is 1 - T)
                const size_t ci = ((size_t)(tile * 4 + q) * (size_t)(chunks - 1) + (size_t)(chunk - 1)) * 64 + pl;
                const float4 ck = ckpt[ci];
                T0 = ck.x;
                c0.w -= ck.y * g0 + ck.z * g1 + ck.w * g2;
                if (SECOND) {
                    const float4 ck2 = second.ckpt[ci];  // (the second render's own checkpoints: same T, its colours)
                    c0.w -= ck2.y * h.x + ck2.z * h.y + ck2.w * h.z;
                }
            }
        }
        const int slot = ring * RING_STRIDE + pi;
        pix[0][slot] = pix[0][slot + RING] = make_float2(c0.x, c0.y);
        pix[1][slot] = pix[1][slot + RING] = make_float2(c0.z, c1.x);
        pix[2][slot] = pix[2][slot + RING] = make_float2(c1.y, c1.z);
        if (SECOND) {
            pix[3][slot] = pix[3][slot + RING] = make_float2(h.x, h.y);
            pix[4][slot] = pix[4][slot + RING] = make_float2(h.z, 0.f);
        }
        gtot0 = c0.w;
    }

    // record (p0,p1,p2) -> the loop's entry form, staged in LDS slot `chunk & 1` by ring 0 (the four rings hold the same
    // entries), + the gradient row of (pair, quadrant)
    float3 q2 = make_float3(0.f, 0.f, 0.f);  // (SECOND) the gathered entry's colour in the second image
    auto stage = [&](const float4 p0, const float4 p1, const float4 p2, const int chunk, uint32_t& row) {
        const uint32_t off = __float_as_uint(p2.y), rmin = __float_as_uint(p2.z), rsz = __float_as_uint(p2.w);
        const uint32_t minx = rmin & 0xFFFFu, miny = rmin >> 16, w = rsz & 0xFFFFu;
        row = gradient_row(off, w, (uint32_t)tx - minx, (uint32_t)ty - miny, (uint32_t)q);
        if (ring == 0) {
            bwd_f4* e = ent[chunk & (ENT_SLOTS - 1)][j];
            e[0] = bwd_f4{p0.x, p0.y, (-0.5f * LOG2E_F) * p0.z, -LOG2E_F * p0.w};
            e[1] = bwd_f4{(-0.5f * LOG2E_F) * p1.x, p1.y, p1.z, p1.w};
            if constexpr (SECOND) e[2] = bwd_f4{p2.x, q2.x, q2.y, q2.z};
            else *reinterpret_cast<float*>(e + 2) = p2.x;  // (the only word of the quad a switch reads back)
        }
    };
    // The gathers are UNCONDITIONAL, at list word min(k, m - 1), and the list word is read a round before the record it
    // names.  (Until now `if (k < m) { id = qlist[..]; p = rec[id] }`: the compiler merged the old and the new record inside
    // that branch -- register moves behind an `s_waitcnt vmcnt(0)` -- so every round start waited for two dependent memory
    // round trips it had meant to leave in flight.  A lane past the end of the list holds a copy of the last entry: no
    // pixel meets it before its own limit `lim`, and its sums are never stored.)
    uint32_t id_ahead = 0;  // the list word of this lane's entry one chunk beyond the gathered one
    auto gather_id = [&](int k) { id_ahead = qlist[qbase + min(k, m - 1)]; };
    auto gather = [&](float4& p0, float4& p1, float4& p2) {  // the record `id_ahead` names
        const uint32_t id = id_ahead;
        p0 = rec[(size_t)id * 3];
        p1 = rec[(size_t)id * 3 + 1];
        p2 = rec[(size_t)id * 3 + 2];
        if (SECOND) q2 = make_float3(second.colors[(size_t)id * 3], second.colors[(size_t)id * 3 + 1], second.colors[(size_t)id * 3 + 2]);
    };

    float4 p0 = zero4, p1 = zero4, p2 = zero4;
    EntryQ cur;  // the entry this lane works on (none yet: alpha = 0)
    cur.q0 = cur.q1 = cur.q2 = bwd_f4{0.f, 0.f, 0.f, 0.f};
    uint32_t row_staged = 0;  // gradient row of this lane's entry in the chunk staged last
    gather_id(j);
    gather(p0, p1, p2);                 // (the four rings hold the same entries)
    gather_id(RING + j);
    stage(p0, p1, p2, 0, row_staged);   // chunk 0, taken by position t of every ring at step t
    gather(p0, p1, p2);                 // chunk 1 in flight during round 0
    gather_id(2 * RING + j);            // ... and the list word of chunk 2
    __syncthreads();
    // LDS address of this lane's entry in slot 0; slot 1 lies ENT_SLOT_BYTES behind it, an immediate offset of the reads
    const uint32_t ent_addr0 = (uint32_t)(uintptr_t)&ent[0][j][0];
    constexpr int ENT_SLOT_BYTES = RING * 3 * (int)sizeof(bwd_f4);

    // Two accumulator sets, named by the PARITY of the chunk they belong to: during round R the lanes
    // that have already taken their entry of chunk R (lane <= t) add into set R & 1, the others still
    // add into the set of chunk R - 1.  A set is therefore complete for ALL lanes when round R + 1 ends
    // ... i.e. it is stored (two full-wave dword stores and ring 0's ninth word) and cleared at the start of round R + 2, instead
    // of every lane storing / clearing its own sums at its own switch step under a one-lane exec mask
    // (where every instruction costs as much as a full-wave one).
    float accA[9], accB[9];
#pragma unroll
    for (int c9 = 0; c9 < 9; c9++) accA[c9] = accB[c9] = 0.f;
    uint32_t rowA = 0, rowB = 0;  // gradient rows of the entries the sets belong to
    // index into pix[c][] of the pixel at this lane when a round starts: ring base + (16 - j) mod 16.  Step t of a round
    // reads the constants of step t + 1 at pbase + t + 1 (the 16 values stored twice in a row: no wrap); after 16 steps the
    // lane is back at its first pixel, so every round starts at pbase: the base never moves.
    const uint32_t pbase = (uint32_t)(ring * RING_STRIDE + pi);
    float2 pc[NP2];  // the constants of the pixel at this lane (read at the round start and one step ahead)
    // state of the pixel currently at this lane: transmittance and the part of Gtot not yet composited
    // (the lane loaded the pixel it starts with)
    float T = T0, Rem = gtot0;

    // The four rings hold partial sums of the same entries.  FOLD, without the LDS unit (until now 18 ds_bpermute per fold):
    // v_permlane16_swap on (p, q) exchanges the odd rows of p with the even rows of q, so p + q has the rows
    // [A0+A1, B0+B1, A2+A3, B2+B3] of two sums A, B; v_permlane32_swap on two such registers exchanges the upper half of
    // one with the lower half of the other, and their sum has the rows [A, B, C, D], A = (A0 + A1) + (A2 + A3) -- the
    // association the xor 16, xor 32 ladder gave ring 0, so the stored bits are what they were.  Row r of f[0] is sum r, of
    // f[1] sum 4 + r; f[2] is sum 8 in every row.
    // (One asm statement, the sums folded in place: with the two builtins the register allocator no longer kept the
    // accumulator sets in fixed registers across the rounds -- 94 VGPRs and moves inside the step loop.  `s_nop 1`: a swap
    // must not read a register a VALU instruction wrote within the last two wait states; inside the statement every swap's
    // operands are at least two instructions old.)
    auto fold_rings = [&](float (&a)[9], float (&f)[3]) {
        float t;
        asm volatile(
            "s_nop 1\n\t"
            "v_permlane16_swap_b32 %[a0], %[a1]\n\t"
            "v_permlane16_swap_b32 %[a2], %[a3]\n\t"
            "v_permlane16_swap_b32 %[a4], %[a5]\n\t"
            "v_permlane16_swap_b32 %[a6], %[a7]\n\t"
            "v_mov_b32 %[t], %[a8]\n\t"
            "v_add_f32 %[a0], %[a0], %[a1]\n\t"
            "v_add_f32 %[a2], %[a2], %[a3]\n\t"
            "v_add_f32 %[a4], %[a4], %[a5]\n\t"
            "v_add_f32 %[a6], %[a6], %[a7]\n\t"
            "v_permlane16_swap_b32 %[a8], %[t]\n\t"
            "v_permlane32_swap_b32 %[a0], %[a2]\n\t"
            "v_permlane32_swap_b32 %[a4], %[a6]\n\t"
            "v_add_f32 %[a8], %[a8], %[t]\n\t"
            "v_add_f32 %[a0], %[a0], %[a2]\n\t"
            "v_add_f32 %[a4], %[a4], %[a6]\n\t"
            "v_mov_b32 %[t], %[a8]\n\t"
            "s_nop 1\n\t"
            "v_permlane32_swap_b32 %[a8], %[t]\n\t"
            "v_add_f32 %[a8], %[a8], %[t]"
            : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [a4] "+v"(a[4]), [a5] "+v"(a[5]),
              [a6] "+v"(a[6]), [a7] "+v"(a[7]), [a8] "+v"(a[8]), [t] "=&v"(t));
        f[0] = a[0];
        f[1] = a[4];
        f[2] = a[8];
    };
    // A finished entry's nine RAW sums go to its row in HBM: ring r stores dwords r and 4 + r of the entry's 32-byte row (two
    // full-wave dword stores: the four rings' lanes of an entry fill 16 contiguous bytes each), ring 0 the ninth word.  What
    // is constant per Gaussian -- opacity, the conic combination of the two first moments, the -1/2 and 1/log2(e) factors --
    // is applied once per Gaussian by segment_reduce_kernel.
    float* const qrow_words = reinterpret_cast<float*>(qrows);
    auto write_row = [&](size_t row, const float (&f)[3]) {
        // (plain stores: the rows are read back by segment_reduce_kernel while much of them is still in the L2 / MALL --
        // streaming "nt" stores made the frame 0.15 ms slower)
        qrow_words[row * 8 + ring] = f[0];
        qrow_words[row * 8 + ring + 4] = f[1];
        if (ring == 0) q8[row] = __float_as_uint(f[2]);  // the ninth sum doubles as the "row written" mark
    };

    // An entry k lives at position k mod 16 of every ring for the steps k .. k+15; the loop runs
    // s = 0 .. m+14, so every entry has seen all its pixels when the loop ends.
    const int total = m + RING - 1;
    constexpr unsigned long long POS0 = 0x0001000100010001ull;  // position 0 of every ring
    // Round start (round R = s0 / 16).  X holds the finished sums of chunk R - 2: store them.  The lanes switch to chunk R
    // during this round (staged one round ago): its row is the one noted then.  The chunk that was in flight (R + 1) is
    // converted and staged for the next round; the chunk after it goes in flight.  (Position 0 of every ring holds its
    // entry of chunk R already: read by the last step of round R - 1, in front of round 0 by the statement below.)
    auto round_start = [&](const int s0, float (&X)[9], uint32_t& rowX) {
        // the pixel constants of the round's first step: the same words every round, read here so that no register carries
        // them across the round boundary (the round-start work below hides the read)
#pragma unroll
        for (int c6 = 0; c6 < NP2; c6++) pc[c6] = pix[c6][pbase];
        const uint32_t row_done = rowX;
        rowX = row_staged;
        stage(p0, p1, p2, s0 / RING + 1, row_staged);  // (slot (R + 1) & 1 held chunk R - 1: its reads ended a round ago)
        gather(p0, p1, p2);                            // chunk R + 2
        gather_id(s0 + 3 * RING + j);
        // ... and the stores BEHIND the round's loads: the counter the loads are waited for with counts the stores too, in
        // order, so stores issued in front of them were waited for with them at the next round start
        if (s0 >= 2 * RING) {
            float f[3];
            fold_rings(X, f);
            write_row(row_done, f);
        }
#pragma unroll
        for (int c9 = 0; c9 < 9; c9++) X[c9] = 0.f;
    };
    // One step.  `pnext`: where the NEXT step's pixel constants lie; `mx`: ring positions <= t; OFF: this round's slot;
    // LAST: step 15 of a full round (last_accumulate).
    auto step = [&](const uint32_t s, const uint32_t pnext, const unsigned long long mx, float (&X)[9], float (&Y)[9], auto off,
                    auto last) {
        constexpr int OFF = decltype(off)::value;
        const float3 g = make_float3(pc[0].x, pc[0].y, pc[1].x);  // dL/dpixel of the pixel at this lane
        const float pxf = pc[1].y, pyf = pc[2].x;
        const uint32_t lim = __float_as_uint(pc[2].y);
        const float h0 = SECOND ? pc[NP2 - 2].x : 0.f, h1 = SECOND ? pc[NP2 - 2].y : 0.f, h2 = SECOND ? pc[NP2 - 1].x : 0.f;
        // next step's pixel constants, fetched now (the round's last step fetches none: see round_start)
        if constexpr (!decltype(last)::value) {
#pragma unroll
            for (int c6 = 0; c6 < NP2; c6++) pc[c6] = pix[c6][pnext];
        }
        const float dx = cur.q0.x - pxf, dy = cur.q0.y - pyf;
        // A2 dx^2 + B2 dx dy + C2 dy^2 in five operations
        const float power2 = __builtin_fmaf(cur.q0.z * dx, dx, __builtin_fmaf(cur.q0.w, dx, cur.q1.x * dy) * dy);
        const float G = __builtin_amdgcn_exp2f(power2);
        const float al = fminf(0.99f, cur.q1.y * G);
        // The pair counts iff power <= 0, the entry lies before the pixel's last contributor (s < lim; a lane that
        // has no entry yet holds zeros, i.e. alpha = 0), and alpha >= 1/255 (which implies the forward's relaxed
        // power2 >= thr pre-test): three compares whose lane masks meet in two scalar ANDs, then one select each
        // for alpha and G (rejected pairs carry alpha = 0).  (Until round 2: two selects more in place of the ANDs.)
        const bool valid = (power2 <= 0.0f) && (s < lim) && (al >= (1.0f / 255.0f));
        const float alpha = valid ? al : 0.f;
        const float Gv = valid ? G : 0.f;
        const float wgt = alpha * T;
        float cg = cur.q1.z * g.x + cur.q1.w * g.y + cur.q2.x * g.z;
        if constexpr (SECOND) cg += cur.q2.y * h0 + cur.q2.z * h1 + cur.q2.w * h2;
        Rem = __builtin_fmaf(-cg, wgt, Rem);
        const float one_m = 1.f - alpha;
        const float dL_dalpha = T * cg - Rem * __builtin_amdgcn_rcpf(one_m);
        T *= one_m;
        const float Gd = Gv * dL_dalpha;  // G dL/dalpha; times opacity it is G dL/dG (applied per Gaussian later)
        const float tdx = Gd * dx, tdy = Gd * dy;
        // sums:  0: t dx   1: t dy   2: t dx^2   3: t dx dy   4: t dy^2   5: G dL/dalpha = dL/dopacity
        //        6..8: w g_c = dL/dcolor     (t = Gd)
        // X += ... on the lanes <= t (they have taken their entry of this round's chunk), Y += ... on the others
        // ... and the positions that take their entry at the next step read it meanwhile
        // ... and the pixel moves on to the next entry = the next lane: T and Rem rotate by one lane inside their ring
        if constexpr (decltype(last)::value)
            last_accumulate<SECOND, ENT_SLOT_BYTES - OFF>(X, Gd, dx, dy, tdx, tdy, wgt, g.x, g.y, g.z, POS0, ent_addr0, cur.q0,
                                                          cur.q1, cur.q2, T, Rem);
        else
            split_accumulate<SECOND, OFF>(X, Y, mx, Gd, dx, dy, tdx, tdy, wgt, g.x, g.y, g.z, (mx << 1) | POS0, ent_addr0,
                                          cur.q0, cur.q1, cur.q2, T, Rem);
    };
    // The 16 steps of a round are STRAIGHT-LINE code: the step index is a compile-time constant, so the pixel constants are
    // read at constant offsets from `pbase` and the lane masks are constants -- no index or mask arithmetic in a round.  The
    // wave's last round leaves the sequence behind its last step (elsewhere a scalar compare and a branch not taken per
    // step) and with it the round loop: nothing but the two sets and their rows is alive at such an exit, so no exit costs
    // a register move on the path the full rounds take.  Returns whether the walk ended in this round.
    // (A run-time loop for the partial round NEXT TO the straight-line body -- in either order, inside or behind the round
    // loop -- made the register allocator split the sets' live ranges: 100-118 VGPRs, four waves per SIMD)
    auto run_round = [&](const int s0, float (&X)[9], uint32_t& rowX, float (&Y)[9], auto off) {
        round_start(s0, X, rowX);
        const int left = total - s0;  // steps still to run: all 16 of this round, or fewer
#define GS_STEP(t)                                                                                                         \
    step((uint32_t)(s0 + (t)), pbase + (uint32_t)((t) + 1), ((1ull << ((t) + 1)) - 1ull) * POS0, X, Y, off,                \
         bwd_const<(t) == RING - 1>{});                                                                                    \
    if (left <= (t) + 1) return true
        GS_STEP(0);
        GS_STEP(1);
        GS_STEP(2);
        GS_STEP(3);
        GS_STEP(4);
        GS_STEP(5);
        GS_STEP(6);
        GS_STEP(7);
        GS_STEP(8);
        GS_STEP(9);
        GS_STEP(10);
        GS_STEP(11);
        GS_STEP(12);
        GS_STEP(13);
        GS_STEP(14);
        GS_STEP(15);
        return false;
#undef GS_STEP
    };
    // position 0 of every ring takes its entry of chunk 0 now (the other positions at the end of the step before theirs)
    switch_entry<SECOND>(cur, ent_addr0, 0ull, POS0);
    for (int s0 = 0;; s0 += 2 * RING) {
        if (run_round(s0, accA, rowA, accB, bwd_const<0>{})) break;
        if (run_round(s0 + RING, accB, rowB, accA, bwd_const<ENT_SLOT_BYTES>{})) break;
    }
    {
        // the two chunks still in the sets: the one taken during the last round and the one before it
        const int last_round = (total - 1) / RING;
        const bool odd = last_round & 1;
        const int k_new = RING * last_round + j, k_old = k_new - RING;
        float fA[3], fB[3];
        fold_rings(accA, fA);
        fold_rings(accB, fB);
        if (k_new <= m - 1) write_row(odd ? rowB : rowA, odd ? fB : fA);
        if (last_round >= 1 && k_old <= m - 1) write_row(odd ? rowA : rowB, odd ? fA : fB);
    }
}

int launch_render_backward(const float* rec, const uint32_t* ranges, const uint32_t* order, int W, int H,
                           const QuadLists& ql, const float* out_color, const float* dL_dpix, const float* dL_dopa,
                           const float* final_T, const float* bg, float* qrows, uint32_t* q8, const SecondImage* second,
                           L1Grad l1, hipStream_t s) {
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int xmap = gs_tune_get(GS_TUNE_XCD_MAP);
    const int chunks = ql.ckpt ? ql.chunks : 1;
    const int bpc = render_grid_blocks(gx * gy, xmap);
    const dim3 grid((unsigned)bpc * (unsigned)chunks);
    const SecondImage none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const float l1_inv_n = 1.0f / (3.0f * (float)W * (float)H);
#define GS_BWD_ARGS                                                                                                       \
    reinterpret_cast<const float4*>(rec), reinterpret_cast<const uint2*>(ranges), order, W, H, gx, gx * gy, xmap, ql.qlist, \
        ql.ncon_c, ql.qcount, out_color, dL_dpix, dL_dopa, final_T, bg, reinterpret_cast<float4*>(qrows), q8, ql.ckpt,    \
        ql.ck_start, chunks, bpc
    if (second) {
        hipLaunchKernelGGL(render_bwd_kernel<2>, grid, dim3(64), 0, s, GS_BWD_ARGS, *second, l1, l1_inv_n);  // (one of the two leaves at once)
        hipLaunchKernelGGL(render_bwd_kernel<3>, grid, dim3(64), 0, s, GS_BWD_ARGS, *second, l1, l1_inv_n);
    } else if (dL_dopa)
        hipLaunchKernelGGL(render_bwd_kernel<1>, grid, dim3(64), 0, s, GS_BWD_ARGS, none, l1, l1_inv_n);
    else
        hipLaunchKernelGGL(render_bwd_kernel<0>, grid, dim3(64), 0, s, GS_BWD_ARGS, none, l1, l1_inv_n);
#undef GS_BWD_ARGS
    GS_LAUNCH_CHECK("render_backward", 0, s);
    return GS_OK;
}
