// capi.hip -- the extern "C" boundary declared in include/gsplat_mi355.h.  Host-side sequencing of
// the stages; no device allocation, no implicit synchronisation (except in debug mode).
#include "common.h"
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <mutex>
#include <vector>

static thread_local int g_last_hip = 0;
static thread_local const char* g_last_stage = "";
void gs_set_error(int hip_err, const char* stage) {
    g_last_hip = hip_err;
    g_last_stage = stage;
}

// ---- tuning switches: the one table behind gs_tuning, the defaults and the environment overrides (what each switch
// does is documented at gs_tuning in include/gsplat_mi355.h, name for name)
struct TuneSwitch {
    const char* name;
    int key, def;
    const char* env;   // read once, when the first switch is read; a value the rule rejects is ignored
    bool (*ok)(int);   // null: every value is taken
};
static const TuneSwitch k_tune[GS_TUNE_COUNT] = {
    {"xcd_map", GS_TUNE_XCD_MAP, 1, nullptr, nullptr},
    {"depth_sort", GS_TUNE_DEPTH_SORT, 1, nullptr, nullptr},  // 1 bucket sort, 0 LSD radix
    {"nt_stores", GS_TUNE_NT_STORES, 1, nullptr, nullptr},
    {"bwd_chunks", GS_TUNE_BWD_CHUNKS, 1, nullptr, nullptr},  // flip between frames only
    // GSPLAT_FWD4=0|1|2: the forward of the tiles marked as long on small images -- one wave per quadrant, four waves x four
    // entries per step, or a wave per chunk of the list (render_fwd.hip: render_chunk)
    {"fwd4", GS_TUNE_FWD4, 1, "GSPLAT_FWD4", nullptr},
    {"small_tiles", GS_TUNE_SMALL_TILES, BWD_CHUNK_MAX_TILES, nullptr, nullptr},  // changes the image state's size
    {"shared_qlist", GS_TUNE_SHARED_QLIST, 1, nullptr, nullptr},
    {"ones_fast", GS_TUNE_ONES_FAST, 1, nullptr, nullptr},
    {"bwd_order", GS_TUNE_BWD_ORDER, 1, nullptr, nullptr},  // 0: the backward walks the tiles in the forward's launch order (A/B: + 12 us at config 3)
    {"fwd_marks", GS_TUNE_FWD_MARKS, 1, nullptr, nullptr},  // 0: the backward sets its row marks itself (A/B)
    // entries per chunk of the chunk-parallel forward (a power of two >= 64) ...
    {"fwdc_ch", GS_TUNE_FWDC_CH, (int)FWDC_CH_MIN, "GSPLAT_FWDC_CH", [](int v) { return v >= 64 && (v & (v - 1)) == 0; }},
    // ... of the tiles whose list is longer than (frame's pairs) / this (and than FWD4_MIN_LIST)
    {"fwdc_div", GS_TUNE_FWDC_DIV, (int)FWD4_TOTAL_DIV, "GSPLAT_FWDC_DIV", [](int v) { return v >= 1; }},
};
struct TuneState {
    std::atomic<int> v[GS_TUNE_COUNT];
    TuneState() {
        for (const TuneSwitch& t : k_tune) {
            int value = t.def;
            if (const char* e = t.env ? getenv(t.env) : nullptr) {
                const int x = atoi(e);
                if (!t.ok || t.ok(x)) value = x;
            }
            v[t.key].store(value);
        }
    }
};
// (a function-local static: initialised once however many threads ask first -- the forward's and autograd's backward thread do)
static TuneState& tune_state() {
    static TuneState st;
    return st;
}
int gs_tune_get(int key) {
    return (key >= 0 && key < GS_TUNE_COUNT) ? tune_state().v[key].load(std::memory_order_relaxed) : 0;
}

// ---- per-stage event timing -------------------------------------------------------------------
struct ProfRec { const char* name; hipEvent_t a, b; };
struct ProfState {
    bool on = false;
    bool armed = false;  // the current stage is being timed
    int nested = 0;      // stage scopes opened inside the one being timed (they belong to it: no record of their own)
    char filter[32] = {0};
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
// process-wide (autograd runs the backward on its own host thread), guarded by a mutex
static ProfState g_prof;
static std::mutex g_prof_mu;
static bool profiling_on() { return g_prof.on; }
void gs_prof_begin(const char* stage, hipStream_t s) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof.armed) { g_prof.nested++; return; }
    g_prof.armed = g_prof.on && (g_prof.filter[0] == 0 || strcmp(g_prof.filter, stage) == 0);
    if (!g_prof.armed) return;
    ProfRec r{stage, g_prof.get(), g_prof.get()};
    (void)hipEventRecord(r.a, s);
    g_prof.recs.push_back(r);
}
void gs_prof_end(hipStream_t s) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof.armed || g_prof.recs.empty()) return;
    if (g_prof.nested > 0) { g_prof.nested--; return; }
    (void)hipEventRecord(g_prof.recs.back().b, s);
    g_prof.armed = false;
}

static int validate(const GsFwdArgs* a) {
    if (!a) return GS_E_BAD_ARG;
    if (a->P < 0 || a->W <= 0 || a->H <= 0) return GS_E_BAD_ARG;
    if (!a->bg || !a->viewmatrix || !a->projmatrix || !a->campos) return GS_E_BAD_ARG;
    if (a->P > 0 && (!a->means3D || !a->opacities)) return GS_E_BAD_ARG;
    if ((a->shs != nullptr) == (a->colors_precomp != nullptr)) return GS_E_EXCLUSIVE;
    const bool sr = a->scales != nullptr && a->rotations != nullptr;
    if ((a->scales != nullptr) != (a->rotations != nullptr)) return GS_E_EXCLUSIVE;
    if (sr == (a->cov3D_precomp != nullptr)) return GS_E_EXCLUSIVE;
    if (a->shs) {
        if (a->sh_degree < 0 || a->sh_degree > 3) return GS_E_BAD_ARG;
        if (a->M < (a->sh_degree + 1) * (a->sh_degree + 1)) return GS_E_BAD_ARG;
        if (a->M > 16) return GS_E_BAD_ARG;  // degree <= 3: the per-Gaussian backward stages 3 M floats per thread in LDS
    }
    // quaternions are read (and their gradients written) as float4
    if (a->rotations && ((uintptr_t)a->rotations & 15u)) return GS_E_BAD_ARG;
    if ((a->W + TILE - 1) / TILE > 0xFFFF || (a->H + TILE - 1) / TILE > 0xFFFF) return GS_E_TOO_LARGE;
    return GS_OK;
}

// ---- stream capture (hipGraph) -----------------------------------------------------------------
// Round 3 recorded a GPU memory fault ("write access to a read-only page") on the first replay of a captured
// gs_forward_preprocess + gs_forward_render.  What those two calls put into the graph besides kernel nodes: a memset
// node (the per-tile totals), a device-to-host memcpy node into the caller's pinned count word, and a kernel that
// STORES into pinned host memory (GsFwdArgs.frame_stats).  None of that is needed under capture: the library now asks
// hipStreamIsCapturing at every entry point, enqueues KERNEL NODES ONLY on a capturing stream (zero_words_kernel instead
// of memset nodes), and answers GS_E_CAPTURE -- before enqueuing anything -- to every call that would need more.
static bool stream_is_capturing(void* stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing((hipStream_t)stream, &st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        // (asking about the legacy stream while another stream captures in global mode is itself a capture error)
        return e == hipErrorStreamCaptureImplicit || e == hipErrorStreamCaptureUnsupported || e == hipErrorStreamCaptureInvalidated;
    }
    return st != hipStreamCaptureStatusNone;
}
// capture-safe entry points: refuse debug mode (it synchronises) and the stage timer (event nodes) under capture
#define GS_CAPTURE_OK_IF(stream, cond)                                           \
    do {                                                                         \
        if (stream_is_capturing(stream) && (!(cond) || profiling_on())) return GS_E_CAPTURE; \
    } while (0)
#define GS_NO_CAPTURE(stream) GS_CAPTURE_OK_IF(stream, false)

__global__ void zero_words_kernel(uint32_t* __restrict__ p, size_t words) {
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += (size_t)gridDim.x * blockDim.x) p[k] = 0u;
}
// `bytes` (a multiple of 4) of zeros as a kernel node (a memset node in eager mode would do: one code path for both)
int gs_zero_async(void* ptr, size_t bytes, const char* stage, hipStream_t s) {
    const size_t words = bytes / 4;
    if (words == 0) return GS_OK;
    const size_t blocks = (words + 255) / 256;
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, (uint32_t*)ptr, words);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { gs_set_error((int)e, stage); return GS_E_HIP; }
    return GS_OK;
}

// shader clock under a VALU-bound load: an FMA stream on every SIMD; the first lane of every workgroup adds its
// s_memtime ticks (shader cycles) and s_memrealtime ticks (100 MHz) to out[0] / out[1]
__global__ __launch_bounds__(256) void clock_probe_kernel(unsigned long long* __restrict__ out, int iters, float seed, float* __restrict__ sink) {
    const unsigned long long t0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = seed + (float)i + (float)threadIdx.x * 1e-3f;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int i = 0; i < 8; i++) a[i] = __builtin_fmaf(a[i], 1.0001f, 0.5f);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) sum += a[i];
    if (sum == 12345.678f) sink[0] = sum;  // (keeps the chains alive; never true in practice)
    if (threadIdx.x == 0) {
        const unsigned long long t1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
        atomicAdd(&out[0], t1 - t0);
        atomicAdd(&out[1], r1 - r0);
    }
}

__global__ __launch_bounds__(64) void xcc_probe_kernel(uint32_t* __restrict__ out) {
    if (threadIdx.x == 0) out[blockIdx.x] = xcc_id();
}

// ---- what the frame path's entry points share -----------------------------------------------------------------
// What every such entry point does first, in the order each of them has always done it: the common validation of `a`;
// the null / range checks on the states (GS_E_BAD_ARG); the entry point's own argument checks (`own`: a callable that
// answers a status); then the three carves -- views of const members where the state pointer is to const -- against the
// sizes the caller passed (GS_E_WORKSPACE).  Nothing is enqueued.  (A call without a binning state: binning = (void*)0,
// D = 0.  A frame without pairs has no binning view either: null members.)
template <class Void, class VoidBin, class G, class B, class I, class Own>
static int frame_states(const GsFwdArgs* a, Void* geom, size_t geom_bytes, VoidBin* binning, size_t binning_bytes, Void* img,
                        size_t img_bytes, int64_t D, G* g, B* b, I* im, Own own) {
    int rc = validate(a);
    if (rc != GS_OK) return rc;
    if (!geom || !img || D < 0 || (D > 0 && !binning)) return GS_E_BAD_ARG;
    if ((rc = own()) != GS_OK) return rc;
    *g = geom_state(geom, a->P);
    *im = img_state(img, a->W, a->H, a->long_lists);
    *b = bin_state(D > 0 ? binning : nullptr, D);
    if (geom_bytes < g->total || img_bytes < im->total || (D > 0 && binning_bytes < b->total)) return GS_E_WORKSPACE;
    return GS_OK;
}

// QuadLists serves the forward, which writes through it, and the backward, which only reads (launch_render_backward);
// its members are not const, so a read-only image state is handed over like this
template <class T> static T* writable(T* p) { return p; }
template <class T> static T* writable(const T* p) { return const_cast<T*>(p); }
// The members of QuadLists every render sets the same way, forward or backward, first or second image (four_waves is
// the forward's; the backward does not look at it)
template <bool RO>
static QuadLists quad_lists(const ImgViewT<RO>& im, const BinView& b, int long_lists) {
    QuadLists ql;
    ql.qlist = b.qlist;
    ql.ncon_c = writable(im.ncon_c);
    ql.qcount = writable(im.qcount);
    ql.chunks = gs_tune_get(GS_TUNE_BWD_CHUNKS) ? im.bwd_chunks : 1;
    ql.four_waves = forward_small_image(im.ntiles, long_lists) ? 1 : 0;
    ql.ckpt = ql.chunks > 1 ? writable(im.ckpt) : nullptr;
    ql.ck_start = ql.chunks > 1 ? writable(im.ck_start) : nullptr;
    return ql;
}
// ... and those of the chunk-parallel forward (render_fwd.hip: render_chunk): the work list of `list` -- this image
// state's own, or for a second render the first render's -- and the hand-off words and records of `own`
template <bool RO>
static void quad_lists_chunked(QuadLists& ql, const ImgView& own, const ImgViewT<RO>& list) {
    ql.chunked = 1;
    ql.cw_hdr = list.cw_hdr;
    ql.cw_units = list.cw_units;
    ql.cw_items = list.cw_items;
    ql.cw_q = own.cw_q;
    ql.cw_flag = own.cw_flag;
    ql.cw_done = own.cw_done;
    ql.cw_rec = own.cw_rec;
}
static int sync_if_debug(const GsFwdArgs* a, const char* stage, hipStream_t s) {
    if (!a->debug) return GS_OK;
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { gs_set_error((int)e, stage); return GS_E_HIP; }
    return GS_OK;
}

extern "C" {

int gs_xcc_probe(uint32_t* xcc, int32_t n_blocks, void* stream) {
    if (!xcc || n_blocks <= 0) return GS_E_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(xcc_probe_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s, xcc);
    GS_LAUNCH_CHECK("xcc_probe", 0, s);
    return GS_OK;
}

int gs_clock_probe(uint64_t* ticks, int32_t iters, void* stream) {
    if (!ticks || iters <= 0) return GS_E_BAD_ARG;
    GS_NO_CAPTURE(stream);
    hipStream_t s = (hipStream_t)stream;
    int rc = gs_zero_async(ticks, 32, "clock_probe.zero", s);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(clock_probe_kernel, dim3(2048), dim3(256), 0, s, (unsigned long long*)ticks, iters, 1.0f, (float*)(ticks + 2));
    GS_LAUNCH_CHECK("clock_probe", 0, s);
    return GS_OK;
}

int gs_geom_bytes(int32_t P, size_t* out) {
    if (!out || P < 0) return GS_E_BAD_ARG;
    *out = geom_layout(P).total;
    return GS_OK;
}
int gs_image_bytes(int32_t W, int32_t H, size_t* out) {
    if (!out || W <= 0 || H <= 0) return GS_E_BAD_ARG;
    *out = img_layout(W, H).total;
    return GS_OK;
}
int gs_image_bytes_for(const GsFwdArgs* a, size_t* out) {
    if (!a || !out || a->W <= 0 || a->H <= 0) return GS_E_BAD_ARG;
    *out = img_layout(a->W, a->H, a->long_lists).total;
    return GS_OK;
}
int gs_binning_bytes(int64_t D, int32_t W, int32_t H, size_t* out) {
    if (!out || D < 0 || W <= 0 || H <= 0) return GS_E_BAD_ARG;
    if (D > GS_MAX_PAIRS) return GS_E_TOO_LARGE;
    *out = bin_layout(D).total;
    return GS_OK;
}
int gs_backward_scratch_bytes(int64_t D, int32_t P, int32_t W, int32_t H, size_t* out) {
    if (!out || D < 0 || P < 0 || W <= 0 || H <= 0) return GS_E_BAD_ARG;
    const ImgLayout I = img_layout(W, H);
    *out = scratch_total_bytes(D, P, I.gx * I.gy);
    return GS_OK;
}

// `poll`: a pinned host word the scan kernel writes the count into directly (gs_forward spins on it)
static int forward_phase1(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* img, size_t img_bytes, int32_t* radii,
                          int64_t* count_host_pinned, unsigned long long* poll, void* stream) {
    GeomView g;
    BinView none;
    ImgView im;
    int rc = frame_states(a, geom, geom_bytes, (void*)nullptr, 0, img, img_bytes, 0, &g, &none, &im,
                          [&]() -> int { return (a->P > 0 && !radii) ? GS_E_BAD_ARG : GS_OK; });
    if (rc != GS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (a->P == 0) {
        rc = gs_zero_async(g.count, COUNT_ZERO_BYTES, "count.zero", s);
        if (rc != GS_OK) return rc;
    } else {
        ZeroJob zt;  // the depth sort's digit totals, cleared by the preprocess kernel
        sort_totals_region(g.hist, a->P, 32, &zt.ptr, &zt.words);
        // ... and the image state's per-tile pair totals, which phase 2's counting pass adds into
        const ZeroJob zi{im.tile_tot, (int)(im.tile_zero_bytes / 4)};
        { StageScope sc_("preprocess", s);
        rc = launch_preprocess(*a, g.rec, g.depths, g.tiles, g.clamped, g.key0, g.val0, radii, g.wsum, g.wkmin, g.wkmax, zt, zi, s); }
        if (rc != GS_OK) return rc;
        // pair numbering (Gaussian-major, index order) and the pair count need nothing of the depth sort, so the count is
        // on its way to the host while the sort runs; (depth key, index) order: ties keep ascending Gaussian index (the
        // reference's tie order); the ranking ends in val0 and, with what binning needs of every Gaussian, in the rank list
        if (gs_tune_get(GS_TUNE_DEPTH_SORT)) {
            StageScope sc_("depth_sort", s);  // the numbering rides in its first launch, the rank list in its last ones
            const DepthSortState ds{g.ds_tmp, g.ds_tmp2, g.ds_cnt, g.ds_pre, g.ds_tot, g.ds_loc, g.ds_grp, g.ds_range, g.ds_nb, g.ds_blocks};
            const PairNumbering pn{g.tiles, g.wsum, g.rec, g.count, poll, g.chunk_pairs, (a->P + 255) / 256};
            const RankOut ro{g.rec, g.tiles, g.val0, g.ranklist, g.chunk_pairs};
            rc = launch_depth_sort(g.key0, g.wkmin, g.wkmax, g.nwaves, a->P, ds, pn, ro, a->debug, s);
            if (rc != GS_OK) return rc;
        } else {  // the LSD radix sort (gs_tuning "depth_sort" = 0): 4 passes, ends in (key0, val0)
            { StageScope sc_("pair_scan", s);
            rc = launch_first_pair(g.tiles, g.wsum, g.rec, g.count, poll, a->P, a->debug, s); }
            if (rc != GS_OK) return rc;
            { StageScope sc_("depth_sort", s);
            rc = launch_sort_pairs(g.key0, g.val0, g.key1, g.val1, g.hist, a->P, 32, true, a->debug, s); }
            if (rc != GS_OK) return rc;
            { StageScope sc_("rank_list", s);
            rc = launch_rank_list(g.val0, g.rec, g.tiles, g.ranklist, g.chunk_pairs, a->P, a->debug, s); }
            if (rc != GS_OK) return rc;
        }
    }
    if (count_host_pinned && (!poll || a->P == 0)) {
        hipError_t e = hipMemcpyAsync(count_host_pinned, g.count, 8, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { gs_set_error((int)e, "count.copy"); return GS_E_HIP; }
    }
    return GS_OK;
}

int gs_forward_preprocess(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* img, size_t img_bytes,
                          int32_t* radii, int64_t* count_host_pinned, void* stream) {
    GS_CAPTURE_OK_IF(stream, a && !a->debug && count_host_pinned == nullptr);
    return forward_phase1(a, geom, geom_bytes, img, img_bytes, radii, count_host_pinned, nullptr, stream);
}

// Phase 2 against a binning state carved for `cap` pairs.  The kernels read the frame's pair count from the geom state
// on the device (PairCount): the phase can be enqueued before the host knows the count; a count beyond `cap` makes every
// kernel do the work of an empty frame (nothing out of bounds) and the caller runs the phase again with a larger state.
// `totals_zeroed`: phase 1 has just run on this image state (its preprocess kernel cleared the per-tile pair totals).
static int forward_phase2(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes, void* img,
                          size_t img_bytes, int64_t cap, float* out_color, void* stream, bool totals_zeroed) {
    GeomView g;
    BinView b;
    ImgView im;
    int rc = frame_states(a, geom, geom_bytes, binning, binning_bytes, img, img_bytes, cap, &g, &b, &im, [&]() -> int {
        if (!out_color) return GS_E_BAD_ARG;
        if (a->l1_target && !a->l1_loss) return GS_E_BAD_ARG;  // the fused L1 loss needs somewhere to put its value
        return cap > GS_MAX_PAIRS ? GS_E_TOO_LARGE : GS_OK;
    });
    if (rc != GS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const PairCount pc{g.count + COUNT_PAIRS, (uint32_t)cap};
    // the marked tiles chunk-parallel (render_fwd.hip: render_chunk): the image state has the cw_* fields exactly then
    const bool chunked = forward_chunked(im.ntiles, a->long_lists);
    if (a->P > 0) {
        rc = launch_tile_lists(g.ranklist, g.chunk_pairs, g.seg_start, a->P, im.gx, im.gy,
                               TileCounts{im.seg_cnt, im.tile_tot, im.tile_zero_bytes, im.cw_xcc_mask}, im.ranges, im.order,
                               b.point_list, pc,
                               LongLists{chunked ? 2 : (forward_small_image(im.ntiles, a->long_lists) ? 1 : 0), (long long*)a->frame_stats,
                                         im.cw_hdr, im.cw_units, (uint32_t)gs_tune_get(GS_TUNE_FWDC_CH), im.cw_items, im.cw_xcc_mask,
                                         chunked ? (uint32_t)gs_tune_get(GS_TUNE_FWDC_DIV) : (uint32_t)FWD4_TOTAL_DIV},
                               totals_zeroed, a->debug, s);
        if (rc != GS_OK) return rc;
    } else {
        rc = gs_zero_async(im.ranges, (size_t)im.ntiles * 8, "ranges.zero", s);
        if (rc != GS_OK) return rc;
        StageScope sc_("ranges_order", s);
        rc = launch_tile_order(im.ranges, nullptr, 0, im.ntiles, im.order, pc, FillJob{nullptr, 0},
                               LongLists{0, nullptr, im.cw_hdr, nullptr}, a->debug, s);
        if (rc != GS_OK) return rc;
    }
    QuadLists ql = quad_lists(im, b, a->long_lists);
    if (chunked) quad_lists_chunked(ql, im, im);
    if (cap > 0) {  // the backward's row marks, set on the side by the render launch (BinLayout::marks) -- or declared unset
        // (not for a frame no backward can follow -- GsFwdArgs.forward_only: a frame rendered under no_grad)
        ql.marks = (gs_tune_get(GS_TUNE_FWD_MARKS) && !a->forward_only) ? b.marks : nullptr;
        ql.mark_quads = (size_t)cap;
        ql.marks_flag = b.marks_flag;
    }
    ql.l1_target = a->l1_target;  // the fused L1 loss rides in the render launch (+ its one-workgroup final sum)
    ql.l1_part = im.l1_part;
    ql.l1_loss = a->l1_loss;
    { StageScope sc_("render_fwd", s);
    rc = launch_render_forward(g.rec, a->P > 0 ? b.point_list : nullptr, im.ranges, im.order, a->bg, a->W, a->H, out_color,
                               im.final_T, im.n_contrib, ql, s); }
    if (rc != GS_OK) return rc;
    return sync_if_debug(a, "render_forward", s);
}

int gs_forward_render(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes,
                      void* img, size_t img_bytes, int64_t D, float* out_color, void* stream) {
    GS_CAPTURE_OK_IF(stream, a && !a->debug && a->frame_stats == nullptr);
    return forward_phase2(a, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, out_color, stream, false);
}

// Both phases in one call, WITHOUT a GPU idle stretch for the pair count.  The binning state the caller passes was
// carved for `capacity` pairs (gs_binning_bytes(capacity): the caller sizes it from the previous frame's count).
// Phase 2 is enqueued right behind phase 1, its kernels reading the count on the device; only then does the host wait
// for the count -- the scan kernel stores it straight into the caller's pinned word -- while the GPU already works on
// phase 2.  If the count turns out larger than the capacity, phase 2 has rendered an empty frame into the buffers
// (nothing out of bounds): GS_E_WORKSPACE is returned with *num_rendered set and the caller runs gs_forward_render with
// a state of the right size.  With capacity 0 (no estimate yet) only phase 1 runs and GS_E_WORKSPACE is returned.
int gs_forward(const GsFwdArgs* a, void* geom, size_t geom_bytes, void* binning, size_t binning_bytes, int64_t capacity,
               void* img, size_t img_bytes, int32_t* radii, int64_t* count_host_pinned, float* out_color,
               int64_t* num_rendered, void* stream) {
    if (!count_host_pinned || !num_rendered || capacity < 0) return GS_E_BAD_ARG;
    GS_NO_CAPTURE(stream);  // (the host waits for the pair count: gs_forward_preprocess + gs_forward_render are the capturable form)
    volatile int64_t* word = count_host_pinned;
    const int64_t pending = -1;
    static std::atomic<bool> poll_works{true};  // cleared for the process if a device write to the word is ever not seen
    const bool poll = a && a->P > 0 && poll_works.load(std::memory_order_relaxed);
    if (poll) *word = pending;
    int rc = forward_phase1(a, geom, geom_bytes, img, img_bytes, radii, count_host_pinned,
                            poll ? (unsigned long long*)count_host_pinned : nullptr, stream);
    if (rc != GS_OK) return rc;
    const bool speculate = capacity > 0 && binning && binning_bytes >= bin_layout(capacity).total && capacity <= GS_MAX_PAIRS;
    if (speculate) {
        rc = forward_phase2(a, geom, geom_bytes, binning, binning_bytes, img, img_bytes, capacity, out_color, stream, true);
        if (rc != GS_OK) return rc;
    }
    bool have = false;
    if (poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (long spin = 0;; spin++) {
            if (*word != pending) { have = true; break; }
            if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
        }
    }
    if (!have) {
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) { gs_set_error((int)e, "count.sync"); return GS_E_HIP; }
        if (poll && *word == pending) {
            // the host word is not device-visible memory on this system: read the count from the geom state and
            // use the copy + synchronise form from now on
            poll_works.store(false, std::memory_order_relaxed);
            int64_t c = 0;
            e = hipMemcpy(&c, geom_state(geom, a->P).count + COUNT_PAIRS, 8, hipMemcpyDeviceToHost);
            if (e != hipSuccess) { gs_set_error((int)e, "count.copy"); return GS_E_HIP; }
            *word = c;
        }
    }
    const int64_t D = *word;
    *num_rendered = D;
    if (D > (int64_t)GS_MAX_PAIRS) return GS_E_TOO_LARGE;
    if (!speculate || D > capacity) return GS_E_WORKSPACE;  // caller sizes the state for D, then gs_forward_render
    return GS_OK;
}

int gs_forward_shared(const GsFwdArgs* a, const void* geom_src, const void* img_src, void* geom, size_t geom_bytes,
                      void* binning, size_t binning_bytes, void* img, size_t img_bytes, int64_t D, float* out_color,
                      void* stream) {
    GS_CAPTURE_OK_IF(stream, a && !a->debug && a->P > 0);
    GeomView g;  // THIS render's states, written ...
    BinView b;
    ImgView im;
    int rc = frame_states(a, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, &g, &b, &im,
                          [&]() -> int { return (!geom_src || !img_src || !out_color) ? GS_E_BAD_ARG : GS_OK; });
    if (rc != GS_OK) return rc;
    // ... and the FIRST render's, read (the caller passes the SAME long_lists as to the first render, so that both image
    // states have the same layout)
    const GeomViewRO first_g = geom_state(geom_src, a->P);
    const ImgViewRO first_im = img_state(img_src, a->W, a->H, a->long_lists);
    hipStream_t s = (hipStream_t)stream;
    const bool chunked = forward_chunked(im.ntiles, a->long_lists);  // (im and first_im have the cw_* fields exactly then)
    QuadLists ql = quad_lists(im, b, a->long_lists);  // (qlist: read, not rewritten -- the recorded quadrant lists are what is walked)
    unsigned long long* not_ones = nullptr;
    if (a->P > 0) {
        StageScope sc_("recolor", s);
        // (the first render's geom state carries the "not all ones" word, zero since that render)
        if (gs_tune_get(GS_TUNE_ONES_FAST) && gs_tune_get(GS_TUNE_SHARED_QLIST) && a->colors_precomp && D > 0)
            not_ones = not_ones_word(first_g);
        // ... and, when the colours may turn out to be all ones, the launch's other workgroups write the image that is
        // right in that case (1 - T of the first render, with its records): the render launch below then leaves at once
        const SecondOnes so{first_im.final_T, first_im.n_contrib, first_im.ncon_c, first_im.qcount, first_im.ckpt, first_im.ck_start,
                            out_color, im.final_T, im.n_contrib, im.ncon_c, im.qcount, ql.ckpt, ql.ck_start, a->bg, a->W, a->H,
                            im.gx, im.ntiles, ql.chunks};
        rc = launch_recolor(*a, first_g.rec, first_g.tiles, g.rec, g.tiles, g.clamped, not_ones,
                            CopyJob{first_im.ranges, im.ranges, im.ntiles * 2}, CopyJob{first_im.order, im.order, im.ntiles},
                            ZeroJob{im.cw_flag, im.cw_clear_words}, not_ones ? &so : nullptr, s);
        if (rc != GS_OK) return rc;
    } else {
        // (no Gaussians: no recolouring launch to ride in) the new image state's own copy of the tile ranges and launch order
        hipError_t e = hipMemcpyAsync(im.ranges, first_im.ranges, (size_t)im.ntiles * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(im.order, first_im.order, (size_t)im.ntiles * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { gs_set_error((int)e, "shared.copy"); return GS_E_HIP; }
    }
    if (gs_tune_get(GS_TUNE_SHARED_QLIST)) {
        ql.src_qcount = first_im.qcount;        // (the fields before the checkpoints sit at the same offsets
        ql.src_n_contrib = first_im.n_contrib;  //  whatever long_lists the first render was given)
        ql.not_ones = not_ones;
    }
    if (chunked && a->P > 0) {
        // the first render's work list (the copied launch order carries its marks); this state's own hand-off words
        // (cleared by the recolouring launch) and records; walking the recorded lists also the first render's records
        quad_lists_chunked(ql, im, first_im);
        if (ql.src_qcount) {
            ql.src_cw_flag = first_im.cw_flag;
            ql.src_cw_rec = first_im.cw_rec;
            ql.src_final_T = first_im.final_T;
        }
    }
    ql.all_ones = im.all_ones;  // (set by the render launch: 1 iff it left the speculative image alone)
    { StageScope sc_("render_fwd", s);
    rc = launch_render_forward(g.rec, b.point_list, im.ranges, im.order, a->bg, a->W, a->H, out_color, im.final_T, im.n_contrib, ql, s); }
    if (rc != GS_OK) return rc;
    return sync_if_debug(a, "render_forward", s);
}

int gs_opacity_image(const GsFwdArgs* a, const void* img, size_t img_bytes, float* opacity, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    int rc = validate(a);
    if (rc != GS_OK) return rc;
    if (!img || !opacity) return GS_E_BAD_ARG;
    const ImgViewRO im = img_state(img, a->W, a->H, a->long_lists);
    if (img_bytes < im.total) return GS_E_WORKSPACE;
    return launch_opacity_image(im.final_T, a->bg, a->W, a->H, opacity, (hipStream_t)stream);
}

static int backward_impl(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes, void* binning,
                         size_t binning_bytes, const void* img, size_t img_bytes, int64_t D, const float* out_color,
                         const float* dL_dpix, const float* dL_dopacity_img, void* scratch, size_t scratch_bytes,
                         const GsGrads* gr, void* stream, const GsSecondImage* second = nullptr) {
    GS_CAPTURE_OK_IF(stream, a && !a->debug);
    GeomViewRO g;
    BinView b;
    ImgViewRO im;
    int rc = frame_states(a, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, &g, &b, &im, [&]() -> int {
        if (!out_color || (!dL_dpix && !a->l1_target) || !gr || (a->P > 0 && !scratch)) return GS_E_BAD_ARG;
        if (a->P > 0 && (!radii || !gr->dL_dmeans3D || !gr->dL_dmeans2D || !gr->dL_dcolors || !gr->dL_dopacity || !gr->dL_dcov3D))
            return GS_E_BAD_ARG;
        if (a->P > 0 && a->shs && !gr->dL_dsh) return GS_E_BAD_ARG;
        if (a->P > 0 && a->scales && (!gr->dL_dscales || !gr->dL_drotations)) return GS_E_BAD_ARG;
        if (gr->dL_drotations && ((uintptr_t)gr->dL_drotations & 15u)) return GS_E_BAD_ARG;  // written as float4
        return GS_OK;
    });
    if (rc != GS_OK) return rc;
    if (a->P > 0 && scratch_bytes < scratch_total_bytes(D, a->P, im.ntiles)) return GS_E_WORKSPACE;
    if (a->P == 0) return GS_OK;
    hipStream_t s = (hipStream_t)stream;
    float* const sums = (float*)((char*)scratch + scratch_rows_bytes(D));
    if (D > 0) {
        const QuadLists ql = quad_lists(im, b, a->long_lists);
        SecondImage si{nullptr, nullptr, nullptr, nullptr, nullptr};
        if (second) {
            // the second render's own image state: its checkpoints (same chunk boundaries: same geometry, same rule)
            const ImgViewRO im2 = img_state(second->img, a->W, a->H, second->long_lists);
            if (second->img_bytes < im2.total || im2.bwd_chunks != im.bwd_chunks) return GS_E_BAD_ARG;
            si = SecondImage{second->colors, second->out_color, second->dL_dpix, ql.chunks > 1 ? im2.ckpt : nullptr, im2.all_ones};
        }
        // the row marks: in the binning state, where the forward has set every word to ROW_UNWRITTEN beside its render
        // kernel; if a backward has run on this state since (marks_flag), the tile-order launch's other workgroups do it
        uint32_t* const q8 = reinterpret_cast<uint32_t*>(b.marks);
        uint32_t* const own_order = (uint32_t*)((char*)sums + scratch_sums_bytes(a->P));
        const bool order_here = gs_tune_get(GS_TUNE_BWD_ORDER) != 0;
        { StageScope sc_("tile_order", s);
        rc = launch_tile_order(im.ranges, ql.qcount, order_here ? 1 : -1, im.ntiles, own_order, PairCount{nullptr, 0},
                               FillJob{b.marks, (size_t)D, gs_tune_get(GS_TUNE_NT_STORES) & 1, b.marks_flag},
                               LongLists{0, nullptr}, a->debug, s); }
        if (rc != GS_OK) return rc;
        { StageScope sc_("render_bwd", s);
        rc = launch_render_backward(g.rec, im.ranges, order_here ? own_order : im.order, a->W, a->H, ql, out_color, dL_dpix,
                                    dL_dopacity_img, im.final_T, a->bg, (float*)scratch, q8, second ? &si : nullptr,
                                    L1Grad{a->l1_target, a->l1_grad}, s); }
        if (rc != GS_OK) return rc;
        rc = sync_if_debug(a, "render_backward", s);
        if (rc != GS_OK) return rc;
    }
    StageScope sc_("gaussian_bwd", s);
    return launch_gaussian_backward(*a, radii, g.rec, g.tiles, g.clamped, reinterpret_cast<const uint32_t*>(b.marks),
                                    (const float*)scratch, sums, b.marks_flag, *gr, s);
}

int gs_backward(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes, void* binning,
                size_t binning_bytes, const void* img, size_t img_bytes, int64_t D, const float* out_color,
                const float* dL_dpix, void* scratch, size_t scratch_bytes, const GsGrads* gr, void* stream) {
    return backward_impl(a, radii, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, out_color, dL_dpix, nullptr,
                         scratch, scratch_bytes, gr, stream);
}

int gs_backward_with_opacity(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes,
                             void* binning, size_t binning_bytes, const void* img, size_t img_bytes, int64_t D,
                             const float* out_color, const float* dL_dpix, const float* dL_dopacity_img, void* scratch,
                             size_t scratch_bytes, const GsGrads* gr, void* stream) {
    if (!dL_dopacity_img) return GS_E_BAD_ARG;
    return backward_impl(a, radii, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, out_color, dL_dpix,
                         dL_dopacity_img, scratch, scratch_bytes, gr, stream);
}

int gs_backward_with_second(const GsFwdArgs* a, const int32_t* radii, const void* geom, size_t geom_bytes,
                            void* binning, size_t binning_bytes, const void* img, size_t img_bytes, int64_t D,
                            const float* out_color, const float* dL_dpix, const GsSecondImage* second, void* scratch,
                            size_t scratch_bytes, const GsGrads* grads, void* stream) {
    if (!second || !second->colors || !second->out_color || !second->dL_dpix || !second->img) return GS_E_BAD_ARG;
    return backward_impl(a, radii, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, out_color, dL_dpix, nullptr,
                         scratch, scratch_bytes, grads, stream, second);
}

int gs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    uint8_t* present, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    (void)projmatrix;
    if (P < 0 || !viewmatrix || (P > 0 && (!means3D || !present))) return GS_E_BAD_ARG;
    if (P == 0) return GS_OK;
    return launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
}

int knn_workspace_bytes(int32_t P, size_t* out) {
    if (!out || P < 0) return GS_E_BAD_ARG;
    *out = knn_ws_bytes(P);
    return GS_OK;
}
int knn_dist2(int32_t P, const float* points, float* mean_d2, void* workspace, size_t workspace_bytes, void* stream) {
    GS_NO_CAPTURE(stream);  // (the sorts clear their tables with memset nodes: untested under replay)
    if (P < 0 || (P > 0 && (!points || !mean_d2 || !workspace))) return GS_E_BAD_ARG;
    if (P == 0) return GS_OK;
    return launch_knn(P, points, mean_d2, workspace, workspace_bytes, (hipStream_t)stream);
}

int gs_build_covariance(int32_t N, const float* scaling, float scaling_modifier, const float* rotation, int32_t rotation_is_matrix,
                        float* cov6, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (N > 0 && (!scaling || !rotation || !cov6))) return GS_E_BAD_ARG;
    if (!rotation_is_matrix && ((uintptr_t)rotation & 15u)) return GS_E_BAD_ARG;  // quaternions are read as float4
    if (N == 0) return GS_OK;
    return launch_build_cov(N, scaling, scaling_modifier, rotation, rotation_is_matrix ? 1 : 0, cov6, (hipStream_t)stream);
}
int gs_build_covariance_backward(int32_t N, const float* scaling, float scaling_modifier, const float* rotation,
                                 int32_t rotation_is_matrix, const float* dL_dcov6, float* dL_dscaling, float* dL_drotation,
                                 void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (N > 0 && (!scaling || !rotation || !dL_dcov6 || !dL_dscaling || !dL_drotation))) return GS_E_BAD_ARG;
    if (!rotation_is_matrix && (((uintptr_t)rotation | (uintptr_t)dL_drotation) & 15u)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    return launch_build_cov_bwd(N, scaling, scaling_modifier, rotation, rotation_is_matrix ? 1 : 0, dL_dcov6, dL_dscaling,
                                dL_drotation, (hipStream_t)stream);
}
int gs_sh2rgb(int32_t N, int32_t sh_degree, int32_t M, const float* shs, const float* xyz, const float* campos,
              const float* fwd_rotation, const float* view_noise_host, float* colors, uint8_t* clamped, void* stream) {
    GS_CAPTURE_OK_IF(stream, view_noise_host == nullptr);  // (a host matrix would be baked into the graph)
    if (N < 0 || sh_degree < 0 || sh_degree > 3 || M < (sh_degree + 1) * (sh_degree + 1) || M > 16) return GS_E_BAD_ARG;
    if (N > 0 && (!shs || !xyz || !campos || !colors || !clamped)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    return launch_sh2rgb(N, sh_degree, M, shs, xyz, campos, fwd_rotation, view_noise_host, colors, clamped, (hipStream_t)stream);
}
int gs_sh2rgb_backward(int32_t N, int32_t sh_degree, int32_t M, const float* shs, const float* xyz, const float* campos,
                       const float* fwd_rotation, const float* view_noise_host, const uint8_t* clamped,
                       const float* dL_dcolors, float* dL_dshs, float* dL_dxyz, void* stream) {
    GS_CAPTURE_OK_IF(stream, view_noise_host == nullptr);
    if (N < 0 || sh_degree < 0 || sh_degree > 3 || M < (sh_degree + 1) * (sh_degree + 1) || M > 16) return GS_E_BAD_ARG;
    if (N > 0 && (!shs || !xyz || !campos || !clamped || !dL_dcolors || !dL_dshs || !dL_dxyz)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    return launch_sh2rgb_bwd(N, sh_degree, M, shs, xyz, campos, fwd_rotation, view_noise_host, clamped, dL_dcolors, dL_dshs,
                             dL_dxyz, (hipStream_t)stream);
}

int gs_l1_loss_workspace_bytes(int64_t n, size_t* out) {
    if (!out || n < 0) return GS_E_BAD_ARG;
    *out = l1_ws_bytes(n);
    return GS_OK;
}
int gs_l1_loss(int64_t n, const float* x, const float* y, float* loss, float* dL_dx, void* workspace, size_t workspace_bytes,
               void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n <= 0 || !x || !y || !loss || !dL_dx || !workspace) return GS_E_BAD_ARG;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)dL_dx) & 15u) return GS_E_BAD_ARG;  // float4 accesses
    if (workspace_bytes < l1_ws_bytes(n)) return GS_E_WORKSPACE;
    return launch_l1_loss(x, y, n, loss, dL_dx, (float*)workspace, (hipStream_t)stream);
}

int gs_bce_loss(int64_t n, const float* x, const float* y, float* loss, float* dL_dx, void* workspace, size_t workspace_bytes,
                void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n <= 0 || !x || !y || !loss || !dL_dx || !workspace) return GS_E_BAD_ARG;
    if (workspace_bytes < l1_ws_bytes(n)) return GS_E_WORKSPACE;
    return launch_bce_loss(x, y, n, loss, dL_dx, (float*)workspace, (hipStream_t)stream);
}

int gs_ssim_workspace_bytes(int32_t C, int32_t H, int32_t W, size_t* out) {
    if (!out || C <= 0 || H <= 0 || W <= 0) return GS_E_BAD_ARG;
    *out = ssim_ws_bytes(C, H, W);
    return GS_OK;
}
int gs_ssim_forward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float* ssim_out, float* dm_dmu1,
                    float* dm_dsigma1_sq, float* dm_dsigma12, void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !ssim_out || !workspace) return GS_E_BAD_ARG;
    if ((dm_dmu1 != nullptr) != (dm_dsigma1_sq != nullptr) || (dm_dmu1 != nullptr) != (dm_dsigma12 != nullptr)) return GS_E_BAD_ARG;
    if (workspace_bytes < ssim_ws_bytes(C, H, W)) return GS_E_WORKSPACE;
    return launch_ssim_forward(C, H, W, img1, img2, ssim_out, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, (float*)workspace,
                               (hipStream_t)stream);
}
int gs_ssim_backward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* dm_dmu1,
                     const float* dm_dsigma1_sq, const float* dm_dsigma12, const float* dL_dssim, float* dL_dimg1,
                     void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dssim || !dL_dimg1)
        return GS_E_BAD_ARG;
    return launch_ssim_backward(C, H, W, img1, img2, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dssim, dL_dimg1,
                                (hipStream_t)stream);
}

int gs_densify_stats(int32_t N, const int32_t* radii, const float* viewspace_grad, float* max_radii2D,
                     float* xyz_gradient_accum, float* denom, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (N > 0 && (!radii || !viewspace_grad || !max_radii2D || !xyz_gradient_accum || !denom))) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    return launch_densify_stats(N, radii, viewspace_grad, max_radii2D, xyz_gradient_accum, denom, (hipStream_t)stream);
}
int gs_adam_step(int32_t n_tensors, const GsAdamTensor* tensors, double beta1, double beta2, double eps, int64_t step,
                 void* stream) {
    GS_NO_CAPTURE(stream);  // (the step number is a host scalar: a replay would repeat the captured step's bias correction)
    if (n_tensors < 0 || n_tensors > GS_ADAM_MAX_TENSORS || (n_tensors > 0 && !tensors) || step < 1) return GS_E_BAD_ARG;
    for (int k = 0; k < n_tensors; k++) {
        const GsAdamTensor& t = tensors[k];
        if (t.n < 0 || (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))) return GS_E_BAD_ARG;
    }
    if (n_tensors == 0) return GS_OK;
    return launch_adam(n_tensors, tensors, beta1, beta2, eps, step, (hipStream_t)stream);
}

// ---- the converter's optimizer step (optim.hip): every argument check comes before the first HIP call
#define GS_OPTIM_MAX_N ((int64_t)1 << 41)  // chunks of 2048 elements are counted in an int
static int grad_tensors_ok(int32_t n_tensors, const GsGradTensor* tensors) {
    if (n_tensors < 0 || n_tensors > GS_OPTIM_MAX_TENSORS || (n_tensors > 0 && !tensors)) return GS_E_BAD_ARG;
    for (int k = 0; k < n_tensors; k++)
        if (tensors[k].n < 0 || (tensors[k].n > 0 && !tensors[k].grad)) return GS_E_BAD_ARG;
    for (int k = 0; k < n_tensors; k++)
        if (tensors[k].n >= GS_OPTIM_MAX_N) return GS_E_TOO_LARGE;
    return GS_OK;
}
int gs_grad_norm_workspace_bytes(int32_t n_tensors, const GsGradTensor* tensors, size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    if (const int rc = grad_tensors_ok(n_tensors, tensors)) return rc;
    *out = grad_norm_workspace_bytes(n_tensors, tensors);
    return GS_OK;
}
int gs_grad_norm(int32_t n_tensors, const GsGradTensor* tensors, float max_norm, float* out, void* workspace,
                 size_t workspace_bytes, void* stream) {
    if (!out || !workspace || !(max_norm >= 0.f)) return GS_E_BAD_ARG;
    if (const int rc = grad_tensors_ok(n_tensors, tensors)) return rc;
    if (workspace_bytes < grad_norm_workspace_bytes(n_tensors, tensors)) return GS_E_WORKSPACE;
    if (n_tensors == 0) return GS_OK;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_grad_norm(n_tensors, tensors, max_norm, out, (float*)workspace, (hipStream_t)stream);
}
int gs_grad_scale(int32_t n_tensors, const GsGradTensor* tensors, const float* clip_coef, void* stream) {
    if (!clip_coef) return GS_E_BAD_ARG;
    if (const int rc = grad_tensors_ok(n_tensors, tensors)) return rc;
    if (n_tensors == 0) return GS_OK;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_grad_scale(n_tensors, tensors, clip_coef, (hipStream_t)stream);
}
int gs_adam_step_ex(int32_t n_tensors, const GsAdamTensorEx* tensors, double beta1, double beta2, double eps, int64_t step,
                    const float* clip_coef, void* stream) {
    if (n_tensors < 0 || n_tensors > GS_OPTIM_MAX_TENSORS || (n_tensors > 0 && !tensors)) return GS_E_BAD_ARG;
    bool host_step = false;
    for (int k = 0; k < n_tensors; k++) {
        const GsAdamTensorEx& t = tensors[k];
        if (t.n < 0 || (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))) return GS_E_BAD_ARG;
        if (!t.step) host_step = true;
    }
    if (host_step && step < 1) return GS_E_BAD_ARG;
    for (int k = 0; k < n_tensors; k++)
        if (tensors[k].n >= GS_OPTIM_MAX_N) return GS_E_TOO_LARGE;
    if (n_tensors == 0) return GS_OK;
    // (a host step number under capture: a replay would repeat the captured step's bias correction)
    GS_CAPTURE_OK_IF(stream, !host_step);
    return launch_adam_ex(n_tensors, tensors, beta1, beta2, eps, host_step ? step : 0, clip_coef, (hipStream_t)stream);
}

// ---- densification cycle (densify.hip).  N < 2^30: the map packs a source index and a two-bit slot into 32 bits, and
// N' <= 2 N stays an int32
#define GS_DENSIFY_MAX_N (1 << 30)
int gs_densify_workspace_bytes(int32_t N, size_t* out) {
    if (!out || N < 0 || N >= GS_DENSIFY_MAX_N) return GS_E_BAD_ARG;
    *out = densify_workspace_bytes(N);
    return GS_OK;
}
int gs_densify_plan(const GsDensifyPlan* p, void* workspace, size_t workspace_bytes, int32_t* count_host_pinned,
                    void* stream) {
    GS_CAPTURE_OK_IF(stream, count_host_pinned == nullptr);
    if (!p || !workspace || p->N < 0 || p->N >= GS_DENSIFY_MAX_N) return GS_E_BAD_ARG;
    if (p->N > 0 && !p->prune_mask && (!p->scaling || !p->opacity || !p->grad_accum || !p->denom)) return GS_E_BAD_ARG;
    if (workspace_bytes < densify_workspace_bytes(p->N)) return GS_E_WORKSPACE;
    return launch_densify_plan(*p, workspace, count_host_pinned, (hipStream_t)stream);
}
int gs_densify_apply(int32_t N, int32_t N_new, const void* workspace, size_t workspace_bytes, int32_t n_tensors,
                     const GsDensifyTensor* tensors, const float* scaling, const float* rotation, const float* noise,
                     void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || N >= GS_DENSIFY_MAX_N || N_new < 0 || N_new > 2 * N || !workspace || n_tensors < 0 ||
        n_tensors > GS_DENSIFY_MAX_TENSORS || (n_tensors > 0 && !tensors))
        return GS_E_BAD_ARG;
    if (workspace_bytes < densify_workspace_bytes(N)) return GS_E_WORKSPACE;
    for (int k = 0; k < n_tensors; k++) {
        const GsDensifyTensor& t = tensors[k];
        if (t.width <= 0 || t.kind < GS_DENSIFY_COPY || t.kind > GS_DENSIFY_CHILD_SCALING) return GS_E_BAD_ARG;
        if (N_new > 0 && (!t.dst || (t.kind != GS_DENSIFY_ZERO && !t.src))) return GS_E_BAD_ARG;
        if ((t.kind == GS_DENSIFY_CHILD_POSITION || t.kind == GS_DENSIFY_CHILD_SCALING) && t.width != 3) return GS_E_BAD_ARG;
        if (t.kind == GS_DENSIFY_CHILD_POSITION && N_new > 0 && (!scaling || !rotation || !noise)) return GS_E_BAD_ARG;
    }
    if (N_new == 0 || n_tensors == 0) return GS_OK;
    return launch_densify_apply(N, N_new, workspace, n_tensors, tensors, scaling, rotation, noise, (hipStream_t)stream);
}
int gs_reset_opacity(int32_t N, const float* opacity_in, float* opacity_out, float* exp_avg, float* exp_avg_sq,
                     void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (N > 0 && (!opacity_in || !opacity_out))) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    return launch_reset_opacity(N, opacity_in, opacity_out, exp_avg, exp_avg_sq, (hipStream_t)stream);
}

// ---- AIAP regularisers (aiap.hip).  M = N (K - 1) pairs stay below 2^31 (the sort and the adjacency index 32-bit words)
static bool aiap_shape_ok(int32_t N, int32_t K, int32_t n_sets) {
    return N >= 1 && K >= 2 && K <= 8 && (n_sets == 1 || n_sets == 2) && (int64_t)N * (K - 1) < ((int64_t)1 << 31);
}
static bool aiap_sets_ok(int32_t n_sets, const GsAiapSet* sets, bool forward) {
    if (!sets) return false;
    for (int k = 0; k < n_sets; k++) {
        const GsAiapSet& s = sets[k];
        if ((s.D != 3 && s.D != 6) || !s.xc || !s.xd || (forward && !s.loss)) return false;
    }
    return true;
}
int gs_aiap_workspace_bytes(int32_t N, int32_t K, int32_t n_sets, size_t* out) {
    if (!out || !aiap_shape_ok(N, K, n_sets)) return GS_E_BAD_ARG;
    *out = aiap_workspace_bytes(N, K);
    return GS_OK;
}
int gs_aiap_forward(int32_t N, int32_t K, const int64_t* idx, int32_t n_sets, const GsAiapSet* sets, void* workspace,
                    size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!aiap_shape_ok(N, K, n_sets) || !idx || !workspace || !aiap_sets_ok(n_sets, sets, true)) return GS_E_BAD_ARG;
    if (workspace_bytes < aiap_workspace_bytes(N, K)) return GS_E_WORKSPACE;
    return launch_aiap_forward(N, K, (const long long*)idx, n_sets, sets, workspace, (hipStream_t)stream);
}
int gs_aiap_backward(int32_t N, int32_t K, const int64_t* idx, int32_t n_sets, const GsAiapSet* sets,
                     const void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!aiap_shape_ok(N, K, n_sets) || !idx || !workspace || !aiap_sets_ok(n_sets, sets, false)) return GS_E_BAD_ARG;
    if (workspace_bytes < aiap_workspace_bytes(N, K)) return GS_E_WORKSPACE;
    return launch_aiap_backward(N, K, (const long long*)idx, n_sets, sets, workspace, (hipStream_t)stream);
}

// ---- hash-grid encoding (hashgrid.hip)
static bool hg_aligned(const void* p, int F) { return p == nullptr || ((uintptr_t)p % (uintptr_t)(4 * (F < 4 ? F : 4))) == 0; }
int gs_hashgrid_levels(const GsHashGrid* grid, int32_t* offsets, float* scales, int32_t* resolutions, int32_t* n_params) {
    if (!grid) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    for (int l = 0; l <= t.L; l++) {
        if (offsets) offsets[l] = (int32_t)t.off[l];
        if (l == t.L) break;
        if (scales) scales[l] = t.scale[l];
        if (resolutions) resolutions[l] = (int32_t)t.res[l];
    }
    if (n_params) *n_params = (int32_t)(t.off[t.L] * (uint32_t)t.F);
    return GS_OK;
}
// the sort numbers the 8 L N (point, level, corner) pairs with 32-bit words
static bool hg_pairs_fit(const HgTable& t, int32_t N) { return (int64_t)8 * t.L * N < ((int64_t)1 << 31); }
int gs_hashgrid_workspace_bytes(const GsHashGrid* grid, int32_t N, size_t* out) {
    if (!grid || !out || N < 0) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    if (!hg_pairs_fit(t, N)) return GS_E_TOO_LARGE;
    *out = hashgrid_workspace_bytes(t, N);
    return GS_OK;
}
int gs_hashgrid_forward(const GsHashGrid* grid, int32_t N, const float* x, const float* params, float* out, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!grid || N < 0) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    if ((int64_t)N * t.L >= ((int64_t)1 << 31)) return GS_E_TOO_LARGE;
    if (N == 0 || !out) return GS_OK;
    if (!x || !params || !hg_aligned(params, t.F) || !hg_aligned(out, t.F) || !hg_aligned(x, 1)) return GS_E_BAD_ARG;
    return launch_hashgrid_forward(t, N, x, params, out, (hipStream_t)stream);
}
int gs_hashgrid_backward(const GsHashGrid* grid, int32_t N, const float* x, const float* params, const float* dL_dout,
                         float* dL_dx, float* dL_dparams, void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (!grid || N < 0) return GS_E_BAD_ARG;
    HgTable t;
    const int rc = hashgrid_table(grid, &t);
    if (rc != GS_OK) return rc;
    if (dL_dparams && !hg_pairs_fit(t, N)) return GS_E_TOO_LARGE;
    if (!dL_dparams && (N == 0 || !dL_dx)) return GS_OK;
    if (N > 0 && (!x || !dL_dout || (dL_dx && !params))) return GS_E_BAD_ARG;
    if (!hg_aligned(params, t.F) || !hg_aligned(dL_dout, t.F) || !hg_aligned(dL_dparams, t.F) || !hg_aligned(x, 1) ||
        !hg_aligned(dL_dx, 1))
        return GS_E_BAD_ARG;
    if (dL_dparams) {
        if (!workspace) return GS_E_BAD_ARG;
        if (workspace_bytes < hashgrid_workspace_bytes(t, N)) return GS_E_WORKSPACE;
    }
    return launch_hashgrid_backward(t, N, x, params, dL_dout, N > 0 ? dL_dx : nullptr, dL_dparams, workspace,
                                    (hipStream_t)stream);
}

// ---- linear blend skinning (skinning.hip)
static bool skin_a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static bool skin_a4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
static bool skin_kind_ok(int32_t kind) { return kind == GS_SKIN_HIERARCHICAL || kind == GS_SKIN_SOFTMAX || kind == GS_SKIN_WEIGHTS; }
int gs_skin_weights_forward(int32_t N, int32_t kind, const float* logits, float* weights, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (kind != GS_SKIN_HIERARCHICAL && kind != GS_SKIN_SOFTMAX)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!logits || !weights || !skin_a16(logits) || !skin_a16(weights)) return GS_E_BAD_ARG;
    return launch_skin_weights_forward(N, kind, logits, weights, (hipStream_t)stream);
}
int gs_skin_weights_backward(int32_t N, int32_t kind, const float* logits, const float* dL_dweights, float* dL_dlogits,
                             void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || (kind != GS_SKIN_HIERARCHICAL && kind != GS_SKIN_SOFTMAX)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!logits || !dL_dweights || !dL_dlogits || !skin_a16(logits) || !skin_a16(dL_dweights) || !skin_a16(dL_dlogits))
        return GS_E_BAD_ARG;
    return launch_skin_weights_backward(N, kind, logits, dL_dweights, dL_dlogits, (hipStream_t)stream);
}
int gs_skinning_workspace_bytes(int32_t N, size_t* out) {
    if (!out || N < 0) return GS_E_BAD_ARG;
    *out = skinning_workspace_bytes(N);
    return GS_OK;
}
int gs_skinning_forward(int32_t N, int32_t kind, const float* w, const float* tfs, const float* xyz, const float* rotation,
                        float* xyz_out, float* rotation_out, float* T_fwd, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || !skin_kind_ok(kind)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!w || !tfs || !xyz || !rotation || !xyz_out || !rotation_out || !T_fwd) return GS_E_BAD_ARG;
    if (!skin_a16(w) || !skin_a16(tfs) || !skin_a16(rotation) || !skin_a16(xyz_out) || !skin_a16(rotation_out) ||
        !skin_a16(T_fwd) || !skin_a4(xyz))
        return GS_E_BAD_ARG;
    return launch_skinning_forward(N, kind, w, tfs, xyz, rotation, xyz_out, rotation_out, T_fwd, (hipStream_t)stream);
}
int gs_skinning_backward(int32_t N, int32_t kind, const float* w, const float* tfs, const float* xyz, const float* rotation,
                         const float* dL_dxyz_out, const float* dL_drotation_out, float* dL_dw, float* dL_dtfs,
                         float* dL_dxyz, float* dL_drotation, void* workspace, size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (N < 0 || !skin_kind_ok(kind)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!w || !tfs || !xyz || !rotation) return GS_E_BAD_ARG;
    if (!skin_a16(w) || !skin_a16(tfs) || !skin_a16(rotation) || !skin_a4(xyz) || !skin_a4(dL_dxyz_out) ||
        !skin_a4(dL_drotation_out) || !skin_a16(dL_dw) || !skin_a4(dL_dtfs) || !skin_a4(dL_dxyz) || !skin_a16(dL_drotation))
        return GS_E_BAD_ARG;
    if (dL_dtfs) {
        if (!workspace || !skin_a16(workspace)) return GS_E_BAD_ARG;
        if (workspace_bytes < skinning_workspace_bytes(N)) return GS_E_WORKSPACE;
    }
    if (!dL_dw && !dL_dtfs && !dL_dxyz && !dL_drotation) return GS_OK;
    return launch_skinning_backward(N, kind, w, tfs, xyz, rotation, dL_dxyz_out, dL_drotation_out, dL_dw, dL_dtfs, dL_dxyz,
                                    dL_drotation, workspace, (hipStream_t)stream);
}

// ---- the skinning regulariser (skinloss.hip)
static bool skin_loss_kind_ok(int32_t kind) { return kind == GS_SKIN_HIERARCHICAL || kind == GS_SKIN_SOFTMAX; }
int gs_mesh_sample(int32_t n, int32_t V, int32_t F, const float* verts, const int32_t* faces, const float* cdf,
                   const float* vweights, const float* aabb_min, const float* aabb_inv_extent, const float* draws,
                   float* points_norm, float* target, int32_t* face, float* bary, float* points, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n < 0 || V < 1 || F < 1) return GS_E_BAD_ARG;
    if (!verts || !faces || !cdf || !vweights || !aabb_min || !aabb_inv_extent) return GS_E_BAD_ARG;
    if (!skin_a4(verts) || !skin_a4(faces) || !skin_a4(cdf) || !skin_a16(vweights) || !skin_a4(aabb_min) ||
        !skin_a4(aabb_inv_extent))
        return GS_E_BAD_ARG;
    if (n == 0) return GS_OK;
    if (!draws || !points_norm || !target) return GS_E_BAD_ARG;
    if (!skin_a4(draws) || !skin_a16(points_norm) || !skin_a16(target) || !skin_a4(face) || !skin_a16(bary) || !skin_a16(points))
        return GS_E_BAD_ARG;
    return launch_mesh_sample(n, V, F, verts, faces, cdf, vweights, aabb_min, aabb_inv_extent, draws, points_norm, target, face,
                              bary, points, (hipStream_t)stream);
}
int gs_skin_loss_workspace_bytes(int32_t n, size_t* out) {
    if (!out || n < 0) return GS_E_BAD_ARG;
    *out = skin_loss_workspace_bytes(n);
    return GS_OK;
}
int gs_skin_loss_forward(int32_t n, int32_t kind, const float* logits, const float* target, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n < 0 || !skin_loss_kind_ok(kind)) return GS_E_BAD_ARG;
    if (n == 0) return GS_OK;
    if (!logits || !target || !loss || !workspace) return GS_E_BAD_ARG;
    if (!skin_a16(logits) || !skin_a16(target) || !skin_a4(loss) || !skin_a16(workspace)) return GS_E_BAD_ARG;
    if (workspace_bytes < skin_loss_workspace_bytes(n)) return GS_E_WORKSPACE;
    return launch_skin_loss_forward(n, kind, logits, target, loss, workspace, (hipStream_t)stream);
}
int gs_skin_loss_backward(int32_t n, int32_t kind, const float* logits, const float* target, const float* dL_dloss,
                          float* dL_dlogits, void* stream) {
    GS_CAPTURE_OK_IF(stream, true);
    if (n < 0 || !skin_loss_kind_ok(kind)) return GS_E_BAD_ARG;
    if (n == 0) return GS_OK;
    if (!logits || !target || !dL_dloss || !dL_dlogits) return GS_E_BAD_ARG;
    if (!skin_a16(logits) || !skin_a16(target) || !skin_a4(dL_dloss) || !skin_a16(dL_dlogits)) return GS_E_BAD_ARG;
    return launch_skin_loss_backward(n, kind, logits, target, dL_dloss, dL_dlogits, (hipStream_t)stream);
}

// ---- SMPL pose correction (pose.hip)
static bool pose_a4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
static bool pose_req(const void* p) { return p && pose_a4(p); }
static int pose_validate(const GsPoseArgs* a) {
    if (!a || a->V < 1 || a->NB < 1 || a->NB > GS_POSE_MAX_BETAS) return GS_E_BAD_ARG;
    for (int i = 1; i < GS_POSE_BONES; i++)
        if (a->parents[i] < 0 || a->parents[i] >= i) return GS_E_BAD_ARG;
    if (!pose_req(a->J_shapedirs) || !pose_req(a->root_orient) || !pose_req(a->pose_body) || !pose_req(a->pose_hand) ||
        !pose_a4(a->rots_gt))
        return GS_E_BAD_ARG;
    return GS_OK;
}
int gs_pose_workspace_bytes(int32_t V, size_t* out) {
    if (!out || V < 1) return GS_E_BAD_ARG;
    *out = pose_workspace_bytes(V);
    return GS_OK;
}
int gs_pose_forward(const GsPoseArgs* a, float* rots, float* Jtrs, float* bone_transforms, float* loss_pose, float* state,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = pose_validate(a)) return rc;
    if (!pose_req(a->v_template) || !pose_req(a->shapedirs) || !pose_req(a->J_template) || !pose_req(a->betas) ||
        !pose_req(a->trans) || !pose_req(rots) || !pose_req(Jtrs) || !pose_req(bone_transforms) || !pose_req(state) ||
        !pose_a4(loss_pose) || (a->rots_gt && !loss_pose))
        return GS_E_BAD_ARG;
    if (!workspace || ((uintptr_t)workspace & 7u)) return GS_E_BAD_ARG;
    if (workspace_bytes < pose_workspace_bytes(a->V)) return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_pose_forward(a, rots, Jtrs, bone_transforms, loss_pose, state, workspace, (hipStream_t)stream);
}
int gs_pose_backward(const GsPoseArgs* a, const float* state, const float* dL_drots, const float* dL_dJtrs,
                     const float* dL_dbone_transforms, const float* dL_dloss_pose, float* dL_dbetas, float* dL_droot_orient,
                     float* dL_dpose_body, float* dL_dpose_hand, float* dL_dtrans, void* stream) {
    if (const int rc = pose_validate(a)) return rc;
    if (!pose_req(state) || !pose_a4(dL_drots) || !pose_a4(dL_dJtrs) || !pose_a4(dL_dbone_transforms) || !pose_a4(dL_dloss_pose) ||
        !pose_a4(dL_dbetas) || !pose_a4(dL_droot_orient) || !pose_a4(dL_dpose_body) || !pose_a4(dL_dpose_hand) || !pose_a4(dL_dtrans))
        return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    if (!dL_dbetas && !dL_droot_orient && !dL_dpose_body && !dL_dpose_hand && !dL_dtrans) return GS_OK;
    return launch_pose_backward(a, state, dL_drots, dL_dJtrs, dL_dbone_transforms, dL_dloss_pose, dL_dbetas, dL_droot_orient,
                                dL_dpose_body, dL_dpose_hand, dL_dtrans, (hipStream_t)stream);
}

// ---- the non-rigid deformer around its MLP (nonrigid.hip)
static bool nr_a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static int pose_enc_validate(const GsPoseEncArgs* a) {
    if (!a || a->d < 1 || a->d > GS_POSE_ENC_MAX_DIM) return GS_E_BAD_ARG;
    for (int i = 1; i < GS_POSE_ENC_JOINTS; i++)
        if (a->parents[i] < 0 || a->parents[i] >= i) return GS_E_BAD_ARG;
    if (!pose_req(a->W0)) return GS_E_BAD_ARG;
    for (int j = 0; j < GS_POSE_ENC_JOINTS; j++)
        if (!pose_req(a->W1[j]) || !pose_req(a->W2[j])) return GS_E_BAD_ARG;
    return GS_OK;
}
int gs_pose_encoder_grad_floats(int32_t d, size_t* out) {
    if (!out || d < 1 || d > GS_POSE_ENC_MAX_DIM) return GS_E_BAD_ARG;
    *out = pose_encoder_grad_floats(d);
    return GS_OK;
}
int gs_pose_encoder_forward(const GsPoseEncArgs* a, float* out, float* state, void* stream) {
    if (const int rc = pose_enc_validate(a)) return rc;
    if (!pose_req(a->rots) || !pose_req(a->Jtrs) || !pose_req(a->b0) || !pose_req(out) || !pose_req(state)) return GS_E_BAD_ARG;
    for (int j = 0; j < GS_POSE_ENC_JOINTS; j++)
        if (!pose_req(a->b1[j]) || !pose_req(a->b2[j])) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_pose_encoder_forward(a, out, state, (hipStream_t)stream);
}
int gs_pose_encoder_backward(const GsPoseEncArgs* a, const float* state, const float* dL_dout, float* dL_dparams,
                             float* dL_drots, float* dL_dJtrs, void* stream) {
    if (const int rc = pose_enc_validate(a)) return rc;
    if (!pose_req(state) || !pose_req(dL_dout) || !pose_a4(dL_dparams) || !pose_a4(dL_drots) || !pose_a4(dL_dJtrs))
        return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    if (!dL_dparams && !dL_drots && !dL_dJtrs) return GS_OK;
    return launch_pose_encoder_backward(a, state, dL_dout, dL_dparams, dL_drots, dL_dJtrs, (hipStream_t)stream);
}
static bool nr_shape_ok(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset) {
    return N >= 0 && D >= 10 && D <= GS_NONRIGID_MAX_D &&
           (scale_offset == GS_NR_SCALE_LOGIT || scale_offset == GS_NR_SCALE_EXP || scale_offset == GS_NR_SCALE_ZERO) &&
           (rot_offset == GS_NR_ROT_ADD || rot_offset == GS_NR_ROT_MULT);
}
int gs_nonrigid_workspace_bytes(int32_t N, int32_t D, size_t* out) {
    if (!out || N < 0 || D < 10 || D > GS_NONRIGID_MAX_D) return GS_E_BAD_ARG;
    *out = nonrigid_workspace_bytes(N, D);
    return GS_OK;
}
int gs_nonrigid_apply_forward(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset, const float* deltas,
                              const float* xyz, const float* scaling, const float* rotation, float* xyz_out,
                              float* scaling_out, float* rotation_out, float* feature, float* losses, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!nr_shape_ok(N, D, scale_offset, rot_offset)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!deltas || !xyz || !rotation || !xyz_out || !rotation_out || (D > 10 && !feature)) return GS_E_BAD_ARG;
    if (scale_offset != GS_NR_SCALE_ZERO && (!scaling || !scaling_out)) return GS_E_BAD_ARG;
    if (scaling_out && !scaling) return GS_E_BAD_ARG;
    if (!nr_a16(deltas) || !nr_a16(rotation) || !nr_a16(rotation_out) || !nr_a16(feature) || !pose_a4(xyz) || !pose_a4(scaling) ||
        !pose_a4(xyz_out) || !pose_a4(scaling_out) || !pose_a4(losses))
        return GS_E_BAD_ARG;
    if (losses) {
        if (!workspace || !pose_a4(workspace)) return GS_E_BAD_ARG;
        if (workspace_bytes < nonrigid_workspace_bytes(N, D)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    return launch_nonrigid_apply_forward(N, D, scale_offset, rot_offset, deltas, xyz, scaling, rotation, xyz_out, scaling_out,
                                         rotation_out, D > 10 ? feature : nullptr, losses, workspace, (hipStream_t)stream);
}
int gs_nonrigid_apply_backward(int32_t N, int32_t D, int32_t scale_offset, int32_t rot_offset, const float* deltas,
                               const float* scaling, const float* rotation, const float* dL_dxyz_out,
                               const float* dL_dscaling_out, const float* dL_drotation_out, const float* dL_dfeature,
                               const float* dL_dnr_xyz, const float* dL_dnr_scale, const float* dL_dnr_rot,
                               float* dL_ddeltas, float* dL_dscaling, float* dL_drotation, void* stream) {
    if (!nr_shape_ok(N, D, scale_offset, rot_offset)) return GS_E_BAD_ARG;
    if (N == 0) return GS_OK;
    if (!deltas || (scale_offset == GS_NR_SCALE_EXP && !scaling) || (rot_offset == GS_NR_ROT_MULT && !rotation)) return GS_E_BAD_ARG;
    if (!nr_a16(deltas) || !nr_a16(rotation) || !nr_a16(dL_drotation_out) || !nr_a16(dL_dfeature) || !nr_a16(dL_ddeltas) ||
        !nr_a16(dL_drotation) || !pose_a4(scaling) || !pose_a4(dL_dxyz_out) || !pose_a4(dL_dscaling_out) || !pose_a4(dL_dnr_xyz) ||
        !pose_a4(dL_dnr_scale) || !pose_a4(dL_dnr_rot) || !pose_a4(dL_dscaling))
        return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    if (!dL_ddeltas && !dL_dscaling && !dL_drotation) return GS_OK;
    return launch_nonrigid_apply_backward(N, D, scale_offset, rot_offset, deltas, scaling, rotation, dL_dxyz_out, dL_dscaling_out,
                                          dL_drotation_out, D > 10 ? dL_dfeature : nullptr, dL_dnr_xyz, dL_dnr_scale, dL_dnr_rot,
                                          dL_ddeltas, dL_dscaling, dL_drotation, (hipStream_t)stream);
}

// ---- the input of the ColorMLP texture (texture.hip)
static int texture_validate(const GsTextureArgs* a) {
    if (!a || a->N < 0 || a->sh_degree < 0 || a->sh_degree > 4 || a->n_before < 0 || a->n_before > GS_TEXTURE_MAX_BEFORE ||
        a->n_after < 0 || a->n_after > GS_TEXTURE_MAX_AFTER || a->latent_dim < 0 || a->latent_dim > GS_TEXTURE_MAX_D)
        return GS_E_BAD_ARG;
    int64_t sum = (a->sh_degree + 1) * (a->sh_degree + 1) - 1 + a->latent_dim;
    for (int b = 0; b < a->n_before; b++) {
        if (a->before_w[b] < 1 || a->before_w[b] > GS_TEXTURE_MAX_D) return GS_E_BAD_ARG;
        sum += a->before_w[b];
    }
    for (int b = 0; b < a->n_after; b++) {
        if (a->after_w[b] < 1 || a->after_w[b] > GS_TEXTURE_MAX_D) return GS_E_BAD_ARG;
        sum += a->after_w[b];
    }
    if (a->D < 1 || a->D > GS_TEXTURE_MAX_D || sum != a->D) return GS_E_BAD_ARG;
    return GS_OK;
}
// what the view direction is made of (sh_degree > 0)
static bool texture_dir_ok(const GsTextureArgs* a) {
    if (!pose_req(a->xyz) || !pose_req(a->campos) || !pose_a4(a->fwd_transform)) return false;
    return !a->fwd_transform || (a->rot_row >= 3 && a->rot_stride >= 2 * (int64_t)a->rot_row + 3);
}
int gs_texture_workspace_bytes(int32_t N, int32_t D, int32_t latent_dim, size_t* out) {
    if (!out || N < 0 || D < 1 || D > GS_TEXTURE_MAX_D || latent_dim < 0 || latent_dim > D) return GS_E_BAD_ARG;
    *out = texture_workspace_bytes(N, D, latent_dim);
    return GS_OK;
}
int gs_texture_input_forward(const GsTextureArgs* a, float* inp, void* stream) {
    if (const int rc = texture_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!inp || !nr_a16(inp)) return GS_E_BAD_ARG;
    for (int b = 0; b < a->n_before; b++)
        if (!a->before[b] || !nr_a16(a->before[b])) return GS_E_BAD_ARG;
    for (int b = 0; b < a->n_after; b++)
        if (!a->after[b] || !nr_a16(a->after[b])) return GS_E_BAD_ARG;
    if (a->latent_dim > 0 && !pose_req(a->latent)) return GS_E_BAD_ARG;
    if (a->sh_degree > 0 && !texture_dir_ok(a)) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_texture_input_forward(a, inp, (hipStream_t)stream);
}
int gs_texture_input_backward(const GsTextureArgs* a, const float* dL_dinp, float* const* dL_dbefore, float* const* dL_dafter,
                              float* dL_dxyz, float* dL_dlatent, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = texture_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!dL_dinp || !nr_a16(dL_dinp)) return GS_E_BAD_ARG;
    TxGrads gr = {};
    bool any = dL_dxyz || dL_dlatent;
    for (int b = 0; b < a->n_before; b++) {
        gr.before[b] = dL_dbefore ? dL_dbefore[b] : nullptr;
        if (!nr_a16(gr.before[b])) return GS_E_BAD_ARG;
        any = any || gr.before[b];
    }
    for (int b = 0; b < a->n_after; b++) {
        gr.after[b] = dL_dafter ? dL_dafter[b] : nullptr;
        if (!nr_a16(gr.after[b])) return GS_E_BAD_ARG;
        any = any || gr.after[b];
    }
    if (dL_dxyz && (a->sh_degree == 0 || !pose_a4(dL_dxyz) || !texture_dir_ok(a))) return GS_E_BAD_ARG;
    if (dL_dlatent) {
        if (a->latent_dim == 0 || !pose_a4(dL_dlatent) || !workspace || !pose_a4(workspace)) return GS_E_BAD_ARG;
        if (workspace_bytes < texture_workspace_bytes(a->N, a->D, a->latent_dim)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    if (!any) return GS_OK;
    return launch_texture_input_backward(a, dL_dinp, gr, dL_dxyz, dL_dlatent, workspace, (hipStream_t)stream);
}

// ---- the fused VanillaCondMLP (mlp.hip)
static int mlp_validate(const GsMlpArgs* a) {
    if (!a || a->N < 0 || a->width < 32 || a->width > GS_MLP_MAX_WIDTH || a->width % 32 != 0 || a->n_hidden < 1 ||
        a->n_hidden > GS_MLP_MAX_HIDDEN || a->dim_in < 1 || a->dim_in > GS_MLP_MAX_IN || a->dim_cond < 0 ||
        a->dim_cond > GS_MLP_MAX_COND || a->dim_out < 1 || a->dim_out > GS_MLP_MAX_OUT || !(a->slope == a->slope))
        return GS_E_BAD_ARG;
    return GS_OK;
}
// x, the condition and every layer's parameters
static bool mlp_inputs_ok(const GsMlpArgs* a) {
    if (!a->x || !nr_a16(a->x) || (a->dim_cond > 0 && !pose_req(a->cond))) return false;
    for (int l = 0; l <= a->n_hidden; l++)
        if (!pose_req(a->W[l]) || !pose_req(a->b[l])) return false;
    return true;
}
int gs_mlp_workspace_bytes(const GsMlpArgs* a, int32_t backward, size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    if (const int rc = mlp_validate(a)) return rc;
    *out = mlp_workspace_bytes(a, backward != 0);
    return GS_OK;
}
int gs_mlp_forward(const GsMlpArgs* a, float* y, float* acts, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = mlp_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!mlp_inputs_ok(a) || !pose_req(y) || !nr_a16(acts)) return GS_E_BAD_ARG;
    if (a->dim_cond > 0) {
        if (!pose_req(workspace)) return GS_E_BAD_ARG;
        if (workspace_bytes < mlp_workspace_bytes(a, 0)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    return launch_mlp_forward(a, y, acts, workspace, (hipStream_t)stream);
}
int gs_mlp_backward(const GsMlpArgs* a, const float* acts, const float* dL_dy, void* workspace, size_t workspace_bytes,
                    void* stream) {
    if (const int rc = mlp_validate(a)) return rc;
    if (a->N == 0) return GS_OK;
    if (!mlp_inputs_ok(a) || !acts || !nr_a16(acts) || !dL_dy || !nr_a16(dL_dy) || !pose_a4(a->dx) || !pose_a4(a->dcond))
        return GS_E_BAD_ARG;
    if (a->dcond && a->dim_cond == 0) return GS_E_BAD_ARG;
    bool any = a->dx || a->dcond;
    for (int l = 0; l <= a->n_hidden; l++) {
        if (!pose_a4(a->dW[l]) || !pose_a4(a->db[l])) return GS_E_BAD_ARG;
        any = any || a->dW[l] || a->db[l];
    }
    if (any) {
        if (!workspace || !nr_a16(workspace)) return GS_E_BAD_ARG;
        if (workspace_bytes < mlp_workspace_bytes(a, 1)) return GS_E_WORKSPACE;
    }
    GS_CAPTURE_OK_IF(stream, true);
    if (!any) return GS_OK;
    return launch_mlp_backward(a, acts, dL_dy, workspace, (hipStream_t)stream);
}

// ---- the LPIPS-VGG perceptual loss (lpips.hip)
static bool lp_a16(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }
static int lpips_validate(const GsLpipsArgs* a) {
    if (!a || a->H < GS_LPIPS_MIN_SIZE || a->H > GS_LPIPS_MAX_SIZE || a->W < GS_LPIPS_MIN_SIZE || a->W > GS_LPIPS_MAX_SIZE)
        return GS_E_BAD_ARG;
    if (!pose_req(a->in0) || !pose_req(a->in1) || !lp_a16(a->packed)) return GS_E_BAD_ARG;
    if (a->cs0 < 1 || a->cs1 < 1 || a->rs0 < a->W || a->rs1 < a->W) return GS_E_BAD_ARG;
    return GS_OK;
}
int gs_lpips_packed_bytes(size_t* out) {
    if (!out) return GS_E_BAD_ARG;
    *out = lpips_packed_bytes();
    return GS_OK;
}
int gs_lpips_pack_weights(const GsLpipsArgs* a, void* packed, size_t packed_bytes, void* stream) {
    if (!a || !lp_a16(packed) || !pose_a4(a->shift) || !pose_a4(a->scale)) return GS_E_BAD_ARG;
    for (int l = 0; l < GS_LPIPS_LAYERS; l++)
        if (!pose_req(a->weight[l]) || !pose_req(a->bias[l])) return GS_E_BAD_ARG;
    for (int k = 0; k < GS_LPIPS_TAPS; k++)
        if (!pose_req(a->lin[k])) return GS_E_BAD_ARG;
    if (packed_bytes < lpips_packed_bytes()) return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_pack(a, (float*)packed, (hipStream_t)stream);
}
int gs_lpips_workspace_bytes(int32_t H, int32_t W, int32_t need_grad0, int32_t need_grad1, int32_t which, size_t* out) {
    if (!out || H < GS_LPIPS_MIN_SIZE || H > GS_LPIPS_MAX_SIZE || W < GS_LPIPS_MIN_SIZE || W > GS_LPIPS_MAX_SIZE || which < 0 ||
        which > GS_LPIPS_WS_BACKWARD)
        return GS_E_BAD_ARG;
    *out = lpips_workspace_bytes(H, W, need_grad0, need_grad1, which);
    return GS_OK;
}
int gs_lpips_forward(const GsLpipsArgs* a, float* loss, float* per_tap, void* saved, size_t saved_bytes, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (const int rc = lpips_validate(a)) return rc;
    if (!pose_req(loss) || !pose_a4(per_tap) || !lp_a16(workspace)) return GS_E_BAD_ARG;
    const size_t need_saved = lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_SAVED);
    if (need_saved && !lp_a16(saved)) return GS_E_BAD_ARG;
    if (saved_bytes < need_saved ||
        workspace_bytes < lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_FORWARD))
        return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_forward(a, loss, per_tap, (float*)saved, (float*)workspace, (hipStream_t)stream);
}
int gs_lpips_backward(const GsLpipsArgs* a, const float* dL_dloss, float* d_in0, float* d_in1, const void* saved,
                      size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = lpips_validate(a)) return rc;
    if (!pose_a4(dL_dloss) || !pose_a4(d_in0) || !pose_a4(d_in1)) return GS_E_BAD_ARG;
    if ((d_in0 && !a->need_grad0) || (d_in1 && !a->need_grad1)) return GS_E_BAD_ARG;
    if (!d_in0 && !d_in1) return GS_OK;
    if (!lp_a16(saved) || !lp_a16(workspace)) return GS_E_BAD_ARG;
    if (saved_bytes < lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_SAVED) ||
        workspace_bytes < lpips_workspace_bytes(a->H, a->W, a->need_grad0, a->need_grad1, GS_LPIPS_WS_BACKWARD))
        return GS_E_WORKSPACE;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_backward(a, dL_dloss, d_in0, d_in1, (const float*)saved, (float*)workspace, (hipStream_t)stream);
}
int gs_lpips_conv(const float* packed, int32_t layer, int32_t backward, int32_t normalize, int32_t H, int32_t W, const float* in,
                  int64_t in_cs, int64_t in_rs, const float* mask, float* out, void* stream) {
    if (!lp_a16(packed) || layer < 0 || layer >= GS_LPIPS_LAYERS || H < 1 || W < 1 || H > GS_LPIPS_MAX_SIZE || W > GS_LPIPS_MAX_SIZE)
        return GS_E_BAD_ARG;
    const bool image_in = layer == 0 && !backward, image_out = layer == 0 && backward;
    if (image_in ? (!pose_req(in) || in_cs < 1 || in_rs < W) : !lp_a16(in)) return GS_E_BAD_ARG;
    if (image_out ? !pose_req(out) : !lp_a16(out)) return GS_E_BAD_ARG;
    if (backward && !lp_a16(mask)) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_conv(packed, layer, backward, normalize, H, W, in, in_cs, in_rs, mask, out, (hipStream_t)stream);
}
int gs_lpips_pool(int32_t backward, int32_t H, int32_t W, int32_t C, const float* in, const float* g, const float* dp, float* out,
                  void* stream) {
    if (H < 1 || W < 1 || H > GS_LPIPS_MAX_SIZE || W > GS_LPIPS_MAX_SIZE || C < 4 || C > 512 || (C & 3) || !lp_a16(in) || !lp_a16(out))
        return GS_E_BAD_ARG;
    if (backward && (!lp_a16(g) || ((H >> 1) && (W >> 1) && !lp_a16(dp)))) return GS_E_BAD_ARG;
    GS_CAPTURE_OK_IF(stream, true);
    return launch_lpips_pool(backward, H, W, C, in, g, dp, out, (hipStream_t)stream);
}

int knn_points(int32_t Nq, const float* queries, int32_t Nr, const float* ref, int32_t K, float* dists, int64_t* idx,
               void* workspace, size_t workspace_bytes, void* stream) {
    GS_NO_CAPTURE(stream);
    if (Nq < 0 || Nr <= 0 || K < 1 || K > 8 || (Nq > 0 && (!queries || !dists || !idx)) || !ref || !workspace) return GS_E_BAD_ARG;
    if (Nq == 0) return GS_OK;
    return launch_knn_points(Nq, queries, Nr, ref, K, dists, (long long*)idx, workspace, workspace_bytes, (hipStream_t)stream);
}

int gs_pair_stats(const GsFwdArgs* a, const void* geom, size_t geom_bytes, const void* binning, size_t binning_bytes, const void* img,
                  size_t img_bytes, int64_t D, uint64_t* counts, void* stream) {
    GS_NO_CAPTURE(stream);
    GeomViewRO g;
    BinViewRO b;
    ImgViewRO im;
    const int rc = frame_states(a, geom, geom_bytes, binning, binning_bytes, img, img_bytes, D, &g, &b, &im,
                                [&]() -> int { return counts ? GS_OK : GS_E_BAD_ARG; });
    if (rc != GS_OK) return rc;
    return launch_pair_stats(g.rec, b.point_list, im.ranges, im.n_contrib, a->W, a->H, (unsigned long long*)counts, (hipStream_t)stream);
}

int gs_geom_field(void* geom, int32_t P, int32_t field, void** out) {
    if (!geom || !out || P < 0) return GS_E_BAD_ARG;
    const GeomView g = geom_state(geom, P);
    switch (field) {
        case GS_GEOM_DEPTHS: *out = g.depths; break;
        case GS_GEOM_TILES: *out = g.tiles; break;
        case GS_GEOM_REC: *out = g.rec; break;
        case GS_GEOM_CLAMPED: *out = g.clamped; break;
        case GS_GEOM_SORTED_IDX: *out = g.val0; break;
        case GS_GEOM_COUNT: *out = g.count; break;
        default: return GS_E_BAD_ARG;
    }
    return GS_OK;
}
int gs_binning_field(void* binning, int64_t D, int32_t W, int32_t H, int32_t field, void** out) {
    if (!binning || !out || D < 0) return GS_E_BAD_ARG;
    const BinView b = bin_state(binning, D);
    (void)W; (void)H;
    switch (field) {
        case GS_BIN_POINT_LIST: *out = b.point_list; break;  // (the tile id of every entry follows from the image state's ranges)
        case GS_BIN_QLIST: *out = b.qlist; break;            // quadrant (tile t, q): [4 ranges[t].x + q n_t, ... + qcount[t][q])
        default: return GS_E_BAD_ARG;
    }
    return GS_OK;
}
int gs_image_field(void* img, int32_t W, int32_t H, int32_t field, void** out) {
    if (!img || !out) return GS_E_BAD_ARG;
    // (long_lists 0 whatever the render was given: these fields sit in front of everything that depends on it, and the
    // chunk-parallel forward's exist without it on small images only -- null in the view otherwise)
    const ImgView im = img_state(img, W, H, 0);
    void* p = nullptr;
    switch (field) {
        case GS_IMG_RANGES: p = im.ranges; break;
        case GS_IMG_N_CONTRIB: p = im.n_contrib; break;
        case GS_IMG_FINAL_T: p = im.final_T; break;
        case GS_IMG_QCOUNT: p = im.qcount; break;
        case GS_IMG_NCON_C: p = im.ncon_c; break;
        case GS_IMG_ORDER: p = im.order; break;
        case GS_IMG_CW_HDR: p = im.cw_hdr; break;      // 16 words: units in use, entries per chunk, .., [4..11] items per XCD
        case GS_IMG_CW_UNITS: p = im.cw_units; break;  // FWDC_MAX_UNITS x {tile, chunk | chunks << 16}
        case GS_IMG_CW_FLAG: p = im.cw_flag; break;    // 4 FWDC_MAX_UNITS words: hits + 1 | dead << 31
        case GS_IMG_CW_REC: p = im.cw_rec; break;      // 4 FWDC_MAX_UNITS records of FWDC_SLOTS x 64 floats
    }
    if (!p) return GS_E_BAD_ARG;
    *out = p;
    return GS_OK;
}

int gs_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.on = on != 0;
    return GS_OK;
}
int gs_profile_reserve(int n_events) {
    // creating an event and RECORDING it for the first time each cost ~0.1 ms: done here, a timed loop would otherwise
    // show them as slow first steps
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t last = nullptr;
    while ((int)g_prof.pool.size() < n_events) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return GS_E_HIP;
        (void)hipEventRecord(e, nullptr);
        last = e;
        g_prof.pool.push_back(e);
    }
    if (last) (void)hipEventSynchronize(last);
    return GS_OK;
}
int gs_profile_filter(const char* stage) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    memset(g_prof.filter, 0, sizeof(g_prof.filter));
    if (stage) strncpy(g_prof.filter, stage, sizeof(g_prof.filter) - 1);
    return GS_OK;
}
int gs_profile_collect(int max, const char** names, float* ms, int32_t* launches, int32_t* n_out) {
    if (max < 0 || !n_out || (max > 0 && (!names || !ms || !launches))) return GS_E_BAD_ARG;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int n = 0;
    for (auto& r : g_prof.recs) {
        float t = 0.f;
        hipError_t e = hipEventSynchronize(r.b);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, r.a, r.b);
        if (e != hipSuccess) { gs_set_error((int)e, "profile.collect"); t = 0.f; }
        int k = 0;
        for (; k < n; k++) if (names[k] == r.name) break;
        if (k == n) {
            if (n < max) { names[n] = r.name; ms[n] = 0.f; launches[n] = 0; n++; } else k = -1;
        }
        if (k >= 0) { ms[k] += t; launches[k] += 1; }
        g_prof.pool.push_back(r.a);
        g_prof.pool.push_back(r.b);
    }
    g_prof.recs.clear();
    *n_out = n;
    return GS_OK;
}

int gs_tuning(const char* name, int value) {
    if (!name) return GS_E_BAD_ARG;
    for (const TuneSwitch& t : k_tune) {
        if (strcmp(name, t.name) != 0) continue;
        if (t.ok && !t.ok(value)) return GS_E_BAD_ARG;
        tune_state().v[t.key].store(value);
        return GS_OK;
    }
    return GS_E_BAD_ARG;
}

const char* gs_status_string(int code) {
    switch (code) {
        case GS_OK: return "ok";
        case GS_E_BAD_ARG: return "bad argument (null required pointer, non-positive size, unsupported SH degree / more than 16 SH coefficients, or rotations not 16-byte aligned)";
        case GS_E_EXCLUSIVE: return "provide exactly one of shs/colors_precomp and exactly one of (scales, rotations)/cov3D_precomp";
        case GS_E_TOO_LARGE: return "num_rendered or tile grid exceeds the supported index space";
        case GS_E_HIP: return "HIP error";
        case GS_E_WORKSPACE: return "state/workspace buffer smaller than gs_*_bytes requires";
        case GS_E_CAPTURE: return "the stream is being captured into a graph and this call is not capture-safe with these arguments (include/gsplat_mi355.h, \"Stream capture\"); nothing was enqueued";
        default: return "unknown status";
    }
}
int gs_last_hip_error(void) { return g_last_hip; }
const char* gs_last_stage(void) { return g_last_stage; }
const char* gs_build_info(void) { return "gsplat_mi355 gfx950 wave64 tile16 rec48"; }

}  // extern "C"
