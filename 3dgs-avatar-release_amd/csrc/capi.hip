// capi.hip -- the frame path's part of the extern "C" boundary declared in include/gsplat_mi355.h (every other module's
// entry points close its own .hip), and what the whole boundary shares: error state, tuning switches, the stage timer, the
// capture query.  Host-side sequencing of the stages; no device allocation, no implicit synchronisation (except in debug mode).
#include "common.h"
#include "boundary.h"
#include "sorted_lists.h"
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
    // GSPLAT_FWD4=0|1: the forward of the tiles marked as long on small images -- one wave per quadrant, or four waves x four
    // entries per step
    {"fwd4", GS_TUNE_FWD4, 1, "GSPLAT_FWD4", [](int v) { return v == 0 || v == 1; }},
    {"small_tiles", GS_TUNE_SMALL_TILES, BWD_CHUNK_MAX_TILES, nullptr, nullptr},  // changes the image state's size
    {"shared_qlist", GS_TUNE_SHARED_QLIST, 1, nullptr, nullptr},
    {"ones_fast", GS_TUNE_ONES_FAST, 1, nullptr, nullptr},
    {"bwd_order", GS_TUNE_BWD_ORDER, 1, nullptr, nullptr},  // 0: the backward walks the tiles in the forward's launch order (A/B: + 12 us at config 3)
    {"fwd_marks", GS_TUNE_FWD_MARKS, 1, nullptr, nullptr},  // 0: the backward sets its row marks itself (A/B)
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
bool profiling_on() { return g_prof.on; }
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
    if (!aligned(a->rotations, 16)) return GS_E_BAD_ARG;
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
bool stream_is_capturing(void* stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing((hipStream_t)stream, &st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        // (asking about the legacy stream while another stream captures in global mode is itself a capture error)
        return e == hipErrorStreamCaptureImplicit || e == hipErrorStreamCaptureUnsupported || e == hipErrorStreamCaptureInvalidated;
    }
    return st != hipStreamCaptureStatusNone;
}
// (GS_CAPTURE_OK_IF / GS_NO_CAPTURE, what every entry point asks with: boundary.h)

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
            rc = launch_rank_list(PairSort{g.key0, g.val0, g.key1, g.val1, g.hist}.sorted_vals(32), g.rec, g.tiles, g.ranklist, g.chunk_pairs, a->P, a->debug, s); }
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
    if (a->P > 0) {
        rc = launch_tile_lists(g.ranklist, g.chunk_pairs, g.seg_start, a->P, im.gx, im.gy,
                               TileCounts{im.seg_cnt, im.tile_tot, im.tile_zero_bytes}, im.ranges, im.order,
                               b.point_list, pc,
                               LongLists{forward_small_image(im.ntiles, a->long_lists) ? 1 : 0, (long long*)a->frame_stats},
                               totals_zeroed, a->debug, s);
        if (rc != GS_OK) return rc;
    } else {
        rc = gs_zero_async(im.ranges, (size_t)im.ntiles * 8, "ranges.zero", s);
        if (rc != GS_OK) return rc;
        StageScope sc_("ranges_order", s);
        rc = launch_tile_order(im.ranges, nullptr, 0, im.ntiles, im.order, pc, FillJob{nullptr, 0},
                               LongLists{0, nullptr}, a->debug, s);
        if (rc != GS_OK) return rc;
    }
    QuadLists ql = quad_lists(im, b, a->long_lists);
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
                            not_ones ? &so : nullptr, s);
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
        if (!aligned(gr->dL_drotations, 16)) return GS_E_BAD_ARG;  // written as float4
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
    { StageScope sc_("gaussian_bwd", s);
    rc = launch_gaussian_backward(*a, radii, g.rec, g.tiles, g.clamped, reinterpret_cast<const uint32_t*>(b.marks),
                                  (const float*)scratch, sums, b.marks_flag, *gr, s); }
    if (rc != GS_OK || !second || !second->dL_dcolors) return rc;
    // the second image's own colour gradient (second_colors.hip): a forward-shaped walk of the tile lists, its per-pair rows
    // in the rows region of the scratch, which the per-Gaussian backward enqueued above was the last to read
    { StageScope sc_("second_colors", s);
    rc = launch_second_colors(g.rec, g.tiles, radii, b.point_list, im.ranges, im.order, im.n_contrib, second->dL_dpix, a->P, a->W,
                              a->H, D, PairCount{g.count + COUNT_PAIRS, (uint32_t)D}, few_long_lists_mode(im.ntiles, a->long_lists),
                              scratch, scratch_rows_bytes(D),
                              second->dL_dcolors, a->debug, s); }
    if (rc != GS_OK) return rc;
    return sync_if_debug(a, "second_colors", s);
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
    // (long_lists 0 whatever the render was given: these fields sit in front of everything that depends on it)
    const ImgView im = img_state(img, W, H, 0);
    void* p = nullptr;
    switch (field) {
        case GS_IMG_RANGES: p = im.ranges; break;
        case GS_IMG_N_CONTRIB: p = im.n_contrib; break;
        case GS_IMG_FINAL_T: p = im.final_T; break;
        case GS_IMG_QCOUNT: p = im.qcount; break;
        case GS_IMG_NCON_C: p = im.ncon_c; break;
        case GS_IMG_ORDER: p = im.order; break;
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
