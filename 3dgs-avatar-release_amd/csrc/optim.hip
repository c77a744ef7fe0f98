// optim.hip -- the per-Gaussian bookkeeping that follows the backward pass in the reference's training
// step:
//   * densification statistics: train.py:219-220 + scene/gaussian_model.py:464-466 -- three boolean-mask
//     indexed updates in torch (each a nonzero() with a host sync, gathers and scatters);
//   * Adam: scene/gaussian_model.py:201-216 builds torch.optim.Adam over six parameter groups
//     (lr per group, eps 1e-15): the foreach implementation launches ~10 kernels per group.
// Here: one streaming kernel for the statistics and ONE launch for the Adam step of all tensors.
#include "common.h"
#include "ordered_sum.h"
#include "boundary.h"

__global__ __launch_bounds__(256) void densify_stats_kernel(int N, const int32_t* __restrict__ radii,
                                                            const float* __restrict__ viewspace_grad,
                                                            float* __restrict__ max_radii2D,
                                                            float* __restrict__ xyz_gradient_accum,
                                                            float* __restrict__ denom) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int r = radii[i];
    if (r <= 0) return;  // visibility_filter = radii > 0
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
    const float gx = viewspace_grad[3 * (size_t)i], gy = viewspace_grad[3 * (size_t)i + 1];
    xyz_gradient_accum[i] += sqrtf(gx * gx + gy * gy);  // torch.norm(grad[:, :2], dim=-1)
    denom[i] += 1.0f;
}

static int launch_densify_stats(int N, const int32_t* radii, const float* viewspace_grad, float* max_radii2D,
                                float* xyz_gradient_accum, float* denom, hipStream_t s) {
    StageScope st("densify_stats", s);
    hipLaunchKernelGGL(densify_stats_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, radii, viewspace_grad, max_radii2D,
                       xyz_gradient_accum, denom);
    GS_LAUNCH_CHECK("densify_stats", 0, s);
    return GS_OK;
}

// torch.optim.Adam (no amsgrad, no weight decay, maximize = false), the arithmetic of its single-tensor
// path in fp32:  m += (g - m) (1 - b1);  v = v b2 + ((1 - b2) g) g;  p += -(lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
struct AdamBatch {
    GsAdamTensor t[GS_ADAM_MAX_TENSORS];
    long long start[GS_ADAM_MAX_TENSORS + 1];  // first 1024-element chunk of every tensor
    int n;
};

__global__ __launch_bounds__(256) void adam_kernel(AdamBatch b, float w1, float beta2, float w2, float eps, float bc1,
                                                   float bc2_sqrt) {
    // which tensor does this chunk belong to (wave-uniform, at most GS_ADAM_MAX_TENSORS steps)
    const long long chunk = blockIdx.x;
    int k = 0;
    while (k + 1 < b.n && chunk >= b.start[k + 1]) k++;
    const GsAdamTensor T = b.t[k];
    const long long base = (chunk - b.start[k]) * 1024;
    const float neg_step = -(T.lr / bc1);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long long i = base + j * 256 + threadIdx.x;
        if (i >= T.n) break;
        const float g = T.grad[i];
        float m = T.exp_avg[i], v = T.exp_avg_sq[i];
        m = m + (g - m) * w1;
        v = v * beta2 + (w2 * g) * g;
        const float den = sqrtf(v) / bc2_sqrt + eps;
        T.param[i] = T.param[i] + neg_step * (m / den);
        T.exp_avg[i] = m;
        T.exp_avg_sq[i] = v;
    }
}

static int launch_adam(int n, const GsAdamTensor* tensors, double beta1, double beta2, double eps, int64_t step, hipStream_t s) {
    AdamBatch b;
    b.n = n;
    long long chunks = 0;
    for (int k = 0; k < n; k++) {
        b.t[k] = tensors[k];
        b.start[k] = chunks;
        chunks += (tensors[k].n + 1023) / 1024;
    }
    b.start[n] = chunks;
    if (chunks == 0) return GS_OK;
    // every scalar is formed in double, as torch forms them from Python floats, and rounded to fp32 once
    // (1 - beta2 taken from an fp32 beta2 would be off by 1e-5)
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    StageScope st("adam", s);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)chunks), dim3(256), 0, s, b, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)eps, (float)bc1, (float)sqrt(bc2));
    GS_LAUNCH_CHECK("adam", 0, s);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------
// The converter's optimizer step (models/gaussian_converter.py:22-39,61-67): clip_grad_norm_ over ~130 parameter
// tensors, torch.optim.Adam with weight decay on two groups, and a step number that lives on the device so that the
// whole step can be captured into a hipGraph.  Four kernels:
//   grad_sumsq_kernel   one workgroup per fixed 2048-element chunk of one tensor: its sum of squares -> one partial
//   grad_norm_final     ONE workgroup adds the partials in a fixed order (strided_sum, then block_sum with the waves
//                       in order: ordered_sum.h; no atomics) -> total_norm, clip_coef
//   adam_begin_step     one thread per tensor: its device `step` scalar += 1 (a launch of its own in front of the
//                       update, so that no workgroup of the update races with the increment; an empty tensor's step
//                       advances too, as torch's does)
//   adam_ex_kernel      adam_kernel's arithmetic on clip_coef * g + weight_decay * p, one launch per batch of tensors
//   grad_scale_kernel   g *= clip_coef in place (the stand-alone clip_grad_norm_)
// The tensor tables travel by value; the batch sizes (include/gsplat_mi355.h) keep every kernel's arguments under 4 KB.
// ---------------------------------------------------------------------------------------------
#define OPT_CHUNK 2048  // elements per workgroup: 256 threads x 2 float4

struct GradBatch {
    const float* g[GS_GRAD_NORM_BATCH];
    long long n[GS_GRAD_NORM_BATCH];
    int start[GS_GRAD_NORM_BATCH + 1];  // first chunk of every tensor within this launch
    int count;
};
struct AdamExBatch {
    GsAdamTensorEx t[GS_ADAM_EX_BATCH];
    int start[GS_ADAM_EX_BATCH + 1];
    int count;
};
struct StepBatch {
    float* step[GS_ADAM_STEP_BATCH];
    int count;
};
static_assert(sizeof(GradBatch) <= 4000 && sizeof(AdamExBatch) + 64 <= 4000 && sizeof(StepBatch) <= 4000,
              "kernel arguments are limited to 4 KB");

// the tensor a chunk belongs to: the last k with start[k] <= chunk (wave-uniform binary search over kernel arguments)
__device__ __forceinline__ int chunk_owner(const int* start, int count, int chunk) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradBatch b, float* __restrict__ partials) {
    __shared__ float lds4[4];
    const int k = chunk_owner(b.start, b.count, (int)blockIdx.x);
    const float* __restrict__ g = b.g[k];
    const long long n = b.n[k];
    const long long base = (long long)((int)blockIdx.x - b.start[k]) * OPT_CHUNK;
    const bool vec = (((uintptr_t)g) & 15u) == 0;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < OPT_CHUNK / 1024; j++) {
        const long long i = base + ((long long)j * 256 + threadIdx.x) * 4;
        if (vec && i + 3 < n) {
            const float4 q = *reinterpret_cast<const float4*>(g + i);
            acc = __builtin_fmaf(q.x, q.x, acc);
            acc = __builtin_fmaf(q.y, q.y, acc);
            acc = __builtin_fmaf(q.z, q.z, acc);
            acc = __builtin_fmaf(q.w, q.w, acc);
        } else {
            for (int e = 0; e < 4; e++)
                if (i + e < n) acc = __builtin_fmaf(g[i + e], g[i + e], acc);  // (explicit: both paths round alike)
        }
    }
    const float s = block_sum<256, WavesInOrder>(acc, lds4);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[0] = total_norm, out[1] = clip_coef = min(max_norm / (total_norm + 1e-6), 1) the way torch.clamp(max=1) takes
// it: a NaN stays a NaN (fminf would return the 1)
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* __restrict__ partials, int n_partials, float max_norm,
                                                              float* __restrict__ out) {
    __shared__ float lds4[4];
    const float s = block_sum<256, WavesInOrder>(strided_sum<256>(partials, n_partials), lds4);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(s);
        float coef = max_norm / (norm + 1e-6f);
        coef = coef > 1.0f ? 1.0f : coef;
        out[0] = norm;
        out[1] = coef;
    }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(GradBatch b, const float* __restrict__ clip_coef) {
    const int k = chunk_owner(b.start, b.count, (int)blockIdx.x);
    float* __restrict__ g = const_cast<float*>(b.g[k]);
    const long long n = b.n[k];
    const long long base = (long long)((int)blockIdx.x - b.start[k]) * OPT_CHUNK;
    const bool vec = (((uintptr_t)g) & 15u) == 0;
    const float c = *clip_coef;
#pragma unroll
    for (int j = 0; j < OPT_CHUNK / 1024; j++) {
        const long long i = base + ((long long)j * 256 + threadIdx.x) * 4;
        if (vec && i + 3 < n) {
            float4 q = *reinterpret_cast<const float4*>(g + i);
            q.x *= c; q.y *= c; q.z *= c; q.w *= c;
            *reinterpret_cast<float4*>(g + i) = q;
        } else {
            for (int e = 0; e < 4; e++)
                if (i + e < n) g[i + e] *= c;
        }
    }
}

__global__ __launch_bounds__(256) void adam_begin_step_kernel(StepBatch b) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < b.count) *b.step[k] += 1.0f;
}

struct AdamScalars {
    float clip, wd, w1, beta2, w2, eps, bc2_sqrt, neg_step;
};
// A product that is rounded to fp32 HERE: this file is compiled with -ffp-contract=fast, under which the backend may fuse any
// product into a following sum (a pragma does not stop it), and the eager, the capturable and the old single-launch path
// must round alike.  The empty statement makes the value opaque to the optimiser; it costs no instruction.
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}
// adam_kernel's arithmetic, written out so that it rounds where adam_kernel rounds (m and p by one FMA each, v by
// three rounded products and a sum), on the effective gradient clip * g + wd * p (each product and the sum rounded, as
// torch rounds them; the sum is skipped without weight decay, as torch skips it)
__device__ __forceinline__ void adam_ex_elem(const AdamScalars& c, float g, float& p, float& m, float& v) {
    g = rounded(c.clip * g);
    if (c.wd != 0.f) g = rounded(g + rounded(c.wd * p));
    m = __builtin_fmaf(g - m, c.w1, m);
    v = rounded(v * c.beta2) + rounded(rounded(c.w2 * g) * g);
    const float den = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = __builtin_fmaf(c.neg_step, m / den, p);
}

__global__ __launch_bounds__(256) void adam_ex_kernel(AdamExBatch b, double beta1, double beta2, float eps, float host_bc1,
                                                      float host_bc2_sqrt, const float* __restrict__ clip_coef) {
    const int k = chunk_owner(b.start, b.count, (int)blockIdx.x);
    const GsAdamTensorEx T = b.t[k];
    const long long base = (long long)((int)blockIdx.x - b.start[k]) * OPT_CHUNK;
    float bc1 = host_bc1, bc2_sqrt = host_bc2_sqrt;
    if (T.step) {
        // the same doubles launch_adam forms on the host, rounded to fp32 once
        const double step = (double)*T.step;
        bc1 = (float)(1.0 - pow(beta1, step));
        bc2_sqrt = (float)sqrt(1.0 - pow(beta2, step));
    }
    const float lr = T.lr_dev ? *T.lr_dev : T.lr;
    AdamScalars c;
    c.clip = clip_coef ? *clip_coef : 1.0f;
    c.wd = T.weight_decay;
    c.w1 = (float)(1.0 - beta1);
    c.beta2 = (float)beta2;
    c.w2 = (float)(1.0 - beta2);
    c.eps = eps;
    c.bc2_sqrt = bc2_sqrt;
    c.neg_step = -(lr / bc1);
    const bool vec = (((uintptr_t)T.param | (uintptr_t)T.grad | (uintptr_t)T.exp_avg | (uintptr_t)T.exp_avg_sq) & 15u) == 0;
#pragma unroll
    for (int j = 0; j < OPT_CHUNK / 1024; j++) {
        const long long i = base + ((long long)j * 256 + threadIdx.x) * 4;
        if (vec && i + 3 < T.n) {
            const float4 g = *reinterpret_cast<const float4*>(T.grad + i);
            float4 p = *reinterpret_cast<const float4*>(T.param + i);
            float4 m = *reinterpret_cast<const float4*>(T.exp_avg + i);
            float4 v = *reinterpret_cast<const float4*>(T.exp_avg_sq + i);
            adam_ex_elem(c, g.x, p.x, m.x, v.x);
            adam_ex_elem(c, g.y, p.y, m.y, v.y);
            adam_ex_elem(c, g.z, p.z, m.z, v.z);
            adam_ex_elem(c, g.w, p.w, m.w, v.w);
            *reinterpret_cast<float4*>(T.param + i) = p;
            *reinterpret_cast<float4*>(T.exp_avg + i) = m;
            *reinterpret_cast<float4*>(T.exp_avg_sq + i) = v;
        } else {
            for (int e = 0; e < 4; e++) {
                if (i + e >= T.n) break;
                float p = T.param[i + e], m = T.exp_avg[i + e], v = T.exp_avg_sq[i + e];
                adam_ex_elem(c, T.grad[i + e], p, m, v);
                T.param[i + e] = p;
                T.exp_avg[i + e] = m;
                T.exp_avg_sq[i + e] = v;
            }
        }
    }
}

static inline long long opt_chunks(long long n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }

static size_t grad_norm_workspace_bytes(int n, const GsGradTensor* tensors) {
    long long chunks = 0;
    for (int k = 0; k < n; k++) chunks += opt_chunks(tensors[k].n);
    return (size_t)(chunks > 0 ? chunks : 1) * sizeof(float);
}

// fills one by-value table with the next tensors that have elements (at most GS_GRAD_NORM_BATCH of them, and fewer
// than 2^31 chunks); returns the index of the first tensor left over
static int next_grad_batch(int n, const GsGradTensor* tensors, int k, GradBatch& b) {
    b.count = 0;
    long long chunks = 0;
    for (; k < n && b.count < GS_GRAD_NORM_BATCH; k++) {
        if (tensors[k].n == 0) continue;
        const long long c = opt_chunks(tensors[k].n);
        if (b.count > 0 && chunks + c > 0x7fffffffLL) break;
        b.g[b.count] = tensors[k].grad;
        b.n[b.count] = tensors[k].n;
        b.start[b.count++] = (int)chunks;
        chunks += c;
    }
    b.start[b.count] = (int)chunks;
    return k;
}

static int launch_grad_norm(int n, const GsGradTensor* tensors, float max_norm, float* out, float* workspace, hipStream_t s) {
    StageScope st("grad_norm", s);
    GradBatch b;
    long long done = 0;
    for (int k = 0; k < n;) {
        k = next_grad_batch(n, tensors, k, b);
        if (b.count == 0) break;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)b.start[b.count]), dim3(256), 0, s, b, workspace + done);
        GS_LAUNCH_CHECK("grad_norm.partials", 0, s);
        done += b.start[b.count];
    }
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (int)done, max_norm, out);
    GS_LAUNCH_CHECK("grad_norm.final", 0, s);
    return GS_OK;
}

static int launch_grad_scale(int n, const GsGradTensor* tensors, const float* clip_coef, hipStream_t s) {
    StageScope st("grad_scale", s);
    GradBatch b;
    for (int k = 0; k < n;) {
        k = next_grad_batch(n, tensors, k, b);
        if (b.count == 0) break;
        hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)b.start[b.count]), dim3(256), 0, s, b, clip_coef);
        GS_LAUNCH_CHECK("grad_scale", 0, s);
    }
    return GS_OK;
}

static int launch_adam_ex(int n, const GsAdamTensorEx* tensors, double beta1, double beta2, double eps, int64_t step,
                          const float* clip_coef, hipStream_t s) {
    StageScope st("adam_ex", s);
    // every device step number first, each in a launch of its own in front of the updates
    {
        StepBatch sb;
        sb.count = 0;
        for (int k = 0; k <= n; k++) {
            if (k < n && tensors[k].step) sb.step[sb.count++] = tensors[k].step;
            if (sb.count == GS_ADAM_STEP_BATCH || (k == n && sb.count > 0)) {
                hipLaunchKernelGGL(adam_begin_step_kernel, dim3((sb.count + 255) / 256), dim3(256), 0, s, sb);
                GS_LAUNCH_CHECK("adam_ex.begin_step", 0, s);
                sb.count = 0;
            }
        }
    }
    float bc1 = 1.f, bc2_sqrt = 1.f;
    if (step >= 1) {
        bc1 = (float)(1.0 - pow(beta1, (double)step));
        bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    }
    AdamExBatch b;
    for (int k = 0; k < n;) {
        b.count = 0;
        long long chunks = 0;
        for (; k < n && b.count < GS_ADAM_EX_BATCH; k++) {
            if (tensors[k].n == 0) continue;
            const long long c = opt_chunks(tensors[k].n);
            if (b.count > 0 && chunks + c > 0x7fffffffLL) break;
            b.t[b.count] = tensors[k];
            b.start[b.count++] = (int)chunks;
            chunks += c;
        }
        if (b.count == 0) break;
        b.start[b.count] = (int)chunks;
        hipLaunchKernelGGL(adam_ex_kernel, dim3((unsigned)chunks), dim3(256), 0, s, b, beta1, beta2, (float)eps, bc1, bc2_sqrt,
                           clip_coef);
        GS_LAUNCH_CHECK("adam_ex", 0, s);
    }
    return GS_OK;
}

extern "C" {

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

// ---- the converter's optimizer step: every argument check comes before the first HIP call
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

}  // extern "C"
