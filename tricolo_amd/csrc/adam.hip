// The optimizer step of TriCoLo (gfx950): overflow guard, step counter, global-norm gradient clipping, dynamic loss scaling and the fused
// Adam update.
// A gradient is read in one of two ways - flat, or through a (pointer, start) segment table - and each reader is written once
// (FlatReader, SegReader); the guard and the sum of squares are two operations over either reader, the update has one kernel per reader.
#include "common.h"
#include "../../include/tricolo_hip.h"
#include <stdio.h>

// ------------------------------------------------------------------------------------------------ fused Adam
// torch.optim.Adam(lr, betas, eps, weight_decay) single-tensor update, L2-in-gradient (config.yaml:50-53,
// tricolo_net.py:43-44).  `step` lives on the device (incremented by tri_adam_tick) so the launch is graph-replayable.
// `step` is a device int[4]: [0] optimizer steps APPLIED (the t of the bias corrections), [1] gradient elements skipped by the per-element
// guard below, [2] the attempt number (applied + skipped steps + 1) of the last step whose gradient tri_adam_guard* found non-finite,
// [3] steps skipped WHOLE for that reason.  Per-step guard (VERDICT r3 item 9 / ADVICE r3): one inf / NaN in an f16 activation gradient
// poisons the BatchNorm-backward sums and through them every gradient further down that tower, so skipping the bad ELEMENTS trains
// the healthy towers on while one tower stands still.  tri_adam_guard* scans the step's gradient once (before the tick); a bad
// gradient makes tri_adam_tick count a skipped step instead of an applied one and the update kernels leave p, m and v untouched -
// what torch.cuda.amp.GradScaler does with an overflowed step.  All device-side: the decision replays inside a captured HIP graph.
__global__ void adam_tick_kernel(int* step) {
    const int attempt = step[0] + step[3] + 1;
    if (step[2] == attempt) step[3] += 1;                          // the guard flagged this attempt: nothing is applied
    else step[0] += 1;
}
extern "C" int tri_adam_tick(int* step, void* stream) {
    adam_tick_kernel<<<1, 1, 0, (hipStream_t)stream>>>(step);
    return tri_check_launch("tri_adam_tick");
}
__device__ __forceinline__ bool adam_step_skipped(const int* step) { return step[2] == step[0] + step[3]; }   // (after the tick)

// ------------------------------------------------------------------------------------------------ the two gradient readers
// Segment table: device pointer and flat start offset of every parameter, ascending - the gradients are read in place from the
// per-parameter tensors autograd produced, no concatenation pass over the 74 MB of gradients first.  Segment sizes / starts are multiples
// of 4 and the gradient tensors 16-byte aligned (checked by the caller), so the table is walked in float4s.  A NULL pointer is a parameter
// without a gradient: torch.optim.Adam leaves its p, m, v untouched, and it is not part of the norm.
#define ADAM_MAX_SEG 1024
struct SegTable {                                                   // the table's copy in LDS (16 KiB): seg_stage makes it, seg_load reads it
    const long* start;
    const float* const* ptr;
    int nseg;
};
__device__ __forceinline__ SegTable seg_stage(const float* const* __restrict__ gptr, const long* __restrict__ gstart, int nseg) {
    __shared__ long sstart[ADAM_MAX_SEG];
    __shared__ const float* sptr[ADAM_MAX_SEG];
    for (int i = threadIdx.x; i < nseg; i += 256) { sstart[i] = gstart[i]; sptr[i] = gptr[i]; }
    __syncthreads();
    return SegTable{sstart, sptr, nseg};
}
// gv = the gradient's float4 at flat float4 index i4; false (gv untouched) when that parameter has no gradient
__device__ __forceinline__ bool seg_load(const SegTable& t, long i4, float4& gv) {
    const long i = i4 * 4;
    int lo = 0, hi = t.nseg - 1;                                    // last segment whose start is <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.start[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const float* gs = t.ptr[lo];
    if (gs) gv = *(const float4*)(gs + (i - t.start[lo]));
    return gs != nullptr;
}
// A reader hands every element of the gradient to an operation exactly once: op.vec(float4) from the grid-stride loop, op.one(float) for
// what does not fill a float4.  The order is part of the contract (the sum of squares adds in it): per thread the grid-stride body first,
// then, in workgroup 0, the head element, then the tail element.  i0 / stride: the grid-stride loop's start and step, taken in the kernel
// itself (blockDim folds to a scalar load there, not inside an inlined function).
struct SegReader {
    const float* const* gptr;
    const long* gstart;
    int nseg;
    long n4;
    template <typename Op>
    __device__ __forceinline__ void scan(Op& op, long i0, long stride) const {
        const SegTable t = seg_stage(gptr, gstart, nseg);
        float4 gv;
        for (long i4 = i0; i4 < n4; i4 += stride)
            if (seg_load(t, i4, gv)) op.vec(gv);
    }
};
struct FlatReader {                                                 // any n >= 0, g 4-byte aligned
    const float* g;
    long n;
    template <typename Op>
    __device__ __forceinline__ void scan(Op& op, long i0, long stride) const {
        // scalar head up to the first 16-byte boundary, float4 body, scalar tail
        long head = (long)(((16 - ((uintptr_t)g & 15)) & 15) >> 2);
        if (head > n) head = n;
        const long n4 = (n - head) >> 2, tail0 = head + n4 * 4;
        const float4* body = (const float4*)(g + head);
        for (long i = i0; i < n4; i += stride) op.vec(body[i]);
        if (blockIdx.x == 0) {
            if ((long)threadIdx.x < head) op.one(g[threadIdx.x]);
            if ((long)threadIdx.x < n - tail0) op.one(g[tail0 + threadIdx.x]);
        }
    }
};
// Grids of the scans.  tri_grad_norm_blocks reports scan_grid(n): one more float4 than n / 4, for the flat reader's head and tail.  The
// segmented guard runs over the compacted list of the gradients no writer vouched for and keeps the grid it has always had.
static inline int scan_grid(long n) { return ew_grid(n / 4 + 1); }

// ------------------------------------------------------------------------------------------------ the two scans
// Guard: OR of the non-finite bits, then one atomicMax per wave that saw one (see adam_tick_kernel).
struct GuardOp {
    int* step;
    unsigned bad;
    __device__ __forceinline__ void vec(const float4& v) {
        const unsigned e = 0x7f800000u;
        bad |= (unsigned)((__builtin_bit_cast(unsigned, v.x) & e) == e) | (unsigned)((__builtin_bit_cast(unsigned, v.y) & e) == e) |
               (unsigned)((__builtin_bit_cast(unsigned, v.z) & e) == e) | (unsigned)((__builtin_bit_cast(unsigned, v.w) & e) == e);
    }
    __device__ __forceinline__ void one(float x) { bad |= (unsigned)!__builtin_isfinite(x); }
    __device__ __forceinline__ void finish() {
        if (__any(bad) && (threadIdx.x & 63) == 0) atomicMax(step + 2, step[0] + step[3] + 1);
    }
};
// Global-norm clipping decided on the device (torch.nn.utils.clip_grad_norm_'s rule), so that it replays inside a captured HIP graph and
// sees the gradient AFTER the data-parallel all-reduce: (1) every workgroup sums (double)g * (double)g over its grid-stride share of the
// elements - a function of n and the grid only - and stores ONE double in partial[blockIdx.x]; (2) one workgroup adds the partials in a
// fixed order and leaves the norm and the coefficient in rec[0..1]; (3) the update kernels read rec[1].  No atomics and no ticket
// anywhere (a ticket taken by 4,096 workgroups on one address cost 110 us in the guard): two runs give the same bits.
struct SumsqOp {
    double* partial;
    double acc;
    __device__ __forceinline__ void vec(const float4& v) {
        acc += ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
    }
    __device__ __forceinline__ void one(float x) { acc += (double)x * (double)x; }
    __device__ __forceinline__ void finish() {
        __shared__ double sh[4];
        acc = block_sum_d(acc, sh);
        if (threadIdx.x == 0) partial[blockIdx.x] = acc;
    }
};
template <typename Reader, typename Op>
__global__ __launch_bounds__(256) void grad_scan_kernel(Reader reader, Op op) {
    reader.scan(op, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
    op.finish();
}
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const double* __restrict__ partial, int nblk, float gscale, float max_norm,
                                                             float* __restrict__ rec, int* __restrict__ clipped) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x != 0) return;
    const double total = fabs((double)gscale) * sqrt(acc);
    float c = 1.f;                                                  // inf / NaN norm: that step belongs to the guard, rec[0] says why
    if (__builtin_isfinite(total)) {
        const double cd = (double)max_norm / (total + 1e-6);
        if (cd < 1.0) c = (float)cd;
    }
    rec[0] = (float)total;
    rec[1] = c;
    if (c < 1.f) clipped[0] += 1;
}
// Dynamic loss scaling (torch.cuda.amp.GradScaler's back-off and growth), decided on the device.  The backward of the step was seeded with
// state[0] = s (the loss kernels take their upstream gradient as a device scalar), so every gradient of the step carries s; this launch
// stands where grad_clip_coef_kernel stands - after the tick, before the update - and does that kernel's work with 1 / s folded in:
// rec[0] is the norm of the TRUE gradient, rec[1] = c / s the one multiplier the *_clipped update kernels read.  Then it moves the scale for
// the NEXT backward: halved (down to min_scale) when the guard skipped this step, doubled (up to max_scale) after growth_interval applied
// steps in a row.  Every scale is a power of two (the entry point checks the bounds), so 1 / s, c / s and gscale / s are exact and s = 1
// leaves the bits grad_clip_coef_kernel leaves.  One workgroup, the partials added in that kernel's order; thread 0 writes, plain stores.
__global__ __launch_bounds__(256) void loss_scale_step_kernel(float* __restrict__ state, int* __restrict__ cnt, const int* __restrict__ step,
                                                              const double* __restrict__ partial, int nblk, float gscale, float max_norm,
                                                              int growth_interval, float min_scale, float max_scale,
                                                              float* __restrict__ rec, int* __restrict__ clipped) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
    acc = block_sum_d(acc, sh);
    if (threadIdx.x != 0) return;
    float s = state[0];
    const float inv = state[1];                                     // 1 / s of the scale this step's backward used
    const double total = fabs((double)gscale) * (double)inv * sqrt(acc);
    float c = 1.f;
    if (nblk > 0 && __builtin_isfinite(total)) {
        const double cd = (double)max_norm / (total + 1e-6);
        if (cd < 1.0) c = (float)cd;
    }
    rec[0] = (float)total;
    rec[1] = c * inv;
    if (c < 1.f) clipped[0] += 1;
    int streak = cnt[0];
    if (adam_step_skipped(step)) {
        streak = 0;
        if (s > min_scale) { s = fmaxf(0.5f * s, min_scale); cnt[1] += 1; }
    } else if (++streak >= growth_interval) {
        streak = 0;
        if (s < max_scale) { s = fminf(2.f * s, max_scale); cnt[2] += 1; }
    }
    cnt[0] = streak;
    state[0] = s;
    state[1] = 1.f / s;
}

// ------------------------------------------------------------------------------------------------ the update
// bias corrections as torch computes them (Python doubles): 1 - beta^t in double, then step_size / bias_correction2_sqrt
struct AdamCoef { float step_size, inv_sqrt_bc2; };
__device__ __forceinline__ AdamCoef adam_coef(int t, float lr, const float* lr_dev, float b1, float b2) {
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    const double l = lr_dev ? (double)*lr_dev : (double)lr;
    AdamCoef c;
    c.step_size = (float)(l / bc1);
    c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    return c;
}
// Overflow guard of the 16-bit modes: activation gradients are stored in f16 under a static 2^12 scale; should one
// overflow, the inf / NaN reaches a parameter gradient.  An element whose gradient is not finite is NOT applied - its parameter and
// both moments keep their values, so a non-finite value can never enter the fp32 master weights or the Adam state, also inside a
// replayed HIP graph - and counted in step[1] (FusedAdam.nonfinite_skipped() reads it).  This per-ELEMENT guard is the fallback of
// callers that do not run tri_adam_guard* first; with the guard pass a bad gradient skips the whole step (see adam_tick_kernel).
__device__ __forceinline__ void adam_note_bad(const int* step, int bad) {
    if (bad) atomicAdd(const_cast<int*>(step) + 1, bad);
}
// The gradient term of the update: g * gmul + wd * p.  CLAMP (a separate instantiation, the clip_grad_value_ rule: tri_adam_step*_clipped with a
// finite clip_value) limits the scaled gradient to [-clip_value, clip_value] BEFORE the weight decay joins it; a NaN passes through the
// clamp, so the per-element guard below still refuses it.  Without CLAMP this is the one expression the update has always evaluated.
template <bool CLAMP>
__device__ __forceinline__ float adam_grad(float g, float gmul, float clip_value, float wd, float p) {
    if constexpr (CLAMP) {
        const float t = g * gmul;
        return (t != t ? t : fminf(fmaxf(t, -clip_value), clip_value)) + wd * p;
    } else {
        return g * gmul + wd * p;
    }
}
// One kernel per reader serves tri_adam_step* and tri_adam_step*_clipped.  coef_dev (DEVICE float, NULL = 1): the clipping coefficient
// tri_grad_clip_coef left in rec[1] - read at run time, so the decision replays inside a captured HIP graph; gmul = gscale * coef is formed
// once, in fp32.  gscale * 1.0f is gscale: the unclipped entry points pass NULL and get the bits of an update that never heard of clipping.
//
// The per-element arithmetic stands twice, in the flat loop and in ADAM1 below, on purpose.  The compiler contracts g * gmul + wd * p
// differently in the two kernels - fma(wd, p, g * gmul) in the flat one, fma(gmul, g, wd * p) in the segmented one (CLAMP = false; with the
// clamp both are fma(wd, p, clamped)) - so their results differ in the last bit of a few elements when wd != 0.  Each kernel keeps the
// bits it has always produced; tests/test_gpu_adam_reader.py pins the pairs that agree.
template <bool CLAMP>
__global__ void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                                 const int* __restrict__ step, float lr, const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                 float wd, float gscale, const float* __restrict__ coef_dev, float clip_value) {
    if (adam_step_skipped(step)) return;
    const float gmul = gscale * (coef_dev ? *coef_dev : 1.f);
    const AdamCoef co = adam_coef(*step, lr, lr_dev, b1, b2);
    const float step_size = co.step_size, inv_sqrt_bc2 = co.inv_sqrt_bc2;
    int bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float pi = p[i];
        float gi = adam_grad<CLAMP>(g[i], gmul, clip_value, wd, pi);
        if (!__builtin_isfinite(gi)) { ++bad; continue; }          // overflow guard: p, m, v of that element stay (see adam_note_bad)
        float mi = b1 * m[i] + (1.f - b1) * gi;
        float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    }
    adam_note_bad(step, bad);
}
// Four elements per thread through the segment table (n4 float4s).
template <bool CLAMP>
__global__ __launch_bounds__(256) void adam_seg_kernel(float* __restrict__ p, const float* const* __restrict__ gptr,
                                                       const long* __restrict__ gstart, int nseg, float* __restrict__ m,
                                                       float* __restrict__ v, long n4, const int* __restrict__ step, float lr,
                                                       const float* __restrict__ lr_dev, float b1, float b2, float eps, float wd,
                                                       float gscale, const float* __restrict__ coef_dev, float clip_value) {
    if (adam_step_skipped(step)) return;
    const float gmul = gscale * (coef_dev ? *coef_dev : 1.f);
    const SegTable t = seg_stage(gptr, gstart, nseg);
    const AdamCoef co = adam_coef(*step, lr, lr_dev, b1, b2);
    const float step_size = co.step_size, inv_sqrt_bc2 = co.inv_sqrt_bc2;
    int bad = 0;
    for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += (long)gridDim.x * blockDim.x) {
        float4 gv;
        if (!seg_load(t, i4, gv)) continue;
        const long i = i4 * 4;
        float4 pv = *(const float4*)(p + i), mv = *(const float4*)(m + i), vv = *(const float4*)(v + i);
#define ADAM1(P, G, M, V)                                   \
    {                                                       \
        const float gi = adam_grad<CLAMP>(G, gmul, clip_value, wd, P); \
        if (__builtin_isfinite(gi)) {                       \
            M = b1 * M + (1.f - b1) * gi;                   \
            V = b2 * V + (1.f - b2) * gi * gi;              \
            P = P - step_size * M / (sqrtf(V) * inv_sqrt_bc2 + eps); \
        } else ++bad;                                       \
    }
        ADAM1(pv.x, gv.x, mv.x, vv.x) ADAM1(pv.y, gv.y, mv.y, vv.y) ADAM1(pv.z, gv.z, mv.z, vv.z) ADAM1(pv.w, gv.w, mv.w, vv.w)
#undef ADAM1
        *(float4*)(p + i) = pv; *(float4*)(m + i) = mv; *(float4*)(v + i) = vv;
    }
    adam_note_bad(step, bad);
}

// ------------------------------------------------------------------------------------------------ entry points
// what every *_segments entry point asks of its table
static int seg_args(const char* entry, const void* grad_ptrs, const long* grad_starts, int nseg, long n) {
    if (nseg >= 1 && nseg <= ADAM_MAX_SEG && n >= 0 && n % 4 == 0 && grad_ptrs && grad_starts) return TRI_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: 1..%d segments, n >= 0, n %% 4 == 0 and both tables expected", entry, ADAM_MAX_SEG);
    tri_set_error(msg);
    return TRI_ERR_ARG;
}
extern "C" int tri_adam_guard(const float* g, long n, int* step, void* stream) {
    if ((uintptr_t)g & 3) { tri_set_error("tri_adam_guard: gradient not 4-byte aligned"); return TRI_ERR_ARG; }
    grad_scan_kernel<<<scan_grid(n), 256, 0, (hipStream_t)stream>>>(FlatReader{g, n}, GuardOp{step, 0u});
    return tri_check_launch("tri_adam_guard");
}
extern "C" int tri_adam_guard_segments(const void* grad_ptrs, const long* grad_starts, int nseg, long n, int* step, void* stream) {
    if (int rc = seg_args("tri_adam_guard_segments", grad_ptrs, grad_starts, nseg, n)) return rc;
    grad_scan_kernel<<<ew_grid(n / 4), 256, 0, (hipStream_t)stream>>>(SegReader{(const float* const*)grad_ptrs, grad_starts, nseg, n / 4},
                                                                       GuardOp{step, 0u});
    return tri_check_launch("tri_adam_guard_segments");
}
extern "C" int tri_grad_norm_blocks(long n) {
    if (n < 0) { tri_set_error("tri_grad_norm_blocks: n < 0"); return TRI_ERR_ARG; }
    return scan_grid(n);
}
extern "C" int tri_grad_sumsq(const float* g, long n, double* partial, void* stream) {
    if (n < 0 || !partial || (n > 0 && !g) || ((uintptr_t)g & 3)) {
        tri_set_error("tri_grad_sumsq: n >= 0, a 4-byte aligned gradient and a partial buffer expected");
        return TRI_ERR_ARG;
    }
    grad_scan_kernel<<<scan_grid(n), 256, 0, (hipStream_t)stream>>>(FlatReader{g, n}, SumsqOp{partial, 0.0});
    return tri_check_launch("tri_grad_sumsq");
}
extern "C" int tri_grad_sumsq_segments(const void* grad_ptrs, const long* grad_starts, int nseg, long n, double* partial, void* stream) {
    if (int rc = seg_args("tri_grad_sumsq_segments", grad_ptrs, grad_starts, nseg, n)) return rc;
    if (!partial) { tri_set_error("tri_grad_sumsq_segments: a partial buffer expected"); return TRI_ERR_ARG; }
    grad_scan_kernel<<<scan_grid(n), 256, 0, (hipStream_t)stream>>>(SegReader{(const float* const*)grad_ptrs, grad_starts, nseg, n / 4},
                                                                     SumsqOp{partial, 0.0});
    return tri_check_launch("tri_grad_sumsq_segments");
}
extern "C" int tri_grad_clip_coef(const double* partial, int nblk, float gscale, float max_norm, float* rec, int* clipped, void* stream) {
    if (nblk < 0 || (nblk > 0 && !partial) || !rec || !clipped || !(max_norm > 0.f)) {
        tri_set_error("tri_grad_clip_coef: nblk >= 0, max_norm > 0 (inf measures only), rec and clipped expected");
        return TRI_ERR_ARG;
    }
    grad_clip_coef_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partial, nblk, gscale, max_norm, rec, clipped);
    return tri_check_launch("tri_grad_clip_coef");
}
// a loss scale: a power of two whose reciprocal and whose products with a coefficient stay normal numbers
static bool loss_scale_ok(float s) {
    int e;
    return s > 0.f && __builtin_isfinite(s) && frexpf(s, &e) == 0.5f && e >= -99 && e <= 101;
}
extern "C" int tri_loss_scale_step(float* state, int* cnt, const int* step, const double* partial, int nblk, float gscale, float max_norm,
                                   int growth_interval, float min_scale, float max_scale, float* rec, int* clipped, void* stream) {
    if (!state || !cnt || !step || !rec || !clipped || nblk < 0 || (nblk > 0 && !partial) || !(max_norm > 0.f) || growth_interval < 1 ||
        !loss_scale_ok(min_scale) || !loss_scale_ok(max_scale) || min_scale > max_scale) {
        tri_set_error("tri_loss_scale_step: state, cnt, step, rec and clipped, nblk >= 0, max_norm > 0 (inf: no norm clip), growth_interval >= 1 "
                      "and min_scale <= max_scale, both powers of two in [2^-100, 2^100], expected");
        return TRI_ERR_ARG;
    }
    loss_scale_step_kernel<<<1, 256, 0, (hipStream_t)stream>>>(state, cnt, step, partial, nblk, gscale, max_norm, growth_interval, min_scale,
                                                               max_scale, rec, clipped);
    return tri_check_launch("tri_loss_scale_step");
}
// An infinite clip_value is "no clamp": the CLAMP = false instantiation, which never looks at it.
extern "C" int tri_adam_step_clipped(float* p, const float* g, float* m, float* v, long n, const int* step, float lr, const float* lr_dev,
                                     float b1, float b2, float eps, float wd, float gscale, const float* coef_dev, float clip_value,
                                     void* stream) {
    if (!(clip_value > 0.f)) { tri_set_error("tri_adam_step_clipped: clip_value > 0 (inf: no clamp)"); return TRI_ERR_ARG; }
    auto kernel = __builtin_isinf(clip_value) ? adam_flat_kernel<false> : adam_flat_kernel<true>;
    kernel<<<ew_grid(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, step, lr, lr_dev, b1, b2, eps, wd, gscale, coef_dev, clip_value);
    return tri_check_launch("tri_adam_step_clipped");
}
extern "C" int tri_adam_step(float* p, const float* g, float* m, float* v, long n, const int* step, float lr, const float* lr_dev,
                             float b1, float b2, float eps, float wd, float gscale, void* stream) {
    adam_flat_kernel<false><<<ew_grid(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, step, lr, lr_dev, b1, b2, eps, wd, gscale, nullptr, INFINITY);
    return tri_check_launch("tri_adam_step");
}
extern "C" int tri_adam_step_segments_clipped(float* p, const void* grad_ptrs, const long* grad_starts, int nseg, float* m, float* v, long n,
                                              const int* step, float lr, const float* lr_dev, float b1, float b2, float eps, float wd,
                                              float gscale, const float* coef_dev, float clip_value, void* stream) {
    if (int rc = seg_args("tri_adam_step_segments_clipped", grad_ptrs, grad_starts, nseg, n)) return rc;
    if (!(clip_value > 0.f)) { tri_set_error("tri_adam_step_segments_clipped: clip_value > 0 (inf: no clamp)"); return TRI_ERR_ARG; }
    auto kernel = __builtin_isinf(clip_value) ? adam_seg_kernel<false> : adam_seg_kernel<true>;
    kernel<<<ew_grid(n / 4), 256, 0, (hipStream_t)stream>>>(p, (const float* const*)grad_ptrs, grad_starts, nseg, m, v, n / 4, step, lr, lr_dev, b1, b2,
                                                             eps, wd, gscale, coef_dev, clip_value);
    return tri_check_launch("tri_adam_step_segments_clipped");
}
extern "C" int tri_adam_step_segments(float* p, const void* grad_ptrs, const long* grad_starts, int nseg, float* m, float* v, long n,
                                      const int* step, float lr, const float* lr_dev, float b1, float b2, float eps, float wd, float gscale,
                                      void* stream) {
    if (int rc = seg_args("tri_adam_step_segments", grad_ptrs, grad_starts, nseg, n)) return rc;
    adam_seg_kernel<false><<<ew_grid(n / 4), 256, 0, (hipStream_t)stream>>>(p, (const float* const*)grad_ptrs, grad_starts, nseg, m, v, n / 4, step,
                                                                             lr, lr_dev, b1, b2, eps, wd, gscale, nullptr, INFINITY);
    return tri_check_launch("tri_adam_step_segments");
}
