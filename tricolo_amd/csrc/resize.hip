// Bicubic antialiased resize of uint8 planes (the one arithmetic step of the reference's loader, general_dataset.py:63-65:
// torchvision Resize(image_size, BICUBIC, antialias=True) on the u8 renderings = cast to fp32, ATen's _upsample_bicubic2d_aa, clamp to
// [0, 255], round half to even, cast to u8).  The interpolation is separable, width pass first:
//
//   per axis   scale = n_in / n_out, support = 2 * max(scale, 1), centre c(i) = scale * (i + 0.5),
//              window [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)),
//              tap weight w((j - c + 0.5) / max(scale, 1)) with the cubic convolution kernel at a = -0.5, normalised to sum 1 over
//              the clipped window
//
// Two kernels.  resize_tables_kernel writes, once per call and axis, the window (first tap, tap count) and the normalised fp32 weights
// of every output index into the caller's workspace, in the order of operations of ATen's weight routine (fp32 values, the "+ 0.5"
// terms in double, no contraction).  resize_kernel gives a workgroup one plane and a band of R output rows: the input rows the band
// needs are staged as u8 in LDS (16-byte loads between a scalar head and tail, so that any width and any plane offset is served),
// the width pass writes an fp32 LDS tile, the height pass reads it, clamps, rounds half to even (v_rndne_f32) and leaves the band's
// rows - one contiguous run of bytes - through LDS as 16-byte stores.  Every tap is one fmaf in tap order on fp32, no atomics: two
// calls give the same bits, and a geometry with n_in == n_out has the weights (0, 1, 0, 0) exactly, so it copies.
#include "common.h"
#include "../../include/tricolo_hip.h"

#define RS_THREADS 256
#define RS_LDS_BUDGET (64 * 1024)               // dynamic LDS a workgroup may ask for without an attribute
#define RS_BAND 16                              // output rows per workgroup when they fit the budget
#define RS_MAX_GRID_Y 32768

static inline size_t rs_align16(size_t x) { return (x + 15) & ~(size_t)15; }
static inline int rs_taps(int n_in, int n_out) {                      // ATen's max_interp_size: ceil(support) * 2 + 1
    const float scale = (float)n_in / (float)n_out;
    const float support = scale >= 1.f ? 2.f * scale : 2.f;
    return (int)ceilf(support) * 2 + 1;
}
// workspace layout: [x windows int2 Wout][x weights fp32 Wout * Kx][y windows int2 Hout][y weights fp32 Hout * Ky], 16-byte aligned parts
struct RsLayout { size_t bx, wx, by, wy, total; int Kx, Ky; };
static inline RsLayout rs_layout(int Hin, int Win, int Hout, int Wout) {
    RsLayout l;
    l.Kx = rs_taps(Win, Wout); l.Ky = rs_taps(Hin, Hout);
    l.bx = 0;
    l.wx = rs_align16(l.bx + (size_t)Wout * 8);
    l.by = rs_align16(l.wx + (size_t)Wout * l.Kx * 4);
    l.wy = rs_align16(l.by + (size_t)Hout * 8);
    l.total = rs_align16(l.wy + (size_t)Hout * l.Ky * 4);
    return l;
}

#pragma clang fp contract(off)
__device__ __forceinline__ float rs_cubic(float x) {                  // cubic convolution, a = -0.5
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
    if (x < 2.f) return ((a * x - 5.f * a) * x + 8.f * a) * x - 4.f * a;
    return 0.f;
}

__global__ __launch_bounds__(RS_THREADS) void resize_tables_kernel(int n_in, int n_out, int K, int2* __restrict__ win, float* __restrict__ wts) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n_out) return;
    const float scale = (float)n_in / (float)n_out;
    const float support = scale >= 1.f ? 2.f * scale : 2.f;
    const float invscale = scale >= 1.f ? (float)(1.0 / (double)scale) : 1.f;
    const float center = (float)((double)scale * ((double)i + 0.5));
    long lo = (long)((double)(center - support) + 0.5), hi = (long)((double)(center + support) + 0.5);
    lo = max(lo, 0L); hi = min(hi, (long)n_in);
    const int size = (int)max(0L, min(hi - lo, (long)K));
    float* w = wts + (size_t)i * K;
    float total = 0.f;
    for (int j = 0; j < size; ++j) {
        const float x = (float)(((double)((float)(j + lo) - center) + 0.5) * (double)invscale);
        w[j] = rs_cubic(x);
        total += w[j];
    }
    for (int j = 0; j < K; ++j) w[j] = (j < size && total != 0.f) ? w[j] / total : 0.f;
    win[i] = make_int2((int)lo, size);
}

// n bytes global -> LDS.  `dst` is placed by the caller so that dst and src have the same offset inside a 16-byte line.
__device__ __forceinline__ void rs_load_bytes(uint8_t* dst, const uint8_t* __restrict__ src, int n, int t) {
    const int head = min(n, (int)((16 - ((size_t)src & 15)) & 15));
    const int body = (n - head) >> 4, tail0 = head + (body << 4);
    if (t < head) dst[t] = src[t];
    for (int k = t; k < body; k += RS_THREADS) *(uint4*)(dst + head + (k << 4)) = *(const uint4*)(src + head + (k << 4));
    if (t < n - tail0) dst[tail0 + t] = src[tail0 + t];
}
__device__ __forceinline__ void rs_store_bytes(uint8_t* __restrict__ dst, const uint8_t* src, int n, int t) {
    const int head = min(n, (int)((16 - ((size_t)dst & 15)) & 15));
    const int body = (n - head) >> 4, tail0 = head + (body << 4);
    if (t < head) dst[t] = src[t];
    for (int k = t; k < body; k += RS_THREADS) *(uint4*)(dst + head + (k << 4)) = *(const uint4*)(src + head + (k << 4));
    if (t < n - tail0) dst[tail0 + t] = src[tail0 + t];
}

#pragma clang fp contract(on)
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(const uint8_t* __restrict__ in, int Hin, int Win, uint8_t* __restrict__ out, int Hout,
                                                            int Wout, const int2* __restrict__ bx, const float* __restrict__ wx, int Kx,
                                                            const int2* __restrict__ by, const float* __restrict__ wy, int Ky, int R,
                                                            int rows_cap, int io_bytes, long plane0, FastDiv div_wout) {
    extern __shared__ __align__(16) uint8_t smem[];
    // [u8 rows in / u8 rows out: io_bytes, a multiple of 16][x windows][band's y windows][fp32 width-pass tile rows_cap * Wout][x weights][band's y weights]
    uint8_t* s_io = smem;
    int2* s_bx = (int2*)(smem + io_bytes);
    int2* s_by = s_bx + Wout;
    float* s_mid = (float*)(s_by + R);
    float* s_wx = s_mid + (size_t)rows_cap * Wout;
    float* s_wy = s_wx + (size_t)Wout * Kx;

    const int t = threadIdx.x;
    const long plane = plane0 + blockIdx.y;
    const int r0 = blockIdx.x * R, nr = min(R, Hout - r0);
    const int2 first = by[r0], last = by[r0 + nr - 1];
    const int row_lo = first.x;
    // windows move forward with the row: [first's start, last's end).  The min() only guards the LDS tiles: the launcher's rs_rows_cap is an
    // upper bound of that span (two rows of slack), so it never cuts a window short.  Both passes start from tap 0 without a test: every
    // window holds at least one tap, because support >= 2 puts the sample under the centre inside [0, n_in) after clipping.
    const int nrows = min(last.x + last.y - row_lo, rows_cap);

    const uint8_t* src = in + ((size_t)plane * Hin + row_lo) * Win;
    uint8_t* s_in = s_io + ((size_t)src & 15);
    rs_load_bytes(s_in, src, nrows * Win, t);
    for (int k = t; k < Wout * Kx; k += RS_THREADS) s_wx[k] = wx[k];
    for (int k = t; k < Wout; k += RS_THREADS) s_bx[k] = bx[k];
    for (int k = t; k < nr * Ky; k += RS_THREADS) s_wy[k] = wy[(size_t)r0 * Ky + k];
    for (int k = t; k < nr; k += RS_THREADS) s_by[k] = by[r0 + k];
    __syncthreads();

    for (int e = t; e < nrows * Wout; e += RS_THREADS) {              // width pass: fp32 [nrows][Wout]
        const int r = (int)fdiv((uint32_t)e, div_wout), c = e - r * Wout;
        const int2 b = s_bx[c];
        const uint8_t* p = s_in + r * Win + b.x;
        const float* w = s_wx + c * Kx;
        float acc = (float)p[0] * w[0];
        for (int j = 1; j < b.y; ++j) acc = fmaf((float)p[j], w[j], acc);
        s_mid[e] = acc;
    }
    __syncthreads();

    uint8_t* dst = out + ((size_t)plane * Hout + r0) * Wout;
    uint8_t* s_out = s_io + ((size_t)dst & 15);                         // the staged input rows are dead from here on
    for (int e = t; e < nr * Wout; e += RS_THREADS) {                  // height pass, clamp, round half to even
        const int r = (int)fdiv((uint32_t)e, div_wout), c = e - r * Wout;
        const int2 b = s_by[r];
        const int base = min(b.x - row_lo, nrows - 1);
        const int cnt = min(b.y, nrows - base);
        const float* p = s_mid + base * Wout + c;
        const float* w = s_wy + r * Ky;
        float acc = p[0] * w[0];
        for (int j = 1; j < cnt; ++j) acc = fmaf(p[j * Wout], w[j], acc);
        s_out[e] = (uint8_t)(int)rintf(fminf(fmaxf(acc, 0.f), 255.f));
    }
    __syncthreads();
    rs_store_bytes(dst, s_out, nr * Wout, t);
}

extern "C" size_t tri_resize_bicubic_aa_workspace(int Hin, int Win, int Hout, int Wout) {
    if (Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return 0;
    return rs_layout(Hin, Win, Hout, Wout).total;
}

// rows of input a band of R output rows can reach: end(last) - start(first) < scale * (R - 1) + 2 * support + 2
static inline long rs_rows_cap(int Hin, int Hout, int R) {
    const double scale = (double)Hin / Hout, support = 2.0 * (scale >= 1.0 ? scale : 1.0);
    return min((long)Hin, (long)(scale * (R - 1) + 2.0 * support) + 3);
}

extern "C" int tri_resize_bicubic_aa_u8(const uint8_t* in, int planes, int Hin, int Win, uint8_t* out, int Hout, int Wout, void* workspace,
                                        void* stream) {
    if (planes < 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) { tri_set_error("tri_resize_bicubic_aa_u8: bad size"); return TRI_ERR_ARG; }
    if (planes == 0) return TRI_OK;
    if (!in || !out || !workspace) { tri_set_error("tri_resize_bicubic_aa_u8: null pointer"); return TRI_ERR_ARG; }
    const RsLayout l = rs_layout(Hin, Win, Hout, Wout);
    // the largest band (up to RS_BAND rows) whose tiles and tables fit the LDS budget
    int R = min(RS_BAND, Hout);
    long cap = 0, io = 0, lds = 0;
    for (; R >= 1; --R) {
        cap = rs_rows_cap(Hin, Hout, R);
        io = (long)rs_align16((size_t)max(cap * Win, (long)R * Wout) + 16);
        lds = io + cap * Wout * 4 + (long)Wout * l.Kx * 4 + (long)Wout * 8 + (long)R * l.Ky * 4 + (long)R * 8;
        if (lds <= RS_LDS_BUDGET) break;
    }
    if (R < 1 || cap * Wout >= (1L << 31)) {
        tri_set_error("tri_resize_bicubic_aa_u8: one output row's window and the weight tables do not fit in 64 KiB of LDS");
        return TRI_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int2* bx = (int2*)(ws + l.bx); float* wx = (float*)(ws + l.wx);
    int2* by = (int2*)(ws + l.by); float* wy = (float*)(ws + l.wy);
    resize_tables_kernel<<<(Wout + RS_THREADS - 1) / RS_THREADS, RS_THREADS, 0, st>>>(Win, Wout, l.Kx, bx, wx);
    resize_tables_kernel<<<(Hout + RS_THREADS - 1) / RS_THREADS, RS_THREADS, 0, st>>>(Hin, Hout, l.Ky, by, wy);
    const unsigned bands = (unsigned)((Hout + R - 1) / R);
    const FastDiv dw = make_fastdiv((uint32_t)Wout);
    for (long p0 = 0; p0 < planes; p0 += RS_MAX_GRID_Y)
        resize_kernel<<<dim3(bands, (unsigned)min((long)RS_MAX_GRID_Y, planes - p0)), RS_THREADS, (size_t)lds, st>>>(
            in, Hin, Win, out, Hout, Wout, bx, wx, l.Kx, by, wy, l.Ky, R, (int)cap, (int)io, p0, dw);
    return tri_check_launch("tri_resize_bicubic_aa_u8");
}
