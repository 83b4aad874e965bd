// Fused NT-Xent / InfoNCE loss, forward + backward, for gfx950.
//
// Replaces the ~15 torch launches per modality pair of /root/reference/tricolo/loss/nt_xent.py:55-74
// (2x normalize, eye, 2x matmul, 2x div, 2x log_softmax, 2x mul/sum, axpy) and their autograd graph with five
// small launches: row-normalise, S = a_hat b_hat^T / T in exact fp32 FMAs (the matrix is tiny, parity matters more
// than MFMA here), row/column log-sum-exp with wave shuffles, the loss sums, and the gradient
// dS = [alpha (softmax_row - I) + (1 - alpha)(softmax_col - I)] / B  contracted on the fly with the other modality
// and pushed through the normalise Jacobian - S^T is never materialised or recomputed.
//
// One kernel set over NtxMulti, the modality / pair index a grid dimension: the all-pairs calls run M = 2 or 3 modalities,
// the single-pair calls (tri_ntxent_fwd_bwd, tri_ntxent_bwd) are its M = 2 case with one pair.
#include <stdio.h>
#include "common.h"
#include "../../include/tricolo_hip.h"

// The learnable temperature (CLIP's logit scale): s = clamp(*logit_scale, 0, max_logit_scale), 1 / T = exp(s).  Every kernel that scales
// by 1 / T reads the DEVICE scalar when the pointer is set, so a captured step follows the parameter from replay to replay; with a NULL
// pointer the host's 1 / temperature is used as before.  (The comparisons keep a NaN, as torch.clamp does.)
__device__ __forceinline__ float ntx_inv_T_of(float s, float max_logit_scale) {
    return expf(s < 0.f ? 0.f : (s > max_logit_scale ? max_logit_scale : s));
}

// S[i][j] = <a_i, b_j> * inv_T ; 64x64 tile per block, 4x4 outputs per thread, K chunks of 16.  The single-pair calls' similarity
// outside the row kernel's range (B > 512 or D % 4 != 0); the all-pairs calls refuse that range, so it has no pair dimension.
__global__ __launch_bounds__(256) void ntx_sim_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int D, float inv_T,
                                                      const float* __restrict__ logit_scale, float max_logit_scale, float* __restrict__ S) {
    __shared__ float sa[16][65], sb[16][65];
    if (logit_scale) inv_T = ntx_inv_T_of(*logit_scale, max_logit_scale);
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < D; k0 += 16) {
        for (int e = t; e < 64 * 16; e += 256) {
            int r = e >> 4, k = e & 15;
            sa[k][r] = (i0 + r < B && k0 + k < D) ? a[(long)(i0 + r) * D + k0 + k] : 0.f;
            sb[k][r] = (j0 + r < B && k0 + k < D) ? b[(long)(j0 + r) * D + k0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = sa[k][ty * 4 + u]; bv[u] = sb[k][tx * 4 + u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int w = 0; w < 4; ++w) acc[u][w] = fmaf(av[u], bv[w], acc[u][w]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            int i = i0 + ty * 4 + u, j = j0 + tx * 4 + w;
            if (i < B && j < B) S[(long)i * B + j] = acc[u][w] * inv_T;
        }
}

// TriCoLoNet._calculate_losses (tricolo_net.py:56-63) evaluates the loss for every pair of modalities and sums them: per pair
// five launches here (fifteen in the reference), plus the additions, plus autograd's accumulation of the two gradients every
// embedding receives - ~25 launches of ~5 us each, in series, with all three towers waiting.  The multi form does the same
// arithmetic for M = 2 or 3 modalities in FOUR launches forward and ONE backward: every modality is normalised once, the
// pair index is a grid dimension, the total is formed by the loss-sum kernel in the reference's order ((l0 + l1) + l2 in
// fp32), and the gradient kernel sums an embedding's contributions from its pairs before the normalise Jacobian (linear).
#define NTX_MAX_MOD 3
struct NtxMulti {
    const float* z[NTX_MAX_MOD];
    float* zhat[NTX_MAX_MOD];
    float* nrm[NTX_MAX_MOD];
    float* S[NTX_MAX_MOD];               // per pair
    float* lse_row[NTX_MAX_MOD];
    float* lse_col[NTX_MAX_MOD];
    float* rowloss[NTX_MAX_MOD];
    const float* dpair[NTX_MAX_MOD];     // backward: upstream gradient of each pair's loss (device scalars, may be NULL)
    const float* dtotal;                 //           ... and of the total (NULL: up0)
    float* dz[NTX_MAX_MOD];
    int pa[NTX_MAX_MOD], pb[NTX_MAX_MOD];
    int M, P, B, D, norm;
    float inv_T, alpha, eps;
    float up0;                           // host-set upstream of the total when dtotal is NULL: 0, or 1 for a single-pair call without dloss
    const float* logit_scale;            // learnable temperature (device scalar; NULL: the fixed inv_T above)
    float max_logit_scale;
    float* rowdls[NTX_MAX_MOD];          // backward, per pair: [B] row partials of d loss / d logit_scale
    float* dlogit_scale;                 //           ... and their gated sum (device scalar, written)
};

__device__ __forceinline__ float ntx_inv_T(const NtxMulti& p) { return p.logit_scale ? ntx_inv_T_of(*p.logit_scale, p.max_logit_scale) : p.inv_T; }

__global__ void ntxm_l2norm_kernel(const NtxMulti p) {
    const int m = blockIdx.y;
    int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.B) return;
    const float* x = p.z[m] + (long)row * p.D;
    float s = 0.f;
#pragma unroll 8                                                   // (rolled loops wait out one load round trip per step: misc.hip l2norm kernels)
    for (int i = lane; i < p.D; i += 64) s += x[i] * x[i];
    s = wave_sum(s);
    float nrm = sqrtf(s);
    float inv = 1.0f / fmaxf(nrm, p.eps);
#pragma unroll 8
    for (int i = lane; i < p.D; i += 64) p.zhat[m][(long)row * p.D + i] = x[i] * inv;
    if (lane == 0) p.nrm[m][row] = nrm;
}

// Small batches (the per-GPU batch of the training step): the 64x64 tiling above would run on one or a handful of CUs.
// Block (row i, pair q) keeps a_i in LDS; each wave takes columns j = wave, wave + 4, ... four at a time (16-byte loads of
// b_j along D, 8 independent loads in flight), reduces with wave shuffles.  D % 4 == 0.
__global__ __launch_bounds__(256) void ntxm_sim_rows_kernel(const NtxMulti p) {
    extern __shared__ float sa[];
    const int i = blockIdx.x, q = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int B = p.B, D = p.D;
    const float* a = p.norm ? p.zhat[p.pa[q]] : p.z[p.pa[q]];
    const float* b = p.norm ? p.zhat[p.pb[q]] : p.z[p.pb[q]];
    float* S = p.S[q];
    const float inv_T = ntx_inv_T(p);
    for (int k = t * 4; k < D; k += 1024) *(float4*)(sa + k) = *(const float4*)(a + (long)i * D + k);
    __syncthreads();
    for (int jb = wave * 4; jb < B; jb += 16) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = lane * 4; k < D; k += 256) {
            const float4 av = *(const float4*)(sa + k);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = jb + u < B ? jb + u : B - 1;
                const float4 bv = *(const float4*)(b + (long)j * D + k);
                acc[u] = fmaf(av.x, bv.x, fmaf(av.y, bv.y, fmaf(av.z, bv.z, fmaf(av.w, bv.w, acc[u]))));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = wave_sum(acc[u]);
            if (lane == 0 && jb + u < B) S[(long)i * B + jb + u] = v * inv_T;
        }
    }
}

// block (index i, pair q): lse over row i and over column i of S_q, and that row's loss contribution
__global__ __launch_bounds__(256) void ntxm_lse_kernel(const NtxMulti p) {
    __shared__ float sh[4];
    const int i = blockIdx.x, q = blockIdx.y, t = threadIdx.x, B = p.B;
    const float* S = p.S[q];
    float mr = -INFINITY, mc = -INFINITY;
    for (int j = t; j < B; j += 256) { mr = fmaxf(mr, S[(long)i * B + j]); mc = fmaxf(mc, S[(long)j * B + i]); }
    mr = block_max(mr, sh);
    mc = block_max(mc, sh);
    float sr = 0.f, sc = 0.f;
    for (int j = t; j < B; j += 256) { sr += expf(S[(long)i * B + j] - mr); sc += expf(S[(long)j * B + i] - mc); }
    sr = block_sum(sr, sh);
    sc = block_sum(sc, sh);
    if (t == 0) {
        float lr = mr + logf(sr), lc = mc + logf(sc), d = S[(long)i * B + i];
        p.lse_row[q][i] = lr;
        p.lse_col[q][i] = lc;
        p.rowloss[q][i] = -(p.alpha * (d - lr) + (1.f - p.alpha) * (d - lc)) / (float)B;
    }
}

// one wave per pair sums its row losses (double, fixed order per lane + shuffle tree: reproducible); thread 0 forms the total
// (write_total = 0: `losses` holds the pair losses only - the single-pair calls' one float)
__global__ void ntxm_loss_sum_kernel(const NtxMulti p, float* __restrict__ losses, int write_total) {
    __shared__ float lp[NTX_MAX_MOD];
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (q < p.P) {
        double s = 0.0;
        for (int i = lane; i < p.B; i += 64) s += (double)p.rowloss[q][i];
        s = wave_sum_d(s);
        if (lane == 0) { lp[q] = (float)s; losses[q] = (float)s; }
    }
    __syncthreads();
    if (threadIdx.x == 0 && write_total) {
        float tot = 0.f;                                           // Python's sum(): ((0 + l0) + l1) + l2 in fp32
        for (int q2 = 0; q2 < p.P; ++q2) tot += lp[q2];
        losses[p.P] = tot;
    }
}

// block (row i, modality m): d z_m[i] summed over the pairs m takes part in.  With a learnable temperature the alpha-side block of a
// pair - the one block that visits row i of S_q - also leaves row i's share of up_q sum_ij G_ij S_ij in rowdls[q][i] (G = d loss_q / d S_q,
// the coefficients below before their 1 / T): d loss / d logit_scale is the sum over q, i of those, because S = exp(s) C and
// d exp(s) / d s = exp(s).  The share is taken as (alpha softmax_row_ij (S_ij - S_ii) + (1 - alpha) softmax_col_ij (S_ij - S_jj)) / B summed over
// j, which sums to the same thing (a softmax row, or column, adds up to 1) without the cancellation of (softmax_ii - 1) S_ii against
// the off-diagonal terms: a rounding of the log-sum-exp then costs a relative error of the terms, not an absolute one of S_ii.
__global__ __launch_bounds__(256) void ntxm_grad_kernel(const NtxMulti p) {
    extern __shared__ float w[];                 // [np][B] coefficients dS_ij (alpha side) or dS_ji, times 1/T, of this modality's np <= 2 pairs
    __shared__ float sh[4];
    const int i = blockIdx.x, m = blockIdx.y, t = threadIdx.x, B = p.B, D = p.D;
    const float* other[2] = {nullptr, nullptr};
    int np = 0;
    const float gt = p.dtotal ? *p.dtotal : p.up0;
    const float inv_T = ntx_inv_T(p);
    for (int q = 0; q < p.P; ++q) {
        const int side = p.pa[q] == m ? 0 : (p.pb[q] == m ? 1 : -1);
        if (side < 0) continue;
        const float up = gt + (p.dpair[q] ? *p.dpair[q] : 0.f);
        const float invB = up / (float)B;         // upstream d(total)/d(loss) folded into the coefficients
        const float* S = p.S[q];
        const float* lr = p.lse_row[q];
        const float* lc = p.lse_col[q];
        const bool want_dls = p.dlogit_scale && side == 0;              // (block-uniform)
        const float sii = want_dls ? S[(long)i * B + i] : 0.f;
        float gs = 0.f;
        for (int j = t; j < B; j += 256) {
            float s, pr, pc;
            if (side == 0) { s = S[(long)i * B + j]; pr = expf(s - lr[i]); pc = expf(s - lc[j]); }
            else           { s = S[(long)j * B + i]; pr = expf(s - lr[j]); pc = expf(s - lc[i]); }
            float delta = (i == j) ? 1.f : 0.f;
            w[np * B + j] = (p.alpha * (pr - delta) + (1.f - p.alpha) * (pc - delta)) * invB * inv_T;
            if (want_dls) gs += p.alpha * pr * (s - sii) + (1.f - p.alpha) * pc * (s - S[(long)j * B + j]);
        }
        if (want_dls) {                            // (sh is free again when block_sum returns)
            gs = block_sum(gs, sh);
            if (t == 0) p.rowdls[q][i] = gs * invB;
        }
        const int o = side == 0 ? p.pb[q] : p.pa[q];
        other[np] = p.norm ? p.zhat[o] : p.z[o];
        ++np;
    }
    __syncthreads();
    const float* self = p.norm ? p.zhat[m] : p.z[m];
    float dot = 0.f;
    float g[8];                                  // D <= 2048; fixed unroll keeps g[] in registers
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int c = t + q * 256;
        g[q] = 0.f;
        if (c < D) {
            float tot = 0.f;
            for (int k = 0; k < np; ++k) {       // pair by pair, then summed: with one pair tot = 0.f + acc
                float acc = 0.f;
                const float* ot = other[k];
                const float* wk = w + k * B;
#pragma unroll 8                                                   // (same summation order; eight loads in flight instead of one)
                for (int j = 0; j < B; ++j) acc = fmaf(wk[j], ot[(long)j * D + c], acc);
                tot += acc;
            }
            g[q] = tot;
            dot += tot * self[(long)i * D + c];
        }
    }
    float inv = 1.0f;
    if (p.norm) {
        dot = block_sum(dot, sh);
        inv = 1.0f / fmaxf(p.nrm[m][i], p.eps);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int c = t + q * 256;
        if (c < D) p.dz[m][(long)i * D + c] = p.norm ? (g[q] - self[(long)i * D + c] * dot) * inv : g[q];
    }
}

// one wave per pair sums its row partials (double, fixed order per lane + shuffle tree, as ntxm_loss_sum_kernel); thread 0 adds the pairs
// in order and gates the sum with the clamp: inside [0, max] (boundaries included, as torch.clamp's backward) it passes, outside it is 0
__global__ void ntxm_dls_sum_kernel(const NtxMulti p) {
    __shared__ double dp[NTX_MAX_MOD];
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (q < p.P) {
        double s = 0.0;
        for (int i = lane; i < p.B; i += 64) s += (double)p.rowdls[q][i];
        s = wave_sum_d(s);
        if (lane == 0) dp[q] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int q2 = 0; q2 < p.P; ++q2) tot += dp[q2];
        const float s0 = *p.logit_scale;
        *p.dlogit_scale = (s0 >= 0.f && s0 <= p.max_logit_scale) ? (float)tot : 0.0f;
    }
}

static size_t ntx_workspace(int M, int B, int D) {
    const int P = M * (M - 1) / 2;
    return (size_t)M * (al256((size_t)B * D * 4) + al256((size_t)B * 4)) + (size_t)P * (3 * al256((size_t)B * 4) + al256((size_t)B * B * 4));
}

// learnable temperature: the same layout, then the [P][B] row partials of d loss / d logit_scale
static size_t ntx_ls_workspace(int M, int B, int D) { return ntx_workspace(M, B, D) + (size_t)(M * (M - 1) / 2) * al256((size_t)B * 4); }

// the temperature of a call: the fixed float, or (ls) the device scalar and its clamp
struct NtxTemp {
    float temperature;
    const float* logit_scale;
    float max_logit_scale;
    bool ls;
};

// multi: the fused range of the all-pairs forms (the row similarity kernel's); the single-pair forms take any 1 <= D <= 2048 and B up to 8192
static int ntx_setup(NtxMulti& p, const float* const* z, int M, int B, int D, const NtxTemp& T, float alpha, int norm, void* workspace,
                     size_t workspace_bytes, bool multi) {
    const char* who = multi ? "tri_ntxent_multi" : "tri_ntxent";
    char msg[160];
    if (M < 2 || M > NTX_MAX_MOD) { tri_set_error("tri_ntxent_multi: 2 or 3 modalities"); return TRI_ERR_ARG; }
    if (multi ? (B < 1 || B > 512 || D < 4 || D > 2048 || D % 4) : (B < 1 || B > 8192 || D < 1 || D > 2048)) {
        tri_set_error(multi ? "tri_ntxent_multi: need 1<=B<=512, 4<=D<=2048, D%4==0 (else use tri_ntxent_fwd_bwd per pair)"
                            : "tri_ntxent: need 1<=B<=8192, 1<=D<=2048");
        return multi ? TRI_ERR_UNSUPPORTED : TRI_ERR_ARG;
    }
    if (T.ls && !T.logit_scale) { snprintf(msg, sizeof(msg), "%s: logit_scale is NULL", who); tri_set_error(msg); return TRI_ERR_ARG; }
    if (T.ls && !(T.max_logit_scale >= 0.f && T.max_logit_scale <= 3.0e38f)) {
        snprintf(msg, sizeof(msg), "%s: max_logit_scale must be finite and >= 0", who); tri_set_error(msg); return TRI_ERR_ARG;
    }
    if (!z || !workspace || workspace_bytes < (T.ls ? ntx_ls_workspace(M, B, D) : ntx_workspace(M, B, D))) { snprintf(msg, sizeof(msg), "%s: workspace too small", who); tri_set_error(msg); return TRI_ERR_ARG; }
    p.M = M; p.P = M * (M - 1) / 2; p.B = B; p.D = D; p.norm = norm; p.alpha = alpha;
    if (T.ls) { p.logit_scale = T.logit_scale; p.max_logit_scale = T.max_logit_scale; }
    else p.inv_T = 1.0f / T.temperature;
    p.eps = 1e-12f;                                // F.normalize default (nt_xent.py:56-57)
    char* w = (char*)workspace;
    for (int m = 0; m < M; ++m) {
        if (!z[m]) { snprintf(msg, sizeof(msg), "%s: NULL embedding", who); tri_set_error(msg); return TRI_ERR_ARG; }
        p.z[m] = z[m];
        p.zhat[m] = (float*)w; w += al256((size_t)B * D * 4);
        p.nrm[m] = (float*)w; w += al256((size_t)B * 4);
    }
    int q = 0;
    for (int a = 0; a < M; ++a)                    // itertools.combinations order: the earlier modality is the alpha side
        for (int b = a + 1; b < M; ++b, ++q) {
            p.pa[q] = a; p.pb[q] = b;
            p.lse_row[q] = (float*)w; w += al256((size_t)B * 4);
            p.lse_col[q] = (float*)w; w += al256((size_t)B * 4);
            p.rowloss[q] = (float*)w; w += al256((size_t)B * 4);
            p.S[q] = (float*)w; w += al256((size_t)B * B * 4);
        }
    if (T.ls)
        for (q = 0; q < p.P; ++q) { p.rowdls[q] = (float*)w; w += al256((size_t)B * 4); }
    return 0;
}

// norm == 0: no normalise launch, the kernels read z, and zhat / nrm are never touched
static int ntx_forward(const NtxMulti& p, float* losses, int write_total, hipStream_t s, const char* who) {
    const int B = p.B, D = p.D;
    if (p.norm) ntxm_l2norm_kernel<<<dim3((B + 3) / 4, p.M), 256, 0, s>>>(p);
    if (B <= 512 && D % 4 == 0) ntxm_sim_rows_kernel<<<dim3(B, p.P), 256, (size_t)D * sizeof(float), s>>>(p);
    else ntx_sim_kernel<<<dim3((B + 63) / 64, (B + 63) / 64), 256, 0, s>>>(p.norm ? p.zhat[0] : p.z[0], p.norm ? p.zhat[1] : p.z[1], B, D, p.inv_T,
                                                                                 p.logit_scale, p.max_logit_scale, p.S[0]);
    ntxm_lse_kernel<<<dim3(B, p.P), 256, 0, s>>>(p);
    ntxm_loss_sum_kernel<<<1, 64 * NTX_MAX_MOD, 0, s>>>(p, losses, write_total);
    return tri_check_launch(who);
}

static int ntx_backward(const NtxMulti& p, hipStream_t s, const char* who) {
    const int np = p.M == 3 ? 2 : 1;               // pairs per modality: at B = 8192 one pair's coefficients are 32 KiB of the 64 KiB a launch gets
    ntxm_grad_kernel<<<dim3(p.B, p.M), 256, (size_t)np * p.B * sizeof(float), s>>>(p);
    if (p.dlogit_scale) ntxm_dls_sum_kernel<<<1, 64 * NTX_MAX_MOD, 0, s>>>(p);
    return tri_check_launch(who);
}

extern "C" size_t tri_ntxent_workspace(int B, int D) { return ntx_workspace(2, B, D); }
extern "C" size_t tri_ntxent_multi_workspace(int M, int B, int D) { return ntx_workspace(M, B, D); }
extern "C" size_t tri_ntxent_ls_workspace(int M, int B, int D) { return ntx_ls_workspace(M, B, D); }

static NtxTemp ntx_fixed(float temperature) { return NtxTemp{temperature, nullptr, 0.f, false}; }
static NtxTemp ntx_learned(const float* logit_scale, float max_logit_scale) { return NtxTemp{0.f, logit_scale, max_logit_scale, true}; }

// a backward call with a learnable temperature needs somewhere to write its gradient
static int ntx_want_dls(NtxMulti& p, const NtxTemp& T, float* dlogit_scale, const char* who) {
    if (!T.ls) return 0;
    if (!dlogit_scale) { char msg[96]; snprintf(msg, sizeof(msg), "%s: dlogit_scale is NULL", who); tri_set_error(msg); return TRI_ERR_ARG; }
    p.dlogit_scale = dlogit_scale;
    return 0;
}

static int ntx_fwd_bwd(const float* za, const float* zb, int B, int D, const NtxTemp& T, float alpha, int norm, float* loss, float* dza, float* dzb,
                       float* dlogit_scale, void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    NtxMulti p{};
    const float* z[2] = {za, zb};
    int rc = ntx_setup(p, z, 2, B, D, T, alpha, norm, workspace, workspace_bytes, false);
    if (rc) return rc;
    char msg[96];
    if (!loss) { snprintf(msg, sizeof(msg), "%s: loss is NULL", who); tri_set_error(msg); return TRI_ERR_ARG; }
    if (dza && dzb && (rc = ntx_want_dls(p, T, dlogit_scale, who))) return rc;
    rc = ntx_forward(p, loss, 0, (hipStream_t)stream, who);
    if (rc || !dza || !dzb) return rc;
    p.dz[0] = dza; p.dz[1] = dzb;
    p.up0 = 1.0f;
    return ntx_backward(p, (hipStream_t)stream, who);
}

static int ntx_bwd(const float* za, const float* zb, int B, int D, const NtxTemp& T, float alpha, int norm, const float* dloss, float* dza, float* dzb,
                   float* dlogit_scale, const void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    NtxMulti p{};
    const float* z[2] = {za, zb};
    int rc = ntx_setup(p, z, 2, B, D, T, alpha, norm, (void*)workspace, workspace_bytes, false);
    if (rc) return rc;
    char msg[96];
    if (!dza || !dzb) { snprintf(msg, sizeof(msg), "%s: NULL gradient buffer", who); tri_set_error(msg); return TRI_ERR_ARG; }
    if ((rc = ntx_want_dls(p, T, dlogit_scale, who))) return rc;
    p.dz[0] = dza; p.dz[1] = dzb;
    p.dpair[0] = dloss;
    p.up0 = dloss ? 0.f : 1.0f;
    return ntx_backward(p, (hipStream_t)stream, who);
}

static int ntx_multi_fwd(const float* const* z, int M, int B, int D, const NtxTemp& T, float alpha, int norm, float* losses, void* workspace,
                         size_t workspace_bytes, void* stream, const char* who) {
    NtxMulti p{};
    int rc = ntx_setup(p, z, M, B, D, T, alpha, norm, workspace, workspace_bytes, true);
    if (rc) return rc;
    return ntx_forward(p, losses, 1, (hipStream_t)stream, who);
}

static int ntx_multi_bwd(const float* const* z, int M, int B, int D, const NtxTemp& T, float alpha, int norm, const float* const* dpair,
                         const float* dtotal, float* const* dz, float* dlogit_scale, const void* workspace, size_t workspace_bytes, void* stream,
                         const char* who) {
    NtxMulti p{};
    int rc = ntx_setup(p, z, M, B, D, T, alpha, norm, (void*)workspace, workspace_bytes, true);
    if (rc) return rc;
    char msg[96];
    if (!dz) { snprintf(msg, sizeof(msg), "%s: dz is NULL", who); tri_set_error(msg); return TRI_ERR_ARG; }
    for (int m = 0; m < M; ++m) {
        if (!dz[m]) { snprintf(msg, sizeof(msg), "%s: NULL gradient buffer", who); tri_set_error(msg); return TRI_ERR_ARG; }
        p.dz[m] = dz[m];
    }
    if ((rc = ntx_want_dls(p, T, dlogit_scale, who))) return rc;
    for (int q = 0; q < p.P; ++q) p.dpair[q] = dpair ? dpair[q] : nullptr;
    p.dtotal = dtotal;
    return ntx_backward(p, (hipStream_t)stream, who);
}

// loss (device scalar) = alpha * CE_rows(S) + (1 - alpha) * CE_cols(S),  S = norm(za) norm(zb)^T / T; dza / dzb (optional, both or
// neither) receive d loss / d za, d loss / d zb.  zis -> za, zjs -> zb in the reference's argument order (alpha is asymmetric).
extern "C" int tri_ntxent_fwd_bwd(const float* za, const float* zb, int B, int D, float temperature, float alpha, int norm,
                                  float* loss, float* dza, float* dzb, void* workspace, size_t workspace_bytes, void* stream) {
    return ntx_fwd_bwd(za, zb, B, D, ntx_fixed(temperature), alpha, norm, loss, dza, dzb, nullptr, workspace, workspace_bytes, stream, "tri_ntxent_fwd_bwd");
}

// The gradient half on its own, for a `workspace` that a tri_ntxent_fwd_bwd(..., dza = dzb = NULL, ...) call filled: dza / dzb =
// (*dloss) * d loss / d za, zb (dloss NULL: exactly 1).  Lets autograd's backward launch ONE kernel per pair with the upstream
// scalar folded in (no elementwise `grad * dloss` passes).
extern "C" int tri_ntxent_bwd(const float* za, const float* zb, int B, int D, float temperature, float alpha, int norm,
                              const float* dloss, float* dza, float* dzb, const void* workspace, size_t workspace_bytes, void* stream) {
    return ntx_bwd(za, zb, B, D, ntx_fixed(temperature), alpha, norm, dloss, dza, dzb, nullptr, workspace, workspace_bytes, stream, "tri_ntxent_bwd");
}

// losses [P + 1] (device): the pair losses in combination order ((0,1), (0,2), (1,2)), then their sum
extern "C" int tri_ntxent_multi_fwd(const float* const* z, int M, int B, int D, float temperature, float alpha, int norm, float* losses,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return ntx_multi_fwd(z, M, B, D, ntx_fixed(temperature), alpha, norm, losses, workspace, workspace_bytes, stream, "tri_ntxent_multi_fwd");
}

// dz[m] = sum over the pairs of m of (dtotal + dpair[pair]) * d loss_pair / d z_m, from the workspace the forward call filled
extern "C" int tri_ntxent_multi_bwd(const float* const* z, int M, int B, int D, float temperature, float alpha, int norm,
                                    const float* const* dpair, const float* dtotal, float* const* dz, const void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return ntx_multi_bwd(z, M, B, D, ntx_fixed(temperature), alpha, norm, dpair, dtotal, dz, nullptr, workspace, workspace_bytes, stream,
                         "tri_ntxent_multi_bwd");
}

// The same four calls with a learnable temperature: 1 / T = exp(clamp(*logit_scale, 0, max_logit_scale)), read on the device by every
// kernel; the backward forms WRITE d / d logit_scale (upstreams folded in, 0 outside the clamp) to the device scalar dlogit_scale with one
// launch more.  Workspace: tri_ntxent_ls_workspace(M, B, D), M = 2 for the single-pair calls.
extern "C" int tri_ntxent_ls_fwd_bwd(const float* za, const float* zb, int B, int D, const float* logit_scale, float max_logit_scale, float alpha,
                                     int norm, float* loss, float* dza, float* dzb, float* dlogit_scale, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return ntx_fwd_bwd(za, zb, B, D, ntx_learned(logit_scale, max_logit_scale), alpha, norm, loss, dza, dzb, dlogit_scale, workspace, workspace_bytes,
                       stream, "tri_ntxent_ls_fwd_bwd");
}

extern "C" int tri_ntxent_ls_bwd(const float* za, const float* zb, int B, int D, const float* logit_scale, float max_logit_scale, float alpha, int norm,
                                 const float* dloss, float* dza, float* dzb, float* dlogit_scale, const void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return ntx_bwd(za, zb, B, D, ntx_learned(logit_scale, max_logit_scale), alpha, norm, dloss, dza, dzb, dlogit_scale, workspace, workspace_bytes, stream,
                   "tri_ntxent_ls_bwd");
}

extern "C" int tri_ntxent_multi_ls_fwd(const float* const* z, int M, int B, int D, const float* logit_scale, float max_logit_scale, float alpha,
                                       int norm, float* losses, void* workspace, size_t workspace_bytes, void* stream) {
    return ntx_multi_fwd(z, M, B, D, ntx_learned(logit_scale, max_logit_scale), alpha, norm, losses, workspace, workspace_bytes, stream,
                         "tri_ntxent_multi_ls_fwd");
}

extern "C" int tri_ntxent_multi_ls_bwd(const float* const* z, int M, int B, int D, const float* logit_scale, float max_logit_scale, float alpha,
                                       int norm, const float* const* dpair, const float* dtotal, float* const* dz, float* dlogit_scale,
                                       const void* workspace, size_t workspace_bytes, void* stream) {
    return ntx_multi_bwd(z, M, B, D, ntx_learned(logit_scale, max_logit_scale), alpha, norm, dpair, dtotal, dz, dlogit_scale, workspace,
                         workspace_bytes, stream, "tri_ntxent_multi_ls_bwd");
}
