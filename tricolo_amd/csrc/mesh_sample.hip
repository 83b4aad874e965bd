// Surface samples of triangle meshes (the front half of the reference's calculate_f1.py: pytorch3d's Meshes.get_bounding_boxes,
// scale_verts and sample_points_from_meshes): per-mesh bounding boxes, the float64 CDF of the fp32 face areas, and S area-weighted
// points per mesh from a counter-based generator - all on the packed batch of N meshes that mesh_batch.h lays out (without materials).
//
//   area[f]  = 0.5 * |(b - a) x (c - a)|, fp32, on the scaled vertices fl32(v * scale[n]); every operation rounded on its own
//              (contraction is off in this file: with an fma the cross product of a face with b == c would be a rounding error
//              instead of exactly 0, and the torch fallback could not form the same bits)
//   cdf[f]   = fl(cb + fl(wb + fl(lb + loc))), float64: `loc` the running sum of the MS_K faces one lane owns, lb / wb / cb the
//              value the lane / wave / chunk before it ended on, each carried forward by ONE serial chain of its level.  Every base
//              is exactly the final value of the element before it, so the CDF never decreases and a face of area 0 repeats its
//              predecessor's value bit for bit - such a face can never be the upper bound of anything.  The chunk is fixed
//              (MS_CHUNK faces from the mesh's first face), so the bits depend on the mesh alone: not on the grid, not on the batch.
//   sample   = Philox4x32-10(key = seed, counter = (s, n, 0, 0)) -> u_f, u1, u2 (24 bits each); face = the smallest f with
//              cdf[f] > u_f * total (float64); point = (1 - r) a + r (1 - u2) b + r u2 c with r = sqrtf(u1), fp32.
// No floating-point atomics anywhere; two runs give the same bits.
#include "mesh_batch.h"
#include "../../include/tricolo_hip.h"

#pragma clang fp contract(off)

#define MS_THREADS 256
#define MS_K 8                                  // consecutive faces per lane of the scan
#define MS_CHUNK (MS_THREADS * MS_K)            // 2,048 faces per chunk - part of the definition of the CDF's bits, never tuned per grid
#define MS_SPT 4                                // samples per thread of the sampler
#define MS_TILE (MS_THREADS * MS_SPT)           // 1,024 samples per workgroup
#define MS_COARSE 2048                          // coarse CDF entries staged in LDS (16 KiB)
#define MS_MAX_BLOCKS (1 << 23)
#define MS_MAX_GRID_Y 32768

// ---- bounding boxes: one workgroup per mesh -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_THREADS) void mesh_bbox_kernel(const float* __restrict__ verts, const long* __restrict__ vert_off, long n0,
                                                               float* __restrict__ bbox) {
    __shared__ float red[4][6];
    const long n = n0 + blockIdx.x;
    const long v0 = vert_off[n], V = vert_off[n + 1] - v0;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long i = t; i < V; i += MS_THREADS) {
        const float* p = verts + (size_t)(v0 + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], p[c]); hi[c] = fmaxf(hi[c], p[c]); }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
        if (lane == 0) { red[wave][c * 2] = lo[c]; red[wave][c * 2 + 1] = hi[c]; }
    }
    __syncthreads();
    if (t < 6) {
        const float a = red[0][t], b = red[1][t], c = red[2][t], d = red[3][t];
        const float r = (t & 1) ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : fminf(fminf(a, b), fminf(c, d));
        bbox[(size_t)n * 6 + t] = V > 0 ? r : 0.f;                      // a mesh without vertices: a zero box
    }
}

extern "C" size_t tri_mesh_batch_size(void) { return sizeof(TriMeshBatch); }

extern "C" int tri_mesh_bbox(const TriMeshBatch* batch, float* bbox, void* stream) {
    MeshBatch m;
    const int bad = mb_from_abi(batch, "tri_mesh_bbox", 0, &m);
    if (bad != TRI_OK) return bad;
    for (long n0 = 0; n0 < m.N; n0 += MS_MAX_BLOCKS)
        mesh_bbox_kernel<<<(unsigned)min((long)MS_MAX_BLOCKS, m.N - n0), MS_THREADS, 0, (hipStream_t)stream>>>(m.verts, m.vert_off, n0, bbox);
    return tri_check_launch("tri_mesh_bbox");
}

// ---- face areas + CDF -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_scaled(const MeshBatch& m, long v0, long V, int i, float s, float* o) {
    const float* p = mb_vertex(m, v0, V, i);
    o[0] = p[0] * s; o[1] = p[1] * s; o[2] = p[2] * s;
}

__device__ __forceinline__ float face_area(const MeshBatch& m, long v0, long V, long f, float s) {
    if (V <= 0) return 0.f;
    const int* fi = m.faces + (size_t)f * 3;
    float a[3], b[3], c[3], x[3];
    load_scaled(m, v0, V, fi[0], s, a);
    load_scaled(m, v0, V, fi[1], s, b);
    load_scaled(m, v0, V, fi[2], s, c);
    mb_cross(a, b, c, x);
    return 0.5f * mb_sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
}

// the value every lane before `lane` ended on: one serial chain over the 64 lanes (fixed order), every lane keeps its own step
__device__ __forceinline__ double wave_chain(double x, double start, int lane, double* mine) {
    double run = start;
#pragma unroll 4
    for (int k = 0; k < 64; ++k) {
        if (lane == k) *mine = run;
        run = run + __shfl(x, k);
    }
    return run;
}

// pass 1: chunk c of mesh n -> cdf[f] = fl(wb + fl(lb + loc)), the chunk-local CDF (final for chunk 0)
__global__ __launch_bounds__(MS_THREADS) void mesh_cdf_local_kernel(MeshBatch m, const float* __restrict__ scale, long n0,
                                                                    double* __restrict__ cdf) {
    __shared__ float sa[MS_CHUNK];
    __shared__ double sc[MS_CHUNK];
    __shared__ double wtot[4];
    const long n = n0 + blockIdx.y;
    const long f0 = m.face_off[n], F = m.face_off[n + 1] - f0, v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    const float s = scale ? scale[n] : 1.f;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long nchunks = (F + MS_CHUNK - 1) / MS_CHUNK;
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long base = c * MS_CHUNK;
        const int cnt = (int)min((long)MS_CHUNK, F - base);
#pragma unroll
        for (int k = 0; k < MS_K; ++k) {                                // coalesced over the faces; faces past the end add 0
            const int j = k * MS_THREADS + t;
            sa[j] = j < cnt ? face_area(m, v0, V, f0 + base + j, s) : 0.f;
        }
        __syncthreads();
        double loc[MS_K], run = 0.0;
#pragma unroll
        for (int k = 0; k < MS_K; ++k) { run = run + (double)sa[t * MS_K + k]; loc[k] = run; }
        double lb = 0.0;
        const double wsum = wave_chain(run, 0.0, lane, &lb);
        if (lane == 0) wtot[wave] = wsum;
        __syncthreads();
        double wb = 0.0;
        for (int w = 0; w < wave; ++w) wb = wb + wtot[w];
#pragma unroll
        for (int k = 0; k < MS_K; ++k) sc[t * MS_K + k] = wb + (lb + loc[k]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MS_K; ++k) {
            const int j = k * MS_THREADS + t;
            if (j < cnt) cdf[(size_t)(f0 + base + j)] = sc[j];
        }
        __syncthreads();
    }
}

// pass 2: one wave per mesh chains the chunk totals: the last element of chunk c becomes cb(c + 1) = fl(cb(c) + its local value)
__global__ __launch_bounds__(MS_THREADS) void mesh_cdf_chain_kernel(const long* __restrict__ face_off, long N, double* __restrict__ cdf,
                                                                    double* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const long f0 = face_off[n], F = face_off[n + 1] - f0;
    const long nchunks = (F + MS_CHUNK - 1) / MS_CHUNK;
    double run = 0.0;
    for (long c0 = 0; c0 < nchunks; c0 += 64) {
        const long c = c0 + lane;
        const bool ok = c < nchunks;
        const size_t last = (size_t)(f0 + min((c + 1) * MS_CHUNK, F) - 1);
        const double x = ok ? cdf[last] : 0.0;
        double before = 0.0;
        run = wave_chain(x, run, lane, &before);
        if (ok && c > 0) cdf[last] = before + x;
    }
    if (lane == 0) total[n] = run;
}

// pass 3: chunks 1.. add cb(c) = the (final) last element of chunk c - 1 to all but their own last element
__global__ __launch_bounds__(MS_THREADS) void mesh_cdf_apply_kernel(const long* __restrict__ face_off, long n0, double* __restrict__ cdf) {
    const long n = n0 + blockIdx.y;
    const long f0 = face_off[n], F = face_off[n + 1] - f0;
    const long nchunks = (F + MS_CHUNK - 1) / MS_CHUNK;
    for (long c = 1 + blockIdx.x; c < nchunks; c += gridDim.x) {
        const long base = c * MS_CHUNK;
        const int cnt = (int)min((long)MS_CHUNK, F - base);
        const double cb = cdf[(size_t)(f0 + base - 1)];
#pragma unroll
        for (int k = 0; k < MS_K; ++k) {
            const int j = k * MS_THREADS + threadIdx.x;
            if (j < cnt - 1) { double* p = cdf + (size_t)(f0 + base + j); *p = cb + *p; }
        }
    }
}

extern "C" int tri_mesh_face_cdf(const TriMeshBatch* batch, const float* scale, long max_faces, double* cdf, double* total, void* stream) {
    MeshBatch m;
    const int bad = mb_from_abi(batch, "tri_mesh_face_cdf", 0, &m);
    if (bad != TRI_OK) return bad;
    if (max_faces < 0) { tri_set_error("tri_mesh_face_cdf: negative size"); return TRI_ERR_ARG; }
    if (max_faces >= (1L << 31)) { tri_set_error("tri_mesh_face_cdf: 2^31 or more faces in a mesh"); return TRI_ERR_UNSUPPORTED; }
    const int N = m.N;
    const long* face_off = m.face_off;
    if (N == 0) return TRI_OK;
    hipStream_t st = (hipStream_t)stream;
    // blockIdx.x walks the chunks of a mesh (grid-stride), blockIdx.y the meshes; max_faces (>= every mesh's face count) sizes the grid
    const long chunks = max(1L, min((max_faces + MS_CHUNK - 1) / MS_CHUNK, 4096L));
    const long per_launch = max(1L, min((long)MS_MAX_GRID_Y, (long)MS_MAX_BLOCKS / chunks));
    for (long n0 = 0; n0 < N; n0 += per_launch)
        mesh_cdf_local_kernel<<<dim3((unsigned)chunks, (unsigned)min(per_launch, N - n0)), MS_THREADS, 0, st>>>(m, scale, n0, cdf);
    mesh_cdf_chain_kernel<<<(unsigned)(((long)N + 3) / 4), MS_THREADS, 0, st>>>(face_off, N, cdf, total);
    if (max_faces > MS_CHUNK)
        for (long n0 = 0; n0 < N; n0 += per_launch)
            mesh_cdf_apply_kernel<<<dim3((unsigned)max(1L, chunks - 1), (unsigned)min(per_launch, N - n0)), MS_THREADS, 0, st>>>(face_off, n0, cdf);
    return tri_check_launch("tri_mesh_face_cdf");
}

// ---- the sampler -----------------------------------------------------------------------------------------------------------------------
// (Philox4x32-10: common.h)
// One workgroup = MS_TILE consecutive samples of one mesh.  Every (MS_COARSE-th part of the) CDF's last entry is staged in LDS once per
// workgroup; a sample's search is ~11 LDS steps and then log2(stride) dependent global loads instead of log2(F) of them, four samples
// per thread in lockstep so that four such chains are in flight.  Points leave through LDS as consecutive dwords (a lane's own 12 bytes
// would be three stride-12 stores per wave).
template <bool IDX>
__global__ __launch_bounds__(MS_THREADS) void mesh_sample_kernel(MeshBatch m, const float* __restrict__ scale, const double* __restrict__ cdf,
                                                                 const double* __restrict__ total, int S, int tiles, long n0, uint32_t k0,
                                                                 uint32_t k1, float* __restrict__ points, long* __restrict__ face_idx) {
    __shared__ double coarse[MS_COARSE];
    __shared__ float sp[MS_TILE * 3];
    const int t = threadIdx.x;
    const long n = n0 + blockIdx.x / (unsigned)tiles;
    const int s0 = (int)(blockIdx.x % (unsigned)tiles) * MS_TILE;
    const int cnt = min(MS_TILE, S - s0);
    const long f0 = m.face_off[n], F = m.face_off[n + 1] - f0, v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    const double A = F > 0 ? total[n] : 0.0;
    float* out = points + ((size_t)n * S + s0) * 3;
    if (!(F > 0 && V > 0 && A > 0.0 && A < INFINITY)) {                // nothing to sample from: zero rows, -1 (pytorch3d zero-fills)
        for (int j = t; j < cnt * 3; j += MS_THREADS) out[j] = 0.f;
        if (IDX) for (int j = t; j < cnt; j += MS_THREADS) face_idx[(size_t)n * S + s0 + j] = -1L;
        return;
    }
    const double* cd = cdf + f0;
    const long stride = (F + MS_COARSE - 1) / MS_COARSE;
    const int nco = (int)((F + stride - 1) / stride);
    for (int k = t; k < nco; k += MS_THREADS) coarse[k] = cd[min((k + 1) * stride, F) - 1];
    __syncthreads();
    const float sc = scale ? scale[n] : 1.f;
    double tt[MS_SPT];
    float u1[MS_SPT], u2[MS_SPT];
    long lo[MS_SPT];
#pragma unroll
    for (int r = 0; r < MS_SPT; ++r) {
        const Philox4 p = philox4x32_10((uint32_t)(s0 + r * MS_THREADS + t), (uint32_t)n, 0u, 0u, k0, k1);
        tt[r] = (double)((float)(p.x[0] >> 8) * 0x1p-24f) * A;
        u1[r] = (float)(p.x[1] >> 8) * 0x1p-24f;
        u2[r] = (float)(p.x[2] >> 8) * 0x1p-24f;
        lo[r] = 0;
    }
    for (int len = nco; len > 1;) {                                    // coarse level: the smallest k with coarse[k] > t
        const int half = len >> 1;
#pragma unroll
        for (int r = 0; r < MS_SPT; ++r) lo[r] = coarse[lo[r] + half - 1] <= tt[r] ? lo[r] + half : lo[r];
        len -= half;
    }
#pragma unroll
    for (int r = 0; r < MS_SPT; ++r) lo[r] *= stride;
    for (long len = stride; len > 1;) {                                // inside the coarse cell; entries past the end count as > t
        const long half = len >> 1;
#pragma unroll
        for (int r = 0; r < MS_SPT; ++r) lo[r] = cd[min(lo[r] + half - 1, F - 1)] <= tt[r] ? lo[r] + half : lo[r];
        len -= half;
    }
#pragma unroll
    for (int r = 0; r < MS_SPT; ++r) {
        const int j = r * MS_THREADS + t;
        if (j >= cnt) continue;
        const long f = min(lo[r], F - 1);
        const int* fi = m.faces + (size_t)(f0 + f) * 3;
        float a[3], b[3], c[3];
        load_scaled(m, v0, V, fi[0], sc, a);
        load_scaled(m, v0, V, fi[1], sc, b);
        load_scaled(m, v0, V, fi[2], sc, c);
        const float rt = mb_sqrt(u1[r]);
        const float w0 = 1.0f - rt, w1 = rt * (1.0f - u2[r]), w2 = rt * u2[r];
#pragma unroll
        for (int k = 0; k < 3; ++k) sp[j * 3 + k] = (w0 * a[k] + w1 * b[k]) + w2 * c[k];
        if (IDX) face_idx[(size_t)n * S + s0 + j] = f;
    }
    __syncthreads();
    for (int j = t; j < cnt * 3; j += MS_THREADS) out[j] = sp[j];
}

extern "C" int tri_mesh_sample_points(const TriMeshBatch* batch, const float* scale, const double* cdf, const double* total, int S,
                                      unsigned long long seed, float* points, long* face_idx, void* stream) {
    MeshBatch m;
    const int bad = mb_from_abi(batch, "tri_mesh_sample_points", 0, &m);
    if (bad != TRI_OK) return bad;
    if (S < 0) { tri_set_error("tri_mesh_sample_points: negative size"); return TRI_ERR_ARG; }
    const int N = m.N;
    if (N == 0 || S == 0) return TRI_OK;
    const int tiles = (S + MS_TILE - 1) / MS_TILE;
    const long per_launch = max(1L, (long)MS_MAX_BLOCKS / tiles);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (long n0 = 0; n0 < N; n0 += per_launch) {
        const unsigned blocks = (unsigned)(min(per_launch, N - n0) * tiles);
        if (face_idx)
            mesh_sample_kernel<true><<<blocks, MS_THREADS, 0, (hipStream_t)stream>>>(m, scale, cdf, total, S, tiles, n0, k0, k1, points, face_idx);
        else
            mesh_sample_kernel<false><<<blocks, MS_THREADS, 0, (hipStream_t)stream>>>(m, scale, cdf, total, S, tiles, n0, k0, k1, points, face_idx);
    }
    return tri_check_launch("tri_mesh_sample_points");
}
