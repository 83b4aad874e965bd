// Coloured solid voxel grids from a packed batch of triangle meshes: the voxel32 / voxel64 / voxel128 entries of a packed .npz made from
// model_normalized.obj instead of the downloaded nrrd_256_filter_div_{V}_solid grids.  The reference has no voxeliser (it reads those
// files), so this is a definition of our own; NOBODY HAS COMPARED A GRID WITH TEXT2SHAPE'S - not the occupancy, not the orientation
// relative to the v2 meshes, not the colour of interior voxels.  The packed batch is the one mesh_batch.h lays out, with its
// materials; per mesh there is a frame fp32 [4] = (origin x, y, z, cell size); mesh x, y, z map to grid i, j, k.
// The kernel is DEFINED by its arithmetic; tricolo_amd/data/voxelize.py restates it in torch and gives the same bits.
//
//   snap (per vertex and axis; contraction is off in this file): t = fl32(fl64(v - o) / fl64(cell)) with v - o an fp32 subtraction,
//     G = (int)rintf(256 t) (1/256 voxel, ties to even).  A face is dropped when |256 t| <= 2^17 fails for any of its vertices (NaN
//     fails too): coordinates stay within 18 bits, a normal component within 2^37, every dot product below 2^57 - all in int64.
//     A mesh with cell <= 0 or a non-finite frame gives an all-zero grid.
//   surface: closed triangle / box overlap, exact, on the box [256 i, 256 (i + 1)]^3 of voxel (i, j, k).  With C = (256 i + 128,
//     256 j + 128, 256 k + 128) and u_k = G_k - C:
//     (a) per axis a: min_k u_k[a] <= 128 and max_k u_k[a] >= -128;
//     (b) n = (u1 - u0) x (u2 - u0): |n . u0| <= 128 (|nx| + |ny| + |nz|); a face with n = 0 is dropped;
//     (c) per edge f_j = u_{j+1} - u_j and unit axis e_i, a = e_i x f_j: min_k a . u_k <= r and max_k a . u_k >= -r with
//         r = 128 (|ax| + |ay| + |az|).
//     A voxel is a surface voxel when at least one face passes all thirteen tests.  Touching counts: a face lying in a voxel boundary
//     plane sets both layers (conservative on purpose: shells stay closed for the fill).  (a) gives the candidate index range per axis,
//     i from ceil(min G / 256) - 1 to floor(max G / 256), clipped to [0, V - 1]: a frame that cuts the mesh is legal.
//     The tests are evaluated as written up to exact integer algebra: n, n . G_0, a and min / max of a . G_k are formed once per
//     face, n . C and a . C per voxel.
//   surface colour: per material q = floor(255 clamp(Kd, 0, 1) + 0.5) in fp32 as raster.hip forms it (grey 0.4 for a mesh without
//     materials).  Per surface voxel the count and the three channel sums over ALL faces that pass - every face weighs the same,
//     whatever its area - by two 64-bit atomic adds of 32-bit fields (count | red << 32, green | blue << 32; a batch holds fewer than
//     2^24 faces, so no field carries).  channel = (2 sum + count) / (2 count) in integers.  Integer sums: independent of face order
//     and of arrival order.
//   fill (mode 1, "carve"): a non-surface voxel is open in one of the six axis directions when no surface voxel lies between it and
//     the grid boundary that way; it is exterior when open in at least one direction, interior otherwise.  An interior voxel takes the
//     colour of the nearest surface voxel along the six axis rays; the smallest distance wins, ties in the order -x, +x, -y, +y, -z,
//     +z.  This fills any cavity no axis ray can see out of; it is no flood fill.
//   output: u8 [N][4][V][V][V] indexed [channel][x][y][z] as read_nrrd returns; alpha 255 on surface and interior voxels, 0 elsewhere,
//     RGB 0 where alpha is 0.  Optionally labels u8 [N][V][V][V]: 0 exterior, 1 surface, 2 interior.
//
// Work: one lane per face sets it up; a candidate box of at most VX_SMALL_COUNT voxels stays with its lane, a larger one is appended
// to a device queue (one atomic add per wave, slots by ballot) that a second kernel on a fixed grid walks - one workgroup per queued
// face - with the count it reads on the device.  No host synchronisation.  The fill reads the occupancy as bit rows along each of the
// three axes (V / 32 words a row, 3 V^3 / 8 bytes a mesh, served from L2): clz / ffs on the row words give the two rays of an axis.
#include <math.h>

#include "mesh_batch.h"
#include "../../include/tricolo_hip.h"

#pragma clang fp contract(off)

#define VX_THREADS 256
#ifndef VX_SMALL_COUNT
#define VX_SMALL_COUNT 27                       // candidate boxes up to 3 x 3 x 3 voxels stay with their lane (8, 27, 64, 216, 512 and
                                                // 4096 timed on a 19,860-face mesh at V = 32 / 64 / 128: 27 was the fastest or within 3 % of it
                                                // at 64 and 128; 8 won at 32 but lost 30 % at 128)
#endif
#define VX_QUEUE_BLOCKS 4096                    // fixed grid of the queue kernel
#define VX_CLEAR_BLOCKS 2048
#define VX_SNAP_MAX 131072.f                    // 2^17 in 1/256 voxel
#define VX_MAX_VOXELS (1L << 31)
#define VX_MAX_FACES (1L << 24)                 // 255 * 2^24 < 2^32: the 32-bit fields of the colour sums never carry

struct VxFace {
    long n[3], nd, nr;                          // the normal, n . G_0, 128 |n|_1
    int ca[9], cb[9];                           // axis 3 j + i = e_i x f_j: its components along (i + 1) % 3 and (i + 2) % 3
    long lo[9], hi[9];                          // min_k / max_k of a . G_k
    int b0[3], b1[3];                           // the candidate index range per axis, clipped to the grid
};

__device__ __forceinline__ long vx_abs(long x) { return x < 0 ? -x : x; }

__device__ __forceinline__ bool vx_setup(const MeshBatch& m, const float* __restrict__ frame, long gf, int n, int V, VxFace& o) {
    const long v0 = m.vert_off[n], NV = m.vert_off[n + 1] - v0;
    if (NV <= 0) return false;
    const float* fr = frame + (size_t)n * 4;
    const float cell = fr[3];
    if (!(cell > 0.f) || !(cell < INFINITY) || !(fabsf(fr[0]) < INFINITY) || !(fabsf(fr[1]) < INFINITY) || !(fabsf(fr[2]) < INFINITY)) return false;
    const int* fi = m.faces + (size_t)gf * 3;
    int G[3][3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = mb_vertex(m, v0, NV, fi[k]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float d = p[a] - fr[a];
            const float s = 256.f * mb_div(d, cell);
            const bool in = fabsf(s) <= VX_SNAP_MAX;                    // false for NaN
            ok = ok && in;
            G[k][a] = in ? (int)rintf(s) : 0;
        }
    }
    if (!ok) return false;
    long e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e1[a] = (long)G[1][a] - G[0][a]; e2[a] = (long)G[2][a] - G[0][a]; }
    o.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    o.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    o.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    if ((o.n[0] | o.n[1] | o.n[2]) == 0) return false;
    o.nd = o.n[0] * G[0][0] + o.n[1] * G[0][1] + o.n[2] * G[0][2];
    o.nr = 128L * (vx_abs(o.n[0]) + vx_abs(o.n[1]) + vx_abs(o.n[2]));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int mn = min(G[0][a], min(G[1][a], G[2][a])), mx = max(G[0][a], max(G[1][a], G[2][a]));
        o.b0[a] = max(0, ((mn + 255) >> 8) - 1);                        // ceil(min / 256) - 1
        o.b1[a] = min(V - 1, mx >> 8);                                  // floor(max / 256)
    }
    if (o.b0[0] > o.b1[0] || o.b0[1] > o.b1[1] || o.b0[2] > o.b1[2]) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int j1 = (j + 1) % 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, e = 3 * j + i;
            const int ca = -(G[j1][i2] - G[j][i2]), cb = G[j1][i1] - G[j][i1];      // e_i x f: [i1] = -f[i2], [i2] = f[i1]
            o.ca[e] = ca;
            o.cb[e] = cb;
            const long p0 = (long)ca * G[0][i1] + (long)cb * G[0][i2];
            const long p1 = (long)ca * G[1][i1] + (long)cb * G[1][i2];
            const long p2 = (long)ca * G[2][i1] + (long)cb * G[2][i2];
            o.lo[e] = min(p0, min(p1, p2));
            o.hi[e] = max(p0, max(p1, p2));
        }
    }
    return true;
}

// tests (b) and (c) at voxel (i, j, k); (a) holds everywhere in the face's candidate box
__device__ __forceinline__ bool vx_hit(const VxFace& f, int i, int j, int k) {
    const int C[3] = {256 * i + 128, 256 * j + 128, 256 * k + 128};
    const long d = f.nd - (f.n[0] * C[0] + f.n[1] * C[1] + f.n[2] * C[2]);
    bool ok = vx_abs(d) <= f.nr;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const int i1 = (e % 3 + 1) % 3, i2 = (e % 3 + 2) % 3;
        const long ac = (long)f.ca[e] * C[i1] + (long)f.cb[e] * C[i2];
        const long r = 128L * ((long)abs(f.ca[e]) + (long)abs(f.cb[e]));
        ok = ok && (f.lo[e] - ac <= r) && (f.hi[e] - ac >= -r);
    }
    return ok;
}

// the two packed addends of face gf: 1 | red << 32 and green | blue << 32
__device__ __forceinline__ void vx_colour(const MeshBatch& m, int n, long gf, u64& A, u64& B) {
    float kd[3];
    mb_face_kd(m, n, gf, kd);
    u64 q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float col = fminf(fmaxf(kd[k], 0.f), 1.f);
        q[k] = (u64)(int)floorf(255.f * col + 0.5f);
    }
    A = 1ULL | (q[0] << 32);
    B = q[1] | (q[2] << 32);
}

__global__ __launch_bounds__(VX_THREADS) void voxelize_clear_kernel(u64* __restrict__ words, long nwords, u64* __restrict__ qcount) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *qcount = 0;
    for (long i = (long)blockIdx.x * VX_THREADS + threadIdx.x; i < nwords; i += (long)gridDim.x * VX_THREADS) words[i] = 0;
}

// one lane per face of the whole batch
__global__ __launch_bounds__(VX_THREADS) void voxelize_faces_kernel(MeshBatch m, const float* __restrict__ frame, long sumF, int V,
                                                                    u64* __restrict__ acc, u64* __restrict__ qcount,
                                                                    unsigned* __restrict__ queue, u64 qcap) {
    const long gf = (long)blockIdx.x * VX_THREADS + threadIdx.x;
    VxFace f;
    bool live = false, big = false;
    int n = 0;
    if (gf < sumF) {
        n = mb_mesh_of(m, gf);
        live = vx_setup(m, frame, gf, n, V, f);
        big = live && (long)(f.b1[0] - f.b0[0] + 1) * (f.b1[1] - f.b0[1] + 1) * (f.b1[2] - f.b0[2] + 1) > VX_SMALL_COUNT;
    }
    const u64 slot = mb_queue_slot(big, qcount);                        // every lane of the wave is here
    if (big && slot < qcap) queue[slot] = (unsigned)gf;
    if (!live || big) return;
    u64 A, B;
    vx_colour(m, n, gf, A, B);
    for (int i = f.b0[0]; i <= f.b1[0]; ++i)
        for (int j = f.b0[1]; j <= f.b1[1]; ++j)
            for (int k = f.b0[2]; k <= f.b1[2]; ++k)
                if (vx_hit(f, i, j, k)) {
                    u64* a = acc + 2 * ((((size_t)n * V + i) * V + j) * V + k);
                    atomicAdd(a, A);
                    atomicAdd(a + 1, B);
                }
}

// fixed grid; workgroup b takes queue entries b, b + gridDim.x, ... up to the count the first kernel left on the device
__global__ __launch_bounds__(VX_THREADS) void voxelize_queue_kernel(MeshBatch m, const float* __restrict__ frame, int V, u64* __restrict__ acc,
                                                                    const u64* __restrict__ qcount, const unsigned* __restrict__ queue,
                                                                    u64 qcap) {
    const u64 count = min(*qcount, qcap);
    for (u64 q = blockIdx.x; q < count; q += gridDim.x) {
        const long gf = queue[q];
        const int n = mb_mesh_of(m, gf);
        VxFace f;
        if (!vx_setup(m, frame, gf, n, V, f)) continue;                                    // the same answer in every lane
        u64 A, B;
        vx_colour(m, n, gf, A, B);
        const int bj = f.b1[1] - f.b0[1] + 1, bk = f.b1[2] - f.b0[2] + 1, bjk = bj * bk;
        const int cnt = (f.b1[0] - f.b0[0] + 1) * bjk;                                     // at most 128^3
        for (int t = threadIdx.x; t < cnt; t += VX_THREADS) {
            const int di = t / bjk, rem = t - di * bjk, dj = rem / bk, dk = rem - dj * bk;
            const int i = f.b0[0] + di, j = f.b0[1] + dj, k = f.b0[2] + dk;
            if (vx_hit(f, i, j, k)) {
                u64* a = acc + 2 * ((((size_t)n * V + i) * V + j) * V + k);
                atomicAdd(a, A);
                atomicAdd(a + 1, B);
            }
        }
    }
}

// one thread per voxel: a surface voxel sets its bit in the x row (j, k), the y row (i, k) and the z row (i, j) of its mesh
__global__ __launch_bounds__(VX_THREADS) void voxelize_rows_kernel(const u64* __restrict__ acc, long nvox, int V, unsigned* __restrict__ bx,
                                                                   unsigned* __restrict__ by, unsigned* __restrict__ bz) {
    const long v = (long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (v >= nvox) return;
    if ((unsigned)acc[2 * v] == 0) return;
    const int W = V >> 5;
    const int k = (int)(v % V), j = (int)((v / V) % V), i = (int)((v / ((long)V * V)) % V);
    const long n = v / ((long)V * V * V);
    atomicOr(bx + ((n * V + j) * V + k) * W + (i >> 5), 1u << (i & 31));
    atomicOr(by + ((n * V + i) * V + k) * W + (j >> 5), 1u << (j & 31));
    atomicOr(bz + ((n * V + i) * V + j) * W + (k >> 5), 1u << (k & 31));
}

// the largest set bit index below p in a row of W words, -1 when there is none
__device__ __forceinline__ int vx_below(const unsigned* __restrict__ row, int p) {
    int w = p >> 5;
    unsigned m = row[w] & ((1u << (p & 31)) - 1u);
    while (true) {
        if (m) return (w << 5) + 31 - __clz((int)m);
        if (--w < 0) return -1;
        m = row[w];
    }
}

// the smallest set bit index above p, -1 when there is none
__device__ __forceinline__ int vx_above(const unsigned* __restrict__ row, int p, int W) {
    int w = p >> 5;
    unsigned m = row[w] & ~((2u << (p & 31)) - 1u);
    while (true) {
        if (m) return (w << 5) + __ffs((int)m) - 1;
        if (++w >= W) return -1;
        m = row[w];
    }
}

// one thread per voxel: its label and colour
__global__ __launch_bounds__(VX_THREADS) void voxelize_resolve_kernel(const u64* __restrict__ acc, long nvox, int V, int fill,
                                                                      const unsigned* __restrict__ bx, const unsigned* __restrict__ by,
                                                                      const unsigned* __restrict__ bz, uint8_t* __restrict__ grid,
                                                                      uint8_t* __restrict__ labels) {
    const long v = (long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (v >= nvox) return;
    const long V3 = (long)V * V * V;
    const long n = v / V3, local = v - n * V3;
    long src = -1;
    int label = 0;
    if ((unsigned)acc[2 * v] != 0) {
        src = v;
        label = 1;
    } else if (fill) {
        const int W = V >> 5;
        const int k = (int)(local % V), j = (int)((local / V) % V), i = (int)(local / ((long)V * V));
        const unsigned* rx = bx + ((n * V + j) * V + k) * W;
        const unsigned* ry = by + ((n * V + i) * V + k) * W;
        const unsigned* rz = bz + ((n * V + i) * V + j) * W;
        const int h[6] = {vx_below(rx, i), vx_above(rx, i, W), vx_below(ry, j), vx_above(ry, j, W), vx_below(rz, k), vx_above(rz, k, W)};
        if (h[0] >= 0 && h[1] >= 0 && h[2] >= 0 && h[3] >= 0 && h[4] >= 0 && h[5] >= 0) {
            const int p[3] = {i, j, k};
            int best = V, hit[3] = {i, j, k};
#pragma unroll
            for (int r = 0; r < 6; ++r) {                               // -x, +x, -y, +y, -z, +z: an earlier ray keeps a tie
                const int dist = (r & 1) ? h[r] - p[r >> 1] : p[r >> 1] - h[r];
                if (dist < best) {
                    best = dist;
                    hit[0] = i; hit[1] = j; hit[2] = k;
                    hit[r >> 1] = h[r];
                }
            }
            src = ((n * V + hit[0]) * V + hit[1]) * V + hit[2];
            label = 2;
        }
    }
    uint8_t* out = grid + (size_t)n * 4 * V3 + local;
    if (labels) labels[v] = (uint8_t)label;
    if (src < 0) {
        out[0] = 0; out[V3] = 0; out[2 * V3] = 0; out[3 * V3] = 0;
        return;
    }
    const u64 A = acc[2 * src], B = acc[2 * src + 1];
    const u64 cnt = A & 0xFFFFFFFFull;
    out[0] = (uint8_t)((2 * (A >> 32) + cnt) / (2 * cnt));
    out[V3] = (uint8_t)((2 * (B & 0xFFFFFFFFull) + cnt) / (2 * cnt));
    out[2 * V3] = (uint8_t)((2 * (B >> 32) + cnt) / (2 * cnt));
    out[3 * V3] = 255;
}

static bool vx_size_ok(int V) { return V == 32 || V == 64 || V == 128; }

extern "C" size_t tri_voxelize_workspace(long sumF, int N, int V) {
    if (N < 0 || sumF < 0 || sumF >= VX_MAX_FACES || !vx_size_ok(V) || (double)N * V * V * V >= (double)VX_MAX_VOXELS) return 0;
    const size_t nvox = (size_t)N * V * V * V;
    return nvox * 16 + 3 * (nvox / 8) + 16 + (size_t)sumF * 4;           // sums | x, y, z bit rows | queue count (padded to 16 bytes) | queue
}

extern "C" int tri_voxelize_meshes(const TriMeshBatch* batch, const float* frame, long sumF, int V, int fill, void* workspace, uint8_t* grid,
                                   uint8_t* labels, void* stream) {
    MeshBatch m;
    const int bad = mb_from_abi(batch, "tri_voxelize_meshes", 0, &m);
    if (bad != TRI_OK) return bad;
    const int N = m.N;
    if (sumF < 0) { tri_set_error("tri_voxelize_meshes: negative size"); return TRI_ERR_ARG; }
    if (fill != 0 && fill != 1) { tri_set_error("tri_voxelize_meshes: fill must be 0 (surface) or 1 (carve)"); return TRI_ERR_ARG; }
    if (!vx_size_ok(V)) { tri_set_error("tri_voxelize_meshes: V must be 32, 64 or 128"); return TRI_ERR_UNSUPPORTED; }
    if (sumF >= VX_MAX_FACES) { tri_set_error("tri_voxelize_meshes: 2^24 or more faces in a batch"); return TRI_ERR_UNSUPPORTED; }
    if ((double)N * V * V * V >= (double)VX_MAX_VOXELS) { tri_set_error("tri_voxelize_meshes: 2^31 or more voxels in one launch"); return TRI_ERR_UNSUPPORTED; }
    const long nvox = (long)N * V * V * V;
    if (nvox == 0) return TRI_OK;
    hipStream_t st = (hipStream_t)stream;
    u64* acc = (u64*)workspace;
    unsigned* bx = (unsigned*)(acc + 2 * nvox);
    unsigned* by = bx + nvox / 32;
    unsigned* bz = by + nvox / 32;
    u64* qcount = (u64*)(bz + nvox / 32);
    unsigned* queue = (unsigned*)(qcount + 2);
    const long nwords = 2 * nvox + 3 * (nvox / 64);
    const unsigned vblocks = (unsigned)((nvox + VX_THREADS - 1) / VX_THREADS);
    voxelize_clear_kernel<<<(unsigned)min((long)VX_CLEAR_BLOCKS, (nwords + VX_THREADS - 1) / VX_THREADS), VX_THREADS, 0, st>>>(acc, nwords, qcount);
    if (sumF > 0) {
        voxelize_faces_kernel<<<(unsigned)((sumF + VX_THREADS - 1) / VX_THREADS), VX_THREADS, 0, st>>>(m, frame, sumF, V, acc, qcount, queue,
                                                                                                       (u64)sumF);
        voxelize_queue_kernel<<<VX_QUEUE_BLOCKS, VX_THREADS, 0, st>>>(m, frame, V, acc, qcount, queue, (u64)sumF);
        if (fill) voxelize_rows_kernel<<<vblocks, VX_THREADS, 0, st>>>(acc, nvox, V, bx, by, bz);
    }
    voxelize_resolve_kernel<<<vblocks, VX_THREADS, 0, st>>>(acc, nvox, V, fill, bx, by, bz, grid, labels);
    return tri_check_launch("tri_voxelize_meshes");
}
