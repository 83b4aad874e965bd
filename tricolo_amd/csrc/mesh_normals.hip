// Vertex normals of a packed batch of triangle meshes (mesh_batch.h), written as the corner normals face_vn fp32 [sumF][3][3] that
// the smooth resolve kernels of raster.hip read.  A DEFINITION OF OUR OWN, as the voxeliser's is: area-weighted (trimesh weighs by
// angle), by vertex INDEX (vertices at one position are not merged), bit-reproducible and independent of the order of the faces.
// tricolo_amd/data/render.py restates it in torch (mesh_vertex_normals_cpu) and gives the same bits.
//
//   pass 1, one lane per face of the batch (mesh n owns it; V = its vertex count, nothing happens for V <= 0):
//     c = (b - a) x (c - a) by mb_cross: fp32, every operation rounded on its own (contraction is off), a, b, c the face's vertices
//       after mb_vertex's unsigned clamp of a bad index;
//     a face with a component of c that is not finite contributes nothing;
//     otherwise every component is clamped to [-2^16, 2^16] and turned into fixed point, q_k = llrint(fl64(c_k) 2^36): the product is
//       exact in float64 (24 bits scaled by a power of two), the rounding is to nearest, ties to even; |q_k| <= 2^52;
//     q is added with 64-bit integer atomics to acc int64 [sumV][3] at each of the face's three (clamped) vertices.  Integer adds
//       commute, so the sums do not depend on the order in which faces arrive - the voxeliser's idiom.  A vertex shared by more than
//       2^10 faces whose components all sit at the clamp would wrap the sum; the wrap is modular and still deterministic.  A component
//       below 2^-37 (a face area of some 1e-11) rounds to 0.
//   pass 2, one lane per face:
//     fill 0 ("missing") and an incoming face_vn whose marker face_vn_in[f][0][0] is not NaN: the nine incoming values, bit for bit;
//     otherwise per corner S = acc[vertex], len = sqrt((fl64(S_x)^2 + fl64(S_y)^2) + fl64(S_z)^2) in float64 in that order,
//       n_k = fl32(fl64(S_k) / len); a face with a corner whose S is (0, 0, 0) - or whose mesh has no vertices - is written as nine
//       NaNs, the marker of a face without normals: it renders flat.
//     fill 1 ("all") overwrites every face.  A mesh without faces has nothing to write.
//
// Work: three launches on the caller's stream - clear acc, pass 1, pass 2 - and no host synchronisation.  The workspace is acc alone,
// 24 bytes per vertex of the batch.  No vertex row outside [0, sumV) is ever added to or read, whatever the offset tables hold.
#include <math.h>

#include "mesh_batch.h"
#include "../../include/tricolo_hip.h"

#pragma clang fp contract(off)

#define MN_THREADS 256
#define MN_CLEAR_BLOCKS 2048
#define MN_CLAMP 65536.f                        // 2^16
#define MN_SCALE 68719476736.0                  // 2^36

__global__ __launch_bounds__(MN_THREADS) void mesh_normals_clear_kernel(long* __restrict__ acc, long n) {
    for (long i = (long)blockIdx.x * MN_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * MN_THREADS) acc[i] = 0;
}

// the row of acc of vertex i of the mesh that owns the V > 0 vertices from v0 (mb_vertex's clamp); -1 when the tables point outside the batch
__device__ __forceinline__ long mn_row(long v0, long V, int i, long sumV) {
    const long r = v0 + min((long)(unsigned)i, V - 1);
    return r >= 0 && r < sumV ? r : -1;
}

__global__ __launch_bounds__(MN_THREADS) void mesh_normals_sum_kernel(MeshBatch m, long sumV, long sumF, u64* __restrict__ acc) {
    const long gf = (long)blockIdx.x * MN_THREADS + threadIdx.x;
    if (gf >= sumF) return;
    const int n = mb_mesh_of(m, gf);
    const long v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    if (V <= 0) return;
    const int* fi = m.faces + (size_t)gf * 3;
    const long r[3] = {mn_row(v0, V, fi[0], sumV), mn_row(v0, V, fi[1], sumV), mn_row(v0, V, fi[2], sumV)};
    if (r[0] < 0 || r[1] < 0 || r[2] < 0) return;
    float c[3];
    mb_cross(m.verts + (size_t)r[0] * 3, m.verts + (size_t)r[1] * 3, m.verts + (size_t)r[2] * 3, c);
    if (!(mb_finite(c[0]) && mb_finite(c[1]) && mb_finite(c[2]))) return;
    u64 q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (u64)llrint((double)fminf(fmaxf(c[k], -MN_CLAMP), MN_CLAMP) * MN_SCALE);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(acc + (size_t)r[j] * 3 + k, q[k]);    // two's complement: the unsigned add is the signed one
    }
}

__global__ __launch_bounds__(MN_THREADS) void mesh_normals_write_kernel(MeshBatch m, long sumV, long sumF, int fill, const long* __restrict__ acc,
                                                                        const float* __restrict__ vn_in, float* __restrict__ vn_out) {
    const long gf = (long)blockIdx.x * MN_THREADS + threadIdx.x;
    if (gf >= sumF) return;
    float* out = vn_out + (size_t)gf * 9;
    if (fill == 0 && vn_in) {
        const unsigned* in = (const unsigned*)vn_in + (size_t)gf * 9;
        const float marker = __uint_as_float(in[0]);
        if (marker == marker) {                                         // given: kept bit for bit
#pragma unroll
            for (int k = 0; k < 9; ++k) ((unsigned*)out)[k] = in[k];
            return;
        }
    }
    const int n = mb_mesh_of(m, gf);
    const long v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    const int* fi = m.faces + (size_t)gf * 3;
    float o[9];
    bool ok = V > 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const long r = ok ? mn_row(v0, V, fi[j], sumV) : -1;
        ok = ok && r >= 0;
        const long* s = acc + (size_t)max(r, 0L) * 3;
        const long sx = ok ? s[0] : 0, sy = ok ? s[1] : 0, sz = ok ? s[2] : 0;
        ok = ok && (sx | sy | sz) != 0;
        const double x = (double)sx, y = (double)sy, z = (double)sz;
        const double len = ok ? sqrt((x * x + y * y) + z * z) : 1.0;
        o[3 * j] = (float)(x / len); o[3 * j + 1] = (float)(y / len); o[3 * j + 2] = (float)(z / len);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = ok ? o[k] : __uint_as_float(0x7FC00000u);
}

extern "C" size_t tri_mesh_vertex_normals_workspace(long sumV) { return sumV > 0 ? (size_t)sumV * 24 : 0; }

extern "C" int tri_mesh_vertex_normals(const TriMeshBatch* batch, long sumV, long sumF, int fill, void* workspace, const float* face_vn_in,
                                       float* face_vn_out, void* stream) {
    MeshBatch m;
    const int bad = mb_from_abi(batch, "tri_mesh_vertex_normals", 0, &m);
    if (bad != TRI_OK) return bad;
    if (sumV < 0 || sumF < 0) { tri_set_error("tri_mesh_vertex_normals: negative size"); return TRI_ERR_ARG; }
    if (fill != 0 && fill != 1) { tri_set_error("tri_mesh_vertex_normals: fill must be 0 (missing) or 1 (all)"); return TRI_ERR_ARG; }
    if (sumF >= (1L << 31) || sumV >= (1L << 31)) {
        tri_set_error("tri_mesh_vertex_normals: 2^31 or more faces or vertices in a batch");
        return TRI_ERR_UNSUPPORTED;
    }
    if (sumF == 0 || m.N == 0) return TRI_OK;
    if (!m.verts || !m.faces || !m.vert_off || !m.face_off || !face_vn_out || (sumV > 0 && !workspace)) {
        tri_set_error("tri_mesh_vertex_normals: the batch, the workspace and the output must not be null");
        return TRI_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((sumF + MN_THREADS - 1) / MN_THREADS);
    if (sumV > 0) {
        const long n = sumV * 3;
        mesh_normals_clear_kernel<<<(unsigned)min((long)MN_CLEAR_BLOCKS, (n + MN_THREADS - 1) / MN_THREADS), MN_THREADS, 0, st>>>((long*)workspace, n);
        mesh_normals_sum_kernel<<<blocks, MN_THREADS, 0, st>>>(m, sumV, sumF, (u64*)workspace);
    }
    mesh_normals_write_kernel<<<blocks, MN_THREADS, 0, st>>>(m, sumV, sumF, fill, (const long*)workspace, face_vn_in, face_vn_out);
    return tri_check_launch("tri_mesh_vertex_normals");
}
