// The packed batch of N triangle meshes that mesh_sample.hip, raster.hip and voxelize.hip work on, and the conventions all three keep;
// tricolo_amd/meshes.py packs it on the host (MeshBatch.pack).  Mesh n owns the rows off[n] .. off[n + 1] - 1 of its arrays:
//   verts fp32 [sumV][3] by vert_off, faces int32 [sumF][3] and face_mat int32 [sumF] by face_off, mat_kd fp32 [sumM][3] by mat_off;
//   the three offset arrays are int64 [N + 1].
// A face holds vertex indices LOCAL to its mesh, face_mat a material index local to the mesh; mat_kd holds diffuse colours.  The host
// validates the indices; the kernels still read each as unsigned and clamp it to the mesh's last vertex (material), so a bad index
// never reads beyond the mesh.  A mesh without vertices has nothing to clamp to - every kernel checks V > 0 first - and a mesh without
// materials is grey 0.4.  The sampler has no use for materials and leaves the three material fields null.
//
// The four groups after N are optional.  A caller hands the batch over as the TriMeshBatch of include/tricolo_hip.h, whose `fields`
// DECLARES the groups that are there; mb_from_abi below is the only place a MeshBatch is filled from one, and a group that is not
// declared reaches the kernels as null / T = 0, whatever its slots held.
//
// Textures (TRI_MESH_TEXTURES: the five fields and T).  face_uv fp32 [sumF][3][2] holds one (u, v)
// per face corner in the order of `faces`; a face whose face_uv[f][0][0] is NaN has no texture coordinates (the host writes NaN into
// all six values).  mat_tex int32 [sumM] names a material's texture by a BATCH-GLOBAL index, -1 = none; any other value is read as
// unsigned and clamped to T - 1, and with T == 0 every material is untextured.  Texture t is the tex_size[t] = (height, width) texels
// from tex_off[t] (int64 [T + 1]) of texels u8 [sumTexels][4] = R, G, B, alpha (ignored, written as 255): one aligned dword each.  Row
// 0 is the top row of the image and v = 0 its bottom (the OBJ convention).  mb_tex_sample below is THE sampling rule - repeat wrap,
// bilinear (mb_bilinear), no mip-maps - of the textured resolve pass of raster.hip and of its face colours.
//
// The mip pyramid (TRI_MESH_MIPS: the two fields; raster.hip's tri_texture_mips builds it and only its mip resolve kernels read it;
// with T == 0 it may be null).  Texture t of size (H0, W0) has L = floor(log2(max(H0, W0))) + 1 levels, level l of size
// (H_l, W_l) = (max(1, H0 >> l), max(1, W0 >> l)); level 0 is a copy of the texture.  mip_texels u8 [sumMipTexels][4] holds the chain
// of texture t from mip_off[t] (int64 [T + 1]): its levels one after the other from level 0, each row major, RGBA with alpha 255.
// There is NO table of level offsets: a kernel walks them from tex_size - level l starts sum_{k < l} H_k W_k texels into the chain, at
// most 24 steps of two shifts, a multiply and an add (mb_mip_level), which costs less than a dependent load per sample would.
// A texel of level l >= 1 is formed from LEVEL 0, not from the level below, in integers: texel (y, x) covers the columns j of level 0
// with weight wx(j) = max(0, min((x + 1) W0, (j + 1) W_l) - max(x W0, j W_l)) (they add up to W0), the rows i with wy(i) likewise in
// H; with S = sum_i sum_j wy(i) wx(j) texel0[i][j][k] and D = H0 W0 the value is (2 S + D) / (2 D) in integer division - the box mean,
// half rounded up; int64 holds it (2 * 255 * 2^48 < 2^63).  For power-of-two sizes that is the rounded mean of the 2^l x 2^l block.
// mb_mip_sample is mb_tex_sample's rule on one level, with that level's own (H_l, W_l).
//
// Corner normals (TRI_MESH_NORMALS).  face_vn fp32 [sumF][3][3] holds one normal per face corner in the order of `faces`, indexed by global face like face_uv; a face whose face_vn[f][0][0] is NaN has no normals (the host writes NaN
// into all nine values) and is shaded flat.  Normals need not be unit length.  They come from the `vn` lines of the OBJ file
// (data/materials.py load_obj_normals) or from mesh_normals.hip (tri_mesh_vertex_normals: area-weighted, by vertex index); only the
// SMOOTH resolve kernels of raster.hip read them.
//
// PBR factors (TRI_MESH_PBR).  mat_pbr fp32 [sumM][2] holds (metallic, roughness) per material, indexed like mat_kd by mat_off and the face's clamped material.  mb_face_pbr
// below reads them: metallic is clamped to [0, 1] and roughness to [0.04, 1], each as fminf(fmaxf(x, lo), hi), so a NaN takes the lower
// bound; a mesh without materials takes (0.2, 0.8) beside its grey 0.4.  Only the BRDF resolve kernels of raster.hip read them.
//
// Contraction is switched off HERE, not only in the including files: `#pragma clang fp contract(off)` covers the code that follows it,
// so a helper defined in a header ahead of the including file's own pragma would be compiled with contraction on - a * b + c became
// v_fmac_f32 in such a helper while the same expression in a kernel body stayed a multiply and an add.  With an fma the cross product
// of a face with b == c is a rounding error instead of exactly 0, and the torch restatements could not form the same bits.
#pragma once
#include <stdio.h>
#include "common.h"
#include "../../include/tricolo_hip.h"

#pragma clang fp contract(off)

typedef unsigned long long u64;

struct MeshBatch {
    const float* __restrict__ verts;
    const int* __restrict__ faces;
    const long* __restrict__ vert_off;
    const long* __restrict__ face_off;
    const int* __restrict__ face_mat;
    const float* __restrict__ mat_kd;
    const long* __restrict__ mat_off;
    int N;
    const float* __restrict__ face_uv;              // the texture fields
    const int* __restrict__ mat_tex;
    const unsigned* __restrict__ texels;            // one RGBA texel per dword, R in the low byte
    const long* __restrict__ tex_off;
    const int* __restrict__ tex_size;
    int T;
    const unsigned* __restrict__ mip_texels;        // the mip pyramid
    const long* __restrict__ mip_off;
    const float* __restrict__ face_vn;              // the corner normals
    const float* __restrict__ mat_pbr;              // (metallic, roughness) per material
};

static inline int mb_refuse(const char* who, const char* what) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    tri_set_error(msg);
    return TRI_ERR_ARG;
}

// *out = the batch entry point `who` was handed, with the groups b->fields declares and every other group null / T = 0; allowed: the
// TRI_MESH_* groups `who` takes.  THE rules of the descriptor (include/tricolo_hip.h states them for callers); TRI_ERR_ARG, with a
// message that begins with `who`, for a descriptor that breaks one.
static inline int mb_from_abi(const TriMeshBatch* b, const char* who, unsigned allowed, MeshBatch* out) {
    if (!b) return mb_refuse(who, "the batch descriptor must not be null");
    if (b->N < 0 || b->T < 0) return mb_refuse(who, "negative size");
    if (b->fields & ~allowed) return mb_refuse(who, "the batch declares a field group that this call does not take");
    const bool tex = b->fields & TRI_MESH_TEXTURES, mips = b->fields & TRI_MESH_MIPS;
    if (mips && !tex) return mb_refuse(who, "TRI_MESH_MIPS needs TRI_MESH_TEXTURES");
    if (tex && b->T > 0 && !(b->face_uv && b->mat_tex && b->texels && b->tex_off && b->tex_size && (!mips || (b->mip_texels && b->mip_off))))
        return mb_refuse(who, mips ? "T > 0 needs all five texture fields and both pyramid fields" : "T > 0 needs all five texture fields");
    if ((b->fields & TRI_MESH_NORMALS) && !b->face_vn) return mb_refuse(who, "face_vn must not be null");
    if ((b->fields & TRI_MESH_PBR) && !b->mat_pbr) return mb_refuse(who, "mat_pbr must not be null");
    *out = MeshBatch{b->verts, b->faces, b->vert_off, b->face_off, b->face_mat, b->mat_kd, b->mat_off, b->N};
    if (tex) {
        out->face_uv = b->face_uv; out->mat_tex = b->mat_tex; out->texels = (const unsigned*)b->texels;
        out->tex_off = b->tex_off; out->tex_size = b->tex_size; out->T = b->T;
    }
    if (mips) { out->mip_texels = (const unsigned*)b->mip_texels; out->mip_off = b->mip_off; }
    if (b->fields & TRI_MESH_NORMALS) out->face_vn = b->face_vn;
    if (b->fields & TRI_MESH_PBR) out->mat_pbr = b->mat_pbr;
    return TRI_OK;
}

// the mesh of global face gf: the largest n with face_off[n] <= gf (meshes without faces are stepped over)
__device__ __forceinline__ int mb_mesh_of(const MeshBatch& m, long gf) {
    int lo = 0, hi = m.N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (m.face_off[mid] <= gf) lo = mid; else hi = mid;
    }
    return lo;
}

// vertex i of the mesh that owns the V > 0 vertices from v0: a bad index reads the mesh's own last vertex, never beyond it
__device__ __forceinline__ const float* mb_vertex(const MeshBatch& m, long v0, long V, int i) {
    return m.verts + (size_t)(v0 + min((long)(unsigned)i, V - 1)) * 3;
}

// the diffuse colour of global face gf of mesh n: a bad material index reads the mesh's own last material; grey without materials
__device__ __forceinline__ void mb_face_kd(const MeshBatch& m, int n, long gf, float* kd) {
    const long m0 = m.mat_off[n], M = m.mat_off[n + 1] - m0;
    const long j = min((long)(unsigned)m.face_mat[gf], M - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) kd[k] = M > 0 ? m.mat_kd[(size_t)(m0 + j) * 3 + k] : 0.4f;
}

// the clamped (metallic, roughness) of global face gf of mesh n (m.mat_pbr is not null): a bad material index reads the mesh's own last
// material; (0.2, 0.8) without materials.  fmaxf first, then fminf: a NaN takes the lower bound, 0 or 0.04.
__device__ __forceinline__ void mb_face_pbr(const MeshBatch& m, int n, long gf, float& metal, float& rough) {
    const long m0 = m.mat_off[n], M = m.mat_off[n + 1] - m0;
    const long j = min((long)(unsigned)m.face_mat[gf], M - 1);
    metal = fminf(fmaxf(M > 0 ? m.mat_pbr[(size_t)(m0 + j) * 2] : 0.2f, 0.f), 1.f);
    rough = fminf(fmaxf(M > 0 ? m.mat_pbr[(size_t)(m0 + j) * 2 + 1] : 0.8f, 0.04f), 1.f);
}

// o = (b - a) x (c - a) in fp32, every operation rounded on its own
__device__ __forceinline__ void mb_cross(const float* a, const float* b, const float* c, float* o) {
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    o[0] = uy * wz - uz * wy; o[1] = uz * wx - ux * wz; o[2] = ux * wy - uy * wx;
}

// The correctly rounded quotient and root (what numpy and torch give on the host).  __fsqrt_rn compiles to the bare v_sqrt_f32 here,
// 1 ulp off in a third of the cases, which biased the sampler's CDF by 2^-26 of the total against the cumsum of the fp32 areas.  Through
// float64 the result is exact: a correctly rounded 53-bit result rounded again to 24 bits equals the directly rounded one (53 >= 2 * 24 + 2).
__device__ __forceinline__ float mb_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float mb_sqrt(float x) { return (float)sqrt((double)x); }

// The texture of global face gf of mesh n, -1 for none: no textures in the batch, a mesh without materials, a material with mat_tex
// -1, or a face whose first texture coordinate is the NaN marker.  A bad index reads the batch's last texture.
__device__ __forceinline__ int mb_face_tex(const MeshBatch& m, int n, long gf) {
    const long m0 = m.mat_off[n], M = m.mat_off[n + 1] - m0;
    if (m.T <= 0 || M <= 0) return -1;
    const int t = m.mat_tex[m0 + min((long)(unsigned)m.face_mat[gf], M - 1)];
    const float u0 = m.face_uv[(size_t)gf * 6];
    if (t == -1 || u0 != u0) return -1;
    return (int)min((long)(unsigned)t, (long)m.T - 1);
}

// i modulo n (n >= 1), correct for negative i
__device__ __forceinline__ int mb_mod(int i, int n) {
    const int r = i % n;
    return r < 0 ? r + n : r;
}

// c[0..2] = the image of size (Ht, Wt) whose texels start at `base` of `texels`, at a finite (u, v), every operation rounded on its own:
//   u <- u - floorf(u), v likewise (repeat);  x = u W - 0.5,  y = (1 - v) H - 0.5;  x0 = floorf(x), fx = x - x0, y likewise;
//   the four neighbours at columns x0, x0 + 1 modulo W and rows y0, y0 + 1 modulo H;  a channel is t = byte / 255 correctly rounded;
//   a = t00 + (t10 - t00) fx (row y0),  b = t01 + (t11 - t01) fx (row y0 + 1),  c = a + (b - a) fy.
// THE bilinear tap of a texture and of a pyramid level.  Ht, Wt >= 1 and last >= 0: whatever the tables hold, no texel index leaves [0, last].
__device__ __forceinline__ void mb_bilinear(const unsigned* __restrict__ texels, long base, long last, int Ht, int Wt, float u, float v, float* c) {
    u = u - floorf(u);
    v = v - floorf(v);
    const float x = u * (float)Wt - 0.5f, y = (1.0f - v) * (float)Ht - 0.5f;
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int xa = mb_mod((int)fminf(xf, 2147483520.f), Wt), ya = mb_mod((int)fminf(yf, 2147483520.f), Ht);     // xf, yf >= -1
    const int xb = xa + 1 == Wt ? 0 : xa + 1, yb = ya + 1 == Ht ? 0 : ya + 1;
    const long ra = base + (long)ya * Wt, rb = base + (long)yb * Wt;
    const unsigned p00 = texels[min(max(ra + xa, 0L), last)], p10 = texels[min(max(ra + xb, 0L), last)];        // four independent loads
    const unsigned p01 = texels[min(max(rb + xa, 0L), last)], p11 = texels[min(max(rb + xb, 0L), last)];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t00 = mb_div((float)((p00 >> (8 * k)) & 255u), 255.f), t10 = mb_div((float)((p10 >> (8 * k)) & 255u), 255.f);
        const float t01 = mb_div((float)((p01 >> (8 * k)) & 255u), 255.f), t11 = mb_div((float)((p11 >> (8 * k)) & 255u), 255.f);
        const float a = t00 + (t10 - t00) * fx, b = t01 + (t11 - t01) * fx;
        c[k] = a + (b - a) * fy;
    }
}

__device__ __forceinline__ bool mb_finite(float x) { return fabsf(x) < INFINITY; }

// c[0..2] = texture t (0 <= t < T) at (u, v) by mb_bilinear; false, with c untouched, for a non-finite u or v.  The host validates the
// tables (1 <= H, W <= 2^24, tex_off the running sum of H W); whatever they hold, no texel index leaves [0, tex_off[T] - 1], and a
// texture without a texel reads as false.
__device__ __forceinline__ bool mb_tex_sample(const MeshBatch& m, int t, float u, float v, float* c) {
    const int Ht = m.tex_size[2 * t], Wt = m.tex_size[2 * t + 1];
    const long last = m.tex_off[m.T] - 1;
    if (!mb_finite(u) || !mb_finite(v) || Ht < 1 || Wt < 1 || last < 0) return false;
    mb_bilinear(m.texels, m.tex_off[t], last, Ht, Wt, u, v, c);
    return true;
}

// The number of levels of a texture of size (H0, W0), both >= 1: floor(log2(max(H0, W0))) + 1.
__device__ __forceinline__ int mb_mip_levels(int H0, int W0) { return 32 - __clz(max(H0, W0)); }

// Level l >= 0 of the chain of a texture of size (H0, W0): its size to Hl, Wl; returns where it starts, in texels from the chain's start.
__device__ __forceinline__ long mb_mip_level(int H0, int W0, int l, int& Hl, int& Wl) {
    long off = 0;
    for (int k = 0; k < l; ++k) off += (long)max(1, H0 >> k) * max(1, W0 >> k);
    Hl = max(1, H0 >> l);
    Wl = max(1, W0 >> l);
    return off;
}

// mb_tex_sample's rule on level l of the pyramid of texture t (0 <= t < T; l is clamped to the texture's levels), with that level's own
// (H_l, W_l): level 0 gives mb_tex_sample's bits.  Whatever the tables hold, no texel index leaves [0, mip_off[T] - 1]; a batch without a
// pyramid texel reads as false.
__device__ __forceinline__ bool mb_mip_sample(const MeshBatch& m, int t, int l, float u, float v, float* c) {
    const int H0 = m.tex_size[2 * t], W0 = m.tex_size[2 * t + 1];
    const long last = m.mip_off[m.T] - 1;
    if (!mb_finite(u) || !mb_finite(v) || H0 < 1 || W0 < 1 || last < 0) return false;
    int Hl, Wl;
    const long base = m.mip_off[t] + mb_mip_level(H0, W0, min(max(l, 0), mb_mip_levels(H0, W0) - 1), Hl, Wl);
    mb_bilinear(m.mip_texels, base, last, Hl, Wl, u, v, c);
    return true;
}

// Queue append.  EVERY lane of the wave must call this; one atomic add on *counter per wave, the slots in lane order.  Returns the
// slot of a lane with pred set (the caller checks it against the queue's capacity); the value means nothing in the other lanes.
__device__ __forceinline__ u64 mb_queue_slot(bool pred, u64* __restrict__ counter) {
    const u64 mask = __ballot(pred);
    if (!mask) return 0;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd(counter, (u64)__popcll(mask));
    return __shfl(base, leader) + (u64)__popcll(mask & ((1ULL << lane) - 1ULL));
}
