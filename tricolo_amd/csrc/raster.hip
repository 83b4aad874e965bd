// Multi-view rendering of a packed batch of triangle meshes (the renderer behind data/preprocess_all_data.py:44-82 of the reference,
// restated as a rasteriser: visibility by a 64-bit atomic max, flat Lambert shading).  The packed batch is the one mesh_batch.h lays out, with
// its materials; per (mesh, view) there is the camera: eye[3] and the 3 x 3 world-to-camera rotation R (row major).
// The kernel is DEFINED by its arithmetic; tricolo_amd/data/render.py restates it in torch and gives the same bits.
//
//   setup (per view and face, fp32, every operation rounded on its own - contraction is off in this file; a / b is the correctly
//   rounded quotient, formed as fl32(fl64(a) / fl64(b)): 53 >= 2 * 24 + 2 bits make the second rounding harmless):
//     q = v - eye;  p.k = (R[k][0] q.x + R[k][1] q.y) + R[k][2] q.z;  nz = -p.z (the camera looks down -z, +y is up)
//     a face with a vertex at nz < znear (or NaN) is dropped whole - there is NO near-plane clipping
//     xs = ((fx p.x) / nz + 1) (W / 2),  ys = (1 - (fy p.y) / nz) (H / 2)   with fy = fl32(1 / tan(yfov / 2)), fx = fl32(fy H / W), both
//                                                                           formed in float64 on the host; row 0 is the top
//     X = (int)rintf(256 xs), Y likewise (1/256 pixel, ties to even); |X| or |Y| > 2^20 drops the face
//   coverage: 2A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) in int64; 2A == 0 drops the face, 2A < 0 swaps vertices 1 and 2 (both sides
//     are visible).  Edge a -> b at the pixel centre P = (256 px + 128, 256 py + 128): E = (b.x - a.x)(P.y - a.y) - (b.y - a.y)(P.x - a.x),
//     E0 on 1 -> 2, E1 on 2 -> 0, E2 on 0 -> 1.  P is covered when every E > 0, or E == 0 on an edge that is top (dy == 0, dx > 0) or
//     left (dy < 0): two faces sharing an edge cover every pixel centre on it exactly once.
//   depth: d_i = 1 / nz_i;  l_i = fl32(E_i) / fl32(2A);  d = (l0 d0 + l1 d1) + l2 d2   (1 / z is linear on the screen; larger = nearer)
//   visibility: key = bits(d) << 32 | (0xFFFFFFFF - face), face local to the mesh; atomic max per pixel over a cleared u64 buffer.
//     d > 0, so the bits order like the values: the nearest face wins, at bit-equal depth the lower index - whatever the arrival order.
//   shading (per pixel, world space): c = (b - a) x (c - a) componentwise as mesh_sample.hip's areas, len = sqrt((cx^2 + cy^2) + cz^2)
//     correctly rounded, e = eye - a, the normal is turned toward the eye by the sign of (cx ex + cy ey) + cz ez; with the light
//     l = (0, 1, 0): ndl = max(+-cy / len, 0) (0 when len == 0), s = 0.1 + fl32(3 / pi) ndl, colour = clamp(Kd s, 0, 1),
//     u8 = floor(255 colour + 0.5); background 255.
//   textured shading (TRI_MESH_TEXTURES only; the batch's texture fields are laid out in mesh_batch.h): visibility is untouched.
//     The pixel's winning face is set up again (the snapped corners, d_i, 2A, the swap of corners 1 and 2 - their UVs swap with
//     them), its three edge functions are formed at this pixel's centre in int64 and l_k = fl32(E_k) / fl32(2A) as for the depth; then
//     w_k = l_k d_k,  d = (w0 + w1) + w2,  b_k = w_k / d (perspective-correct weights),  u = (b0 u0 + b1 u1) + b2 u2,  v likewise;
//     (u, v) is sampled by mb_tex_sample (mesh_batch.h: repeat wrap, bilinear over texel centres, no mip-maps) to c, and
//     colour = clamp((Kd c) s, 0, 1).  A face without a texture - by its material, by the NaN marker in its face_uv, or at a pixel
//     where u or v is not finite - takes the path above, Kd s, bit for bit.  Kd x texel is the MTL rule.
//   face colours (tri_mesh_face_colours, for the voxeliser; no camera, the UVs are used affinely): Kd times the mean of the four
//     samples at barycentric (1/3, 1/3, 1/3), (2/3, 1/6, 1/6), (1/6, 2/3, 1/6), (1/6, 1/6, 2/3) - u = (b0 u0 + b1 u1) + b2 u2 with the
//     fp32 constants RS_B13, RS_B23, RS_B16 - summed in that order and multiplied by 0.25f; Kd for a face without a texture or with
//     a sample that is not finite.
//   four samples per pixel (samples == 4 only; everything above is untouched by it): the positions, in 1/256 pixel from the
//     pixel's top-left corner, are sample 0 (96, 32), 1 (224, 96), 2 (32, 160), 3 (160, 224) - the 4x rotated grid; the centre (128, 128)
//     is not one of them.  Vertices are snapped to 1/256 pixel, so every position is an integer and coverage stays exact in int64.
//     Coverage, depth and the key of a sample are the rules above evaluated at P = (256 px + ox, 256 py + oy) instead of the centre:
//     the same face set-up (dropped faces, the swap, the snap range), E_k(sample) = E_k(centre) + (ox - 128)(-dy_k) + (oy - 128) dx_k,
//     the top-left rule, l_k = fl32(E_k) / fl32(2A), d = (l0 d0 + l1 d1) + l2 d2, an atomic max over u64 [N][views][H][W][4], the
//     sample innermost.  The box of candidate pixels holds every pixel with a sample inside the face's bounding box,
//     ceil((Xmin - 224) / 256) .. floor((Xmax - 32) / 256) - up to a pixel wider on each side than the box of centres; results are
//     defined by coverage, never by the box.  Every sample is coloured exactly as the pixel it would be above: 255 for none, u8 of
//     clamp(Kd s, 0, 1) for an untextured face, and for a textured one (u, v) from the edge functions AT THE SAMPLE'S OWN POSITION,
//     mb_tex_sample, clamp((Kd c) s, 0, 1), with the same fallback to Kd s.  The pixel is (c0 + c1 + c2 + c3 + 2) >> 2 per channel of the
//     four u8 colours: a multisample resolve for untextured faces, 4x supersampling for textured ones - no attribute is ever
//     extrapolated outside its face.  The visibility output is int32 [N][views][H][W][4], the face at each sample.
//   mip-mapped textures (tri_texture_mips builds the pyramid mesh_batch.h lays out - exact integer box means of level 0 - and
//     a TRI_MESH_MIPS render alone reads it; everything above is untouched by it, visibility included).  A definition of our own:
//     nobody has compared a pixel of it with pyrender's mip-mapping.  At a position P - the pixel centre, or a sample's own position
//     with four samples - where face f with texture t of size (H0, W0) and L levels won:
//     (u, v) and d at P exactly as above (l_k, w_k = l_k d_k, d, b_k, u, v); a (u, v) that is not finite leaves the face untextured there.
//     (u_x, v_x), d_x: the same arithmetic with the edge functions E_k + sx_k, one whole pixel to the right; (u_y, v_y), d_y with
//     E_k + sy_k, one whole pixel down.  The face's PLANE is extended beyond its edges for these two evaluations only; no colour is
//     ever taken there.  The differences are taken before the repeat wrap.  With four samples the step is still one whole pixel and
//     there is no LOD bias: every sample picks the level a pixel would.
//     a = (u_x - u) W0,  b = (v_x - v) H0,  c = (u_y - u) W0,  e = (v_y - v) H0  (W0, H0 as fp32);  r2 = max(a a + b b, c c + e e);
//     rho = sqrt(r2) correctly rounded.  Which levels:
//       d_x or d_y not above 0 (the plane crosses the eye), or one of u_x, v_x, u_y, v_y, r2 not finite: level L - 1 alone;
//       rho <= 1 (magnified): level 0 alone - bit for bit the colour of the textured shading above;
//       else l = floor(log2(rho)) from the exponent bits of rho, g = rho 2^-l - 1 in [0, 1) (the mantissa of rho under exponent 0,
//       minus 1: exact); l >= L - 1: level L - 1 alone; else per channel c = c_l + (c_{l+1} - c_l) g,
//     c_l = mb_mip_sample (mesh_batch.h) of level l at (u, v): mb_tex_sample's rule with the level's own (H_l, W_l).  g is linear in
//     rho, not its logarithm, so that every step is reproducible; the selection is continuous and monotone in rho - at rho = 1, at
//     every octave and at the top level - and within 0.087 of a level of the logarithm.  colour = clamp((Kd c) s, 0, 1) as above.
//   smooth shading (TRI_MESH_NORMALS only; the batch's corner normals face_vn are laid out in mesh_batch.h; everything above
//     is untouched by it, visibility included - the clear, faces and queue passes are the same kernels).  At a position P - the pixel
//     centre, or a sample's own position with four samples - where face f won and f has normals (its marker is not NaN):
//     the face is set up again, its edge functions are formed at P, and the perspective-correct weights are those of the textured
//     shading (rs_weights): l_k = fl32(E_k) / fl32(2A), w_k = l_k d_k, d = (w0 + w1) + w2, b_k = w_k / d;
//     n_j = (b0 n0_j + b1 n1_j) + b2 n2_j per component, corners 1 and 2 swapped with the face's vertices as the UVs are;
//     if an n_j is not finite, or len = sqrt((n_x^2 + n_y^2) + n_z^2) correctly rounded is 0, the position takes the flat shade s
//     above, bit for bit; otherwise e = eye - a with a the face's vertex 0 (the e of the flat shade), side = (n_x e_x + n_y e_y) + n_z e_z,
//     ndl = max(+-n_y / len, 0) with the sign of `side`, s = 0.1 + fl32(3 / pi) ndl, and the colour is formed exactly as above: u8 of
//     clamp(Kd s, 0, 1), or of clamp((Kd c) s, 0, 1) with the texel c of the textured and mip-mapped modes.  A face without normals
//     is shaded flat.  The interpolated normal is turned toward the eye per POSITION, as the flat one is per face, because neither
//     ShapeNet's winding nor its vn lines can be trusted: compared with one-sided lighting that brightens the last pixels before a
//     silhouette, where the interpolated normal already points away from the eye.  The turn is ours; so is the reading that the
//     reference's pyrender meshes are smooth-shaded (data/render.py).  With four samples an untextured face WITH normals is coloured
//     per sample - its shade varies across the pixel - and no longer once per face; a face without normals keeps that path.
//   the glTF metallic-roughness BRDF (TRI_MESH_PBR only; the batch's PBR factors mat_pbr are laid out in mesh_batch.h;
//     everything above is untouched by it, visibility included - the clear, faces and queue passes are the same kernels).  The formulas
//     are the glTF 2.0 specification's, the clamps of the cosines the Khronos glTF-WebGL-PBR reference shader's; that pyrender shades
//     this way is a reading from memory nobody has checked (data/render.py).  At a position P - the pixel centre, or a sample's own
//     position with four samples - where face f of mesh n won, every operation fp32 and rounded on its own, sums in the order written:
//     base_k per channel: what the modes above multiply the shade with - Kd, or Kd c with the texel c of the textured and mip-mapped
//       modes, with their fallbacks to Kd;
//     (m, r) = mb_face_pbr (mesh_batch.h): m = fminf(fmaxf(metallic, 0), 1), r = fminf(fmaxf(roughness, 0.04), 1) - a NaN takes the
//       lower bound - and (0.2, 0.8) for a mesh without materials;  alpha = r r,  a2 = alpha alpha;
//     n: the unit normal of the Lambert modes.  Flat: x = (b - a) x (c - a), len = sqrt((x_x^2 + x_y^2) + x_z^2), n_j = x_j / len, every
//       n_j negated when side = (x_x e_x + x_y e_y) + x_z e_z < 0 with e = eye - a.  Smooth, for a face with corner normals whose
//       interpolation at P is finite with len != 0 (the rule above): n_j = +-(interpolated n_j) / len by the sign of its own side.  The
//       Lambert shade at P is s = 0.1 + fl32(3 / pi) max(n_y, 0) (n_y = 0 for a flat len of 0) - the bits of the modes above;
//     b_k, d = rs_weights at P;  p_j = (b0 a_j + b1 b_j) + b2 c_j with the face's corners in the swapped order, as the UVs are;
//     q = eye - p,  dist = sqrt((q_x^2 + q_y^2) + q_z^2),  v_j = q_j / dist;  l = (0, 1, 0);  g = (v_x, 1 + v_y, v_z),
//     hl = sqrt((g_x^2 + g_y^2) + g_z^2),  h_j = g_j / hl;
//     NL = clamp(n_y, 0.001, 1),  NV = clamp(|(n_x v_x + n_y v_y) + n_z v_z|, 0.001, 1),  NH = clamp((n_x h_x + n_y h_y) + n_z h_z, 0, 1),
//     VH = clamp((v_x h_x + v_y h_y) + v_z h_z, 0, 1),  clamp(x, lo, hi) = fminf(fmaxf(x, lo), hi);
//     w = 1 - VH,  w5 = (((w w) w) w) w  (four multiplications);
//     g(x) = (2 x) / (x + sqrt(a2 + (1 - a2) (x x))),  G = g(NL) g(NV);   t = (NH NH) (a2 - 1) + 1,  D = a2 / ((pi t) t), pi = fl32(pi);
//     S = (G D) / ((4 NL) NV)  - the specular term without its Fresnel factor, one quotient for the three channels;
//     per channel  F0 = 0.04 + (base - 0.04) m,  cdiff = (0.96 base) (1 - m),  F = F0 + (1 - F0) w5,
//       colour = clamp(0.1 base + (3 NL) (((1 - F) cdiff) / pi + F S), 0, 1),  u8 = floor(255 colour + 0.5);  background 255.
//     No pow, exp or log; every root and quotient is the correctly rounded one (mb_sqrt, mb_div).
//     Fallback: where a b_k is not finite, dist or hl is zero or not finite, or the len of the normal in use is zero or not finite (or
//     the winner could not be set up again, which cannot happen), the position takes the Lambert colour u8(clamp(base s, 0, 1)) - what
//     the same batch without TRI_MESH_PBR writes there, bit for bit.
//     With four samples every sample of every face is coloured at its own position - v varies across the pixel, so the once-per-face
//     shortcut of untextured flat faces does not apply - and the pixel is still (c0 + c1 + c2 + c3 + 2) >> 2.
//
// Work: one lane per (view, face) sets the face up; a pixel box of at most RS_SMALL x RS_SMALL is rasterised by the lane itself, a
// larger one is appended to a device queue (one atomic add per wave, slots by ballot), and a second kernel on a fixed grid walks the
// queue - one workgroup per queued face, its lanes tiling the box - with the count it reads on the device.  No host synchronisation.
// Every mode is that one sequence (rs_render: clear, faces, queue, resolve), its kernels templates on the keys per pixel S, 1 or 4, and
// the resolve on the mode, on SMOOTH and on BRDF as well; the face set-up (rs_setup), a key (rs_pixel), the perspective-correct weights at a
// position (rs_weights) and (u, v, d) from them (rs_uvd), the texel of a face there (rs_texel, over mesh_batch.h's one bilinear tap),
// the smooth shade there (rs_smooth_shade), the metallic-roughness colour there (rs_brdf_u8, with the unit normals of rs_flat_normal and
// rs_smooth_normal) and a Lambert colour (rs_colour_u8) are each stated once for all of them.  With four
// samples the split is by the samples' box, and the two inner walks differ on purpose: the one-sample lane visits every pixel of its
// box; the four-sample lane moves a cursor over its box's samples to ITS next covered one with integer tests only - a pixel whose four
// samples all lie outside one edge (the largest of that edge's four offsets is still negative) is stepped over whole - and only then
// runs the quotients and the atomic, so a wave runs that body once per covered sample of its busiest lane, not once per sample of the
// box.  The queue kernel's lanes tile the box's samples, so neighbouring lanes touch neighbouring keys.
#include <math.h>
#include <stdio.h>

#include "mesh_batch.h"
#include "../../include/tricolo_hip.h"

#pragma clang fp contract(off)

#define RS_THREADS 256
#define RS_SMALL 8                              // boxes up to 8 x 8 pixel centres stay with their lane
#define RS_QUEUE_BLOCKS 4096                    // fixed grid of the queue kernel
#define RS_CLEAR_BLOCKS 2048
#define RS_SNAP_MAX 1048576.f                   // 2^20 in 1/256 pixel
#define RS_MAX_PIXELS (1L << 31)
#define RS_AA_LO 32                             // the leftmost / topmost and the rightmost / lowest of the four samples, in 1/256 pixel
#define RS_AA_HI 224
#define RS_KDIFF 0.95492965f                    // fl32(3 / pi): intensity 3, Lambert's 1 / pi
#define RS_PI 3.14159274f                       // fl32(pi)
#define RS_B13 0.33333334f                      // fl32(1 / 3), fl32(2 / 3), fl32(1 / 6): the sample positions of the face colours
#define RS_B23 0.6666667f
#define RS_B16 0.16666667f

struct RsFace {
    long A2, e[3];                              // doubled area (> 0); the edge functions at the centre of pixel (x0, y0)
    int sx[3], sy[3], bias[3];                  // their steps per pixel in x and y; 0 on a top / left edge, -1 otherwise
    float d[3];
    int x0, x1, y0, y1;                         // the box of pixel centres, clipped to the image
    int swap;                                   // 1 when vertices 1 and 2 changed places
};

// LO, HI: the box takes pixel px when 256 px + HI >= Xmin and 256 px + LO <= Xmax - (128, 128), the pixel centres, unless the caller
// says otherwise; the four-sample kernels say (32, 224), the leftmost / topmost and the rightmost / lowest sample.  o.e is taken at the
// centre of pixel (x0, y0) either way.
template <int LO = 128, int HI = 128>
__device__ __forceinline__ bool rs_setup(const MeshBatch& m, const float* __restrict__ cam, long gf, int n, long nv, int H, int W, float fx,
                                         float fy, float znear, RsFace& o) {
    const long v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    if (V <= 0) return false;
    const float* c = cam + (size_t)nv * 12;
    const int* fi = m.faces + (size_t)gf * 3;
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    int X[3], Y[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = mb_vertex(m, v0, V, fi[k]);
        const float qx = p[0] - c[0], qy = p[1] - c[1], qz = p[2] - c[2];
        const float px = (c[3] * qx + c[4] * qy) + c[5] * qz;
        const float py = (c[6] * qx + c[7] * qy) + c[8] * qz;
        const float nz = -((c[9] * qx + c[10] * qy) + c[11] * qz);
        const bool front = nz >= znear;                                 // false for NaN
        const float z = front ? nz : 1.f;
        const float xf = rintf(((mb_div(fx * px, z) + 1.0f) * hw) * 256.f);
        const float yf = rintf(((1.0f - mb_div(fy * py, z)) * hh) * 256.f);
        const bool in = fabsf(xf) <= RS_SNAP_MAX && fabsf(yf) <= RS_SNAP_MAX;
        ok = ok && front && in;
        X[k] = in ? (int)xf : 0;
        Y[k] = in ? (int)yf : 0;
        o.d[k] = mb_div(1.0f, z);
    }
    if (!ok) return false;
    long A2 = (long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long)(X[2] - X[0]) * (Y[1] - Y[0]);
    if (A2 == 0) return false;
    o.swap = A2 < 0;
    if (A2 < 0) {
        int t = X[1]; X[1] = X[2]; X[2] = t;
        t = Y[1]; Y[1] = Y[2]; Y[2] = t;
        const float s = o.d[1]; o.d[1] = o.d[2]; o.d[2] = s;
        A2 = -A2;
    }
    o.A2 = A2;
    o.x0 = max(0, (min(X[0], min(X[1], X[2])) + (255 - HI)) >> 8);      // ceil((X - HI) / 256): + 127 for the centres
    o.x1 = min(W - 1, (max(X[0], max(X[1], X[2])) - LO) >> 8);          // floor((X - LO) / 256): - 128
    o.y0 = max(0, (min(Y[0], min(Y[1], Y[2])) + (255 - HI)) >> 8);
    o.y1 = min(H - 1, (max(Y[0], max(Y[1], Y[2])) - LO) >> 8);
    if (o.x0 > o.x1 || o.y0 > o.y1) return false;
    const long Px = 256L * o.x0 + 128, Py = 256L * o.y0 + 128;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                       // edge k runs from vertex k + 1 to vertex k + 2
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const int dx = X[b] - X[a], dy = Y[b] - Y[a];
        o.e[k] = (long)dx * (Py - Y[a]) - (long)dy * (Px - X[a]);
        o.sx[k] = -256 * dy;                                            // |dx|, |dy| <= 2^21: the steps fit 32 bits
        o.sy[k] = 256 * dx;
        o.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
    }
    return true;
}

// Sample s of a pixel relative to its centre, in 1/256 pixel: (-32, -96), (96, -32), (-96, 32), (32, 96).
__device__ __forceinline__ int rs_sample_x(int s) { return s == 0 ? -32 : s == 1 ? 96 : s == 2 ? -96 : 32; }
__device__ __forceinline__ int rs_sample_y(int s) { return 64 * s - 96; }

// What edge k of f gains from the centre of a pixel to its sample s: (ox - 128)(-dy) + (oy - 128) dx.  sx = -256 dy and sy = 256 dx
// are exact multiples, |dx|, |dy| <= 2^21: below 2^29.
__device__ __forceinline__ int rs_sample_step(const RsFace& f, int k, int s) {
    return rs_sample_x(s) * (f.sx[k] >> 8) + rs_sample_y(s) * (f.sy[k] >> 8);
}

__device__ __forceinline__ void rs_pixel(const RsFace& f, long e0, long e1, long e2, u64* __restrict__ kp, unsigned low) {
    if (((e0 + f.bias[0]) | (e1 + f.bias[1]) | (e2 + f.bias[2])) < 0) return;
    const float fa = (float)(double)f.A2;
    const float l0 = mb_div((float)(double)e0, fa), l1 = mb_div((float)(double)e1, fa), l2 = mb_div((float)(double)e2, fa);
    const float d = (l0 * f.d[0] + l1 * f.d[1]) + l2 * f.d[2];
    const u64 key = ((u64)__float_as_uint(d) << 32) | low;
    if (*kp < key) atomicMax(kp, key);                                  // keys only grow: a stale read costs an atomic, never a pixel
}

// S below: the keys per pixel, 1 (the pixel centre; keys u64 [N][views][H][W]) or 4 (keys u64 [N][views][H][W][4]).  RS_LO(S), RS_HI(S): rs_setup's box.
#define RS_LO(S) ((S) == 4 ? RS_AA_LO : 128)
#define RS_HI(S) ((S) == 4 ? RS_AA_HI : 128)

// n stores of a K and the queue count.  K: a key with one sample, two keys at once with four - 16 bytes per lane and step, which the
// one-sample call does not take: its clear measured 4 us slower with them (profiles/r13/NOTES_one_rasteriser.md)
template <typename K>
__global__ __launch_bounds__(RS_THREADS) void raster_clear_kernel(K* __restrict__ keys, long n, u64* __restrict__ qcount) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *qcount = 0;
    for (long i = (long)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * RS_THREADS) keys[i] = K{};
}

// blockIdx.y = view, one lane per face of the whole batch; a lane keeps boxes of up to RS_SMALL x RS_SMALL pixels
template <int S>
__global__ __launch_bounds__(RS_THREADS) void raster_faces_kernel(MeshBatch m, const float* __restrict__ cam, long sumF, int views, int H, int W,
                                                                  float fx, float fy, float znear, u64* __restrict__ keys,
                                                                  u64* __restrict__ qcount, uint2* __restrict__ queue, u64 qcap) {
    const long gf = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    const int view = blockIdx.y;
    RsFace f;
    bool live = false, big = false;
    int n = 0;
    long nv = 0;
    if (gf < sumF) {
        n = mb_mesh_of(m, gf);
        nv = (long)n * views + view;
        live = rs_setup<RS_LO(S), RS_HI(S)>(m, cam, gf, n, nv, H, W, fx, fy, znear, f);
        big = live && (f.x1 - f.x0 >= RS_SMALL || f.y1 - f.y0 >= RS_SMALL);
    }
    const u64 slot = mb_queue_slot(big, qcount);                        // every lane of the wave is here
    if (big && slot < qcap) queue[slot] = make_uint2((unsigned)gf, (unsigned)view);
    if (!live || big) return;
    const unsigned low = 0xFFFFFFFFu - (unsigned)(gf - m.face_off[n]);
    u64* row = keys + ((size_t)nv * H + f.y0) * W * S;
    long r0 = f.e[0], r1 = f.e[1], r2 = f.e[2];
    if (S == 1) {
        for (int y = f.y0; y <= f.y1; ++y, row += W, r0 += f.sy[0], r1 += f.sy[1], r2 += f.sy[2]) {
            long e0 = r0, e1 = r1, e2 = r2;
            for (int x = f.x0; x <= f.x1; ++x, e0 += f.sx[0], e1 += f.sx[1], e2 += f.sx[2]) rs_pixel(f, e0, e1, e2, row + x, low);
        }
        return;
    }
    int top[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        top[k] = max(max(rs_sample_step(f, k, 0), rs_sample_step(f, k, 1)), max(rs_sample_step(f, k, 2), rs_sample_step(f, k, 3)));
    // A cursor (y, x, s) walks the box's samples row by row; r and e are the edge functions at the centres of pixel (x0, y) and (x, y).
    long e0 = r0, e1 = r1, e2 = r2;
    int x = f.x0, y = f.y0, s = 0;
    auto next_pixel = [&]() {
        s = 0;
        if (++x <= f.x1) { e0 += f.sx[0]; e1 += f.sx[1]; e2 += f.sx[2]; return; }
        x = f.x0; ++y; row += (size_t)W * 4;
        r0 += f.sy[0]; r1 += f.sy[1]; r2 += f.sy[2];
        e0 = r0; e1 = r1; e2 = r2;
    };
    while (y <= f.y1) {
        long c0 = 0, c1 = 0, c2 = 0;
        bool hit = false;
        while (y <= f.y1) {                                             // integer tests only: the lane stops at ITS next covered sample
            if (s == 0 && ((e0 + top[0]) | (e1 + top[1]) | (e2 + top[2])) < 0) { next_pixel(); continue; }   // all four outside one edge
            c0 = e0 + rs_sample_step(f, 0, s); c1 = e1 + rs_sample_step(f, 1, s); c2 = e2 + rs_sample_step(f, 2, s);
            hit = ((c0 + f.bias[0]) | (c1 + f.bias[1]) | (c2 + f.bias[2])) >= 0;
            if (hit) break;
            if (++s == 4) next_pixel();
        }
        if (!hit) break;
        rs_pixel(f, c0, c1, c2, row + 4 * (size_t)x + s, low);          // so the wave runs the quotients and the atomic once per covered sample
        if (++s == 4) next_pixel();
    }
}

// fixed grid; workgroup b takes queue entries b, b + gridDim.x, ... up to the count the first kernel left on the device.  The lanes tile
// the box's SAMPLES (RS_THREADS is a multiple of S: a lane keeps its sample s, whose step from the pixel's centre is 0 with one sample)
template <int S>
__global__ __launch_bounds__(RS_THREADS) void raster_queue_kernel(MeshBatch m, const float* __restrict__ cam, int views, int H, int W, float fx,
                                                                  float fy, float znear, u64* __restrict__ keys,
                                                                  const u64* __restrict__ qcount, const uint2* __restrict__ queue, u64 qcap) {
    const u64 count = min(*qcount, qcap);
    const int s = threadIdx.x % S;
    for (u64 q = blockIdx.x; q < count; q += gridDim.x) {
        const uint2 item = queue[q];
        const long gf = item.x;
        const int n = mb_mesh_of(m, gf);
        const long nv = (long)n * views + (int)item.y;
        RsFace f;
        if (!rs_setup<RS_LO(S), RS_HI(S)>(m, cam, gf, n, nv, H, W, fx, fy, znear, f)) continue;  // the same answer in every lane
        const unsigned low = 0xFFFFFFFFu - (unsigned)(gf - m.face_off[n]);
        const int bw = f.x1 - f.x0 + 1, cnt = bw * (f.y1 - f.y0 + 1);
        const long s0 = f.e[0] + (S == 1 ? 0 : rs_sample_step(f, 0, s)), s1 = f.e[1] + (S == 1 ? 0 : rs_sample_step(f, 1, s)),
                   s2 = f.e[2] + (S == 1 ? 0 : rs_sample_step(f, 2, s));
        u64* box = keys + (((size_t)nv * H + f.y0) * W + f.x0) * S + s;
        for (int i = threadIdx.x / S; i < cnt; i += RS_THREADS / S) {
            const int iy = i / bw, ix = i - iy * bw;
            rs_pixel(f, s0 + (long)ix * f.sx[0] + (long)iy * f.sy[0], s1 + (long)ix * f.sx[1] + (long)iy * f.sy[1],
                     s2 + (long)ix * f.sx[2] + (long)iy * f.sy[2], box + ((size_t)iy * W + ix) * S, low);
        }
    }
}

// The flat Lambert shade s of the face (a, b, c) seen from `eye` (the camera's first three values).
__device__ __forceinline__ float rs_shade(const float* a, const float* b, const float* c, const float* eye) {
    float x[3];
    mb_cross(a, b, c, x);
    const float len = mb_sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const float ex = eye[0] - a[0], ey = eye[1] - a[1], ez = eye[2] - a[2];
    const float side = (x[0] * ex + x[1] * ey) + x[2] * ez;
    float ndl = 0.f;
    if (len > 0.f) {
        const float ny = mb_div(x[1], len);
        ndl = fmaxf(side < 0.f ? -ny : ny, 0.f);
    }
    return 0.1f + RS_KDIFF * ndl;
}

// The edge functions of f at the centre of pixel (px, py); f.e holds them at the centre of pixel (x0, y0).
__device__ __forceinline__ void rs_edges(const RsFace& f, int px, int py, long* e) {
    const long dx = px - f.x0, dy = py - f.y0;
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = f.e[k] + dx * f.sx[k] + dy * f.sy[k];
}

// THE perspective-correct weights b0, b1, b2 and d of a face with fa = fl32(2A), where its edge functions are e[0..2]
__device__ __forceinline__ void rs_weights(const RsFace& f, float fa, const long* e, float& b0, float& b1, float& b2, float& d) {
    const float l0 = mb_div((float)(double)e[0], fa), l1 = mb_div((float)(double)e[1], fa), l2 = mb_div((float)(double)e[2], fa);
    const float w0 = l0 * f.d[0], w1 = l1 * f.d[1], w2 = l2 * f.d[2];
    d = (w0 + w1) + w2;
    b0 = mb_div(w0, d); b1 = mb_div(w1, d); b2 = mb_div(w2, d);
}

// THE (u, v) and d of a face with corner UVs q[0..5] (the swap applied) and fa = fl32(2A), where its edge functions are e[0..2]
__device__ __forceinline__ void rs_uvd(const RsFace& f, const float* q, float fa, const long* e, float& u, float& v, float& d) {
    float b0, b1, b2;
    rs_weights(f, fa, e, b0, b1, b2, d);
    u = (b0 * q[0] + b1 * q[2]) + b2 * q[4];
    v = (b0 * q[1] + b1 * q[3]) + b2 * q[5];
}

// true when global face gf carries corner normals: the marker face_vn[gf][0][0] is not NaN
__device__ __forceinline__ bool rs_has_vn(const MeshBatch& m, long gf) {
    const float n0 = m.face_vn[(size_t)gf * 9];
    return n0 == n0;
}

// The smooth Lambert shade of face gf (with corner normals; set up by the caller as f; a: its vertex 0) where its edge functions are
// e[0..2], seen from `eye`: the normal interpolated with the perspective-correct weights and turned toward the eye (head of this
// file).  Leaves `shade` - the caller's flat one - as it is where the interpolated normal is not finite or has no length.
__device__ __forceinline__ void rs_smooth_shade(const MeshBatch& m, const RsFace& f, long gf, const long* e, const float* a, const float* eye,
                                                float& shade) {
    const float* vn = m.face_vn + (size_t)gf * 9;
    const int i1 = f.swap ? 2 : 1, i2 = f.swap ? 1 : 2;
    float b0, b1, b2, d, n[3];
    rs_weights(f, (float)(double)f.A2, e, b0, b1, b2, d);
#pragma unroll
    for (int j = 0; j < 3; ++j) n[j] = (b0 * vn[j] + b1 * vn[3 * i1 + j]) + b2 * vn[3 * i2 + j];
    if (!(mb_finite(n[0]) && mb_finite(n[1]) && mb_finite(n[2]))) return;
    const float len = mb_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (len == 0.f) return;
    const float ex = eye[0] - a[0], ey = eye[1] - a[1], ez = eye[2] - a[2];
    const float side = (n[0] * ex + n[1] * ey) + n[2] * ez;
    const float ny = mb_div(n[1], len);
    shade = 0.1f + RS_KDIFF * fmaxf(side < 0.f ? -ny : ny, 0.f);
}

// The level of detail at a position with (u, v), d, from (ux, vx), dx one whole pixel to the right and (uy, vy), dy one whole pixel down
// (head of this file), for a texture of size (H0, W0): the level to sample; true when level lo + 1 is blended in by frac.
__device__ __forceinline__ bool rs_mip_lod(int H0, int W0, float u, float v, float ux, float vx, float dx, float uy, float vy, float dy, int& lo,
                                           float& frac) {
    const float a = (ux - u) * (float)W0, b = (vx - v) * (float)H0, g = (uy - u) * (float)W0, e = (vy - v) * (float)H0;
    const float r2 = fmaxf(a * a + b * b, g * g + e * e);
    const int top = mb_mip_levels(H0, W0) - 1;
    lo = top;                                                           // the footprint is unbounded: the coarsest level alone
    frac = 0.f;
    if (!(dx > 0.f && dy > 0.f && mb_finite(ux) && mb_finite(vx) && mb_finite(uy) && mb_finite(vy) && mb_finite(r2))) return false;
    const float rho = mb_sqrt(r2);
    if (rho <= 1.0f) { lo = 0; return false; }                          // magnified: the texture itself
    const unsigned bits = __float_as_uint(rho);                         // rho > 1 and finite: a normal number
    const int l = (int)(bits >> 23) - 127;
    if (l >= top) return false;
    lo = l;
    frac = __uint_as_float((bits & 0x007FFFFFu) | 0x3F800000u) - 1.0f;
    return true;
}

// The texture colour c[0..2] of face gf (texture t), set up by the caller as f, where its edge functions are e[0..2]: false where the
// face is untextured there.  MIP: from the pyramid, the level of detail from (u, v) there, one whole pixel to the right and one down.
template <bool MIP>
__device__ __forceinline__ bool rs_texel(const MeshBatch& m, const RsFace& f, long gf, int t, const long* e, float* c) {
    const float* uv = m.face_uv + (size_t)gf * 6;
    const int i1 = f.swap ? 2 : 1, i2 = f.swap ? 1 : 2;
    const float q[6] = {uv[0], uv[1], uv[2 * i1], uv[2 * i1 + 1], uv[2 * i2], uv[2 * i2 + 1]};
    const float fa = (float)(double)f.A2;
    float u, v, d;
    rs_uvd(f, q, fa, e, u, v, d);
    if (!MIP) return mb_tex_sample(m, t, u, v, c);
    if (!mb_finite(u) || !mb_finite(v)) return false;
    const int H0 = m.tex_size[2 * t], W0 = m.tex_size[2 * t + 1];
    if (H0 < 1 || W0 < 1) return false;
    const long ex[3] = {e[0] + f.sx[0], e[1] + f.sx[1], e[2] + f.sx[2]}, ey[3] = {e[0] + f.sy[0], e[1] + f.sy[1], e[2] + f.sy[2]};
    float ux, vx, dx, uy, vy, dy, frac;
    rs_uvd(f, q, fa, ex, ux, vx, dx);
    rs_uvd(f, q, fa, ey, uy, vy, dy);
    int lo;
    const bool two = rs_mip_lod(H0, W0, u, v, ux, vx, dx, uy, vy, dy, lo, frac);
    if (!mb_mip_sample(m, t, lo, u, v, c)) return false;
    if (two) {
        float h[3];
        if (!mb_mip_sample(m, t, lo + 1, u, v, h)) return false;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = c[k] + (h[k] - c[k]) * frac;
    }
    return true;
}

// c = u8 of clamp(kd s, 0, 1), the colour of a pixel or of a sample
__device__ __forceinline__ void rs_colour_u8(const float* kd, float shade, int* c) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float col = fminf(fmaxf(kd[k] * shade, 0.f), 1.f);
        c[k] = (int)(uint8_t)(int)floorf(255.f * col + 0.5f);
    }
}

// The unit flat normal n of the face (a, b, c), turned toward `eye`; n = 0 where the cross product has no length.  0.1 + RS_KDIFF
// fmaxf(n[1], 0) is rs_shade's value, bit for bit.  True when the length is above 0 and finite: the BRDF may use n.
__device__ __forceinline__ bool rs_flat_normal(const float* a, const float* b, const float* c, const float* eye, float* n) {
    float x[3];
    mb_cross(a, b, c, x);
    const float len = mb_sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const float ex = eye[0] - a[0], ey = eye[1] - a[1], ez = eye[2] - a[2];
    const float side = (x[0] * ex + x[1] * ey) + x[2] * ez;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float nj = len > 0.f ? mb_div(x[j], len) : 0.f;
        n[j] = side < 0.f ? -nj : nj;
    }
    return len > 0.f && mb_finite(len);
}

// The unit smooth normal of face gf (with corner normals; a: its vertex 0) from the weights b0, b1, b2 of rs_weights, turned toward
// `eye`: rs_smooth_shade's normal, so that 0.1 + RS_KDIFF fmaxf(n[1], 0) is its shade, bit for bit.  Leaves n and good - the caller's
// flat ones - as they are where the interpolated normal is not finite or has no length; good: the length is finite as well.
__device__ __forceinline__ void rs_smooth_normal(const MeshBatch& m, const RsFace& f, long gf, float b0, float b1, float b2, const float* a,
                                                 const float* eye, float* n, bool& good) {
    const float* vn = m.face_vn + (size_t)gf * 9;
    const int i1 = f.swap ? 2 : 1, i2 = f.swap ? 1 : 2;
    float x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = (b0 * vn[j] + b1 * vn[3 * i1 + j]) + b2 * vn[3 * i2 + j];
    if (!(mb_finite(x[0]) && mb_finite(x[1]) && mb_finite(x[2]))) return;
    const float len = mb_sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    if (len == 0.f) return;
    const float ex = eye[0] - a[0], ey = eye[1] - a[1], ez = eye[2] - a[2];
    const float side = (x[0] * ex + x[1] * ey) + x[2] * ez;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float nj = mb_div(x[j], len);
        n[j] = side < 0.f ? -nj : nj;
    }
    good = mb_finite(len);
}

__device__ __forceinline__ float rs_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// Smith-GGX for one direction: (2 x) / (x + sqrt(a2 + (1 - a2) (x x)))
__device__ __forceinline__ float rs_smith(float x, float a2) { return mb_div(2.f * x, x + mb_sqrt(a2 + (1.f - a2) * (x * x))); }

// THE metallic-roughness colour (head of this file) of a position with the weights b0, b1, b2 on the face with corners pa, pb, pc (the
// swap applied), the unit normal n, base colour `base` and the clamped factors (metal, rough), seen from `eye`: col[0..2] as u8 values.
// False, with col untouched, where the position falls back to the Lambert colour.
__device__ __forceinline__ bool rs_brdf_u8(const float* base, float metal, float rough, const float* n, const float* pa, const float* pb,
                                           const float* pc, float b0, float b1, float b2, const float* eye, int* col) {
    if (!(mb_finite(b0) && mb_finite(b1) && mb_finite(b2))) return false;
    float q[3], v[3], h[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = eye[j] - ((b0 * pa[j] + b1 * pb[j]) + b2 * pc[j]);
    const float dist = mb_sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    if (!(dist > 0.f && mb_finite(dist))) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = mb_div(q[j], dist);
    const float gx = v[0], gy = 1.0f + v[1], gz = v[2];
    const float hl = mb_sqrt((gx * gx + gy * gy) + gz * gz);
    if (!(hl > 0.f && mb_finite(hl))) return false;
    h[0] = mb_div(gx, hl); h[1] = mb_div(gy, hl); h[2] = mb_div(gz, hl);
    const float NL = rs_clamp(n[1], 0.001f, 1.f);
    const float NV = rs_clamp(fabsf((n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]), 0.001f, 1.f);
    const float NH = rs_clamp((n[0] * h[0] + n[1] * h[1]) + n[2] * h[2], 0.f, 1.f);
    const float VH = rs_clamp((v[0] * h[0] + v[1] * h[1]) + v[2] * h[2], 0.f, 1.f);
    const float w = 1.0f - VH, w5 = (((w * w) * w) * w) * w;
    const float alpha = rough * rough, a2 = alpha * alpha;
    const float G = rs_smith(NL, a2) * rs_smith(NV, a2);
    const float t = (NH * NH) * (a2 - 1.0f) + 1.0f;
    const float D = mb_div(a2, (RS_PI * t) * t);
    const float S = mb_div(G * D, (4.f * NL) * NV);
    const float light = 3.f * NL;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float F0 = 0.04f + (base[k] - 0.04f) * metal, cdiff = (0.96f * base[k]) * (1.0f - metal);
        const float F = F0 + (1.0f - F0) * w5;
        const float c = rs_clamp(0.1f * base[k] + light * (mb_div((1.0f - F) * cdiff, RS_PI) + F * S), 0.f, 1.f);
        col[k] = (int)(uint8_t)(int)floorf(255.f * c + 0.5f);
    }
    return true;
}

// one thread per pixel of a BRDF call, S keys per pixel: every position - the pixel centre, or each of the four samples - is coloured
// on its own by rs_brdf_u8, or where that falls back by rs_colour_u8 with the Lambert shade of the position; the pixel is the colour
// of its one position or the rounded integer mean of four.  A face met in the sample before is not set up again.
template <int S, bool TEX, bool MIP, bool SMOOTH>
__device__ __forceinline__ void rs_resolve_brdf(const MeshBatch& m, const float* __restrict__ cam, int views, int H, int W, long npix, float fx,
                                                float fy, float znear, const u64* __restrict__ keys, uint8_t* __restrict__ image,
                                                int* __restrict__ visibility) {
    const long i = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= npix) return;
    const int HW = H * W;
    const long nv = i / HW;
    const int pix = (int)(i - nv * HW), n = (int)(nv / views);
    u64 key4[4] = {0, 0, 0, 0};
    if (S == 4) {
        const ulonglong2* kp = (const ulonglong2*)(keys + 4 * (size_t)i);           // the workspace is 16-byte aligned
        const ulonglong2 ka = kp[0], kb = kp[1];
        key4[0] = ka.x; key4[1] = ka.y; key4[2] = kb.x; key4[3] = kb.y;
    } else {
        key4[0] = keys[i];
    }
    const float* eye = cam + (size_t)nv * 12;
    const long f0 = m.face_off[n], F = m.face_off[n + 1] - f0, v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    int sum[3] = {S == 4 ? 2 : 0, S == 4 ? 2 : 0, S == 4 ? 2 : 0}, t = -1;
    long prev = -1, centre[3] = {0, 0, 0};
    float kd[3] = {0.f, 0.f, 0.f}, flat[3] = {0.f, 0.f, 0.f}, metal = 0.f, rough = 0.f;
    bool set = false, vn = false, flat_good = false;
    const float *pa = m.verts, *pb = m.verts, *pc = m.verts;
    RsFace f;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        const u64 key = s == 0 ? key4[0] : s == 1 ? key4[1] : s == 2 ? key4[2] : key4[3];
        const long lf = (long)(0xFFFFFFFFu - (unsigned)key);
        const bool none = key == 0 || lf >= F || V <= 0;
        if (visibility) visibility[(size_t)S * i + s] = none ? -1 : (int)lf;
        if (none) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sum[k] += 255;
            continue;
        }
        if (lf != prev) {
            prev = lf;
            const int* fi = m.faces + (size_t)(f0 + lf) * 3;
            pa = mb_vertex(m, v0, V, fi[0]);
            const float *p1 = mb_vertex(m, v0, V, fi[1]), *p2 = mb_vertex(m, v0, V, fi[2]);
            flat_good = rs_flat_normal(pa, p1, p2, eye, flat);
            mb_face_kd(m, n, f0 + lf, kd);
            mb_face_pbr(m, n, f0 + lf, metal, rough);
            if (SMOOTH) vn = rs_has_vn(m, f0 + lf);
            if (TEX) t = mb_face_tex(m, n, f0 + lf);
            set = rs_setup<RS_LO(S), RS_HI(S)>(m, cam, f0 + lf, n, nv, H, W, fx, fy, znear, f);       // the winner: true
            if (set) rs_edges(f, pix % W, pix / W, centre);
            pb = set && f.swap ? p2 : p1;
            pc = set && f.swap ? p1 : p2;
        }
        float c[3], base[3] = {kd[0], kd[1], kd[2]}, nrm[3] = {flat[0], flat[1], flat[2]};
        bool good = flat_good;
        int col[3];
        bool done = false;
        if (set) {
            const long e[3] = {centre[0] + (S == 1 ? 0 : rs_sample_step(f, 0, s)), centre[1] + (S == 1 ? 0 : rs_sample_step(f, 1, s)),
                               centre[2] + (S == 1 ? 0 : rs_sample_step(f, 2, s))};
            float b0, b1, b2, d;
            rs_weights(f, (float)(double)f.A2, e, b0, b1, b2, d);
            if (vn) rs_smooth_normal(m, f, f0 + lf, b0, b1, b2, pa, eye, nrm, good);
            if (t >= 0 && rs_texel<MIP>(m, f, f0 + lf, t, e, c)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) base[k] = kd[k] * c[k];
            }
            done = good && rs_brdf_u8(base, metal, rough, nrm, pa, pb, pc, b0, b1, b2, eye, col);
        }
        if (!done) rs_colour_u8(base, 0.1f + RS_KDIFF * fmaxf(nrm[1], 0.f), col);
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += col[k];
    }
    uint8_t* out = image + (size_t)nv * 3 * HW + pix;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)k * HW] = (uint8_t)(S == 4 ? sum[k] >> 2 : sum[k]);
}

// one thread per pixel: the winning face's flat Lambert colour, 255 where nothing was drawn.  TEX: the textured resolve pass - the
// lanes of a wave whose face has a texture set it up again and run rs_texel together, the others wait for them and keep their Kd.
// SMOOTH: a face with corner normals is set up again as well and takes rs_smooth_shade at the pixel centre.
template <bool TEX, bool MIP, bool SMOOTH>
__device__ __forceinline__ void rs_resolve(const MeshBatch& m, const float* __restrict__ cam, int views, int H, int W, long npix, float fx, float fy,
                                           float znear, const u64* __restrict__ keys, uint8_t* __restrict__ image, int* __restrict__ visibility) {
    const long i = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= npix) return;
    const int HW = H * W;
    const long nv = i / HW;
    const int pix = (int)(i - nv * HW), n = (int)(nv / views);
    const u64 key = keys[i];
    uint8_t* out = image + (size_t)nv * 3 * HW + pix;
    const long f0 = m.face_off[n], F = m.face_off[n + 1] - f0, v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    const long lf = (long)(0xFFFFFFFFu - (unsigned)key);
    if (key == 0 || lf >= F || V <= 0) {
        out[0] = 255; out[HW] = 255; out[2 * (size_t)HW] = 255;
        if (visibility) visibility[i] = -1;
        return;
    }
    if (visibility) visibility[i] = (int)lf;
    const int* fi = m.faces + (size_t)(f0 + lf) * 3;
    const float* a = mb_vertex(m, v0, V, fi[0]);
    float shade = rs_shade(a, mb_vertex(m, v0, V, fi[1]), mb_vertex(m, v0, V, fi[2]), cam + (size_t)nv * 12);
    float kd[3];
    mb_face_kd(m, n, f0 + lf, kd);
    if (TEX || SMOOTH) {
        const int t = TEX ? mb_face_tex(m, n, f0 + lf) : -1;
        const bool vn = SMOOTH && rs_has_vn(m, f0 + lf);
        RsFace f;
        if ((t >= 0 || vn) && rs_setup(m, cam, f0 + lf, n, nv, H, W, fx, fy, znear, f)) {    // the winner of a pixel was set up before: true
            long e[3];
            float c[3];
            rs_edges(f, pix % W, pix / W, e);
            if (vn) rs_smooth_shade(m, f, f0 + lf, e, a, cam + (size_t)nv * 12, shade);
            if (t >= 0 && rs_texel<MIP>(m, f, f0 + lf, t, e, c)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) kd[k] = kd[k] * c[k];
            }
        }
    }
    int col[3];
    rs_colour_u8(kd, shade, col);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)k * HW] = (uint8_t)col[k];
}

// one thread per pixel of the four-sample key buffer: every sample is coloured as rs_resolve colours a pixel - a textured face from (u, v)
// at the sample's own position - and the pixel is the rounded integer mean.  A face met in the sample before is not shaded or set up
// again, and an untextured one keeps its colour.  SMOOTH: a face with corner normals is shaded per sample, by rs_smooth_shade at the
// sample's own position, textured or not; a face without them keeps the once-per-face path.
template <bool TEX, bool MIP, bool SMOOTH>
__device__ __forceinline__ void rs_resolve_aa(const MeshBatch& m, const float* __restrict__ cam, int views, int H, int W, long npix, float fx,
                                              float fy, float znear, const u64* __restrict__ keys, uint8_t* __restrict__ image,
                                              int* __restrict__ visibility) {
    const long i = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= npix) return;
    const int HW = H * W;
    const long nv = i / HW;
    const int pix = (int)(i - nv * HW), n = (int)(nv / views);
    const ulonglong2* kp = (const ulonglong2*)(keys + 4 * (size_t)i);               // the workspace is 16-byte aligned
    const ulonglong2 ka = kp[0], kb = kp[1];
    const long f0 = m.face_off[n], F = m.face_off[n + 1] - f0, v0 = m.vert_off[n], V = m.vert_off[n + 1] - v0;
    int sum[3] = {2, 2, 2}, col[3] = {255, 255, 255}, t = -1;
    long prev = -1, centre[3] = {0, 0, 0};
    float shade = 0.f, kd[3] = {0.f, 0.f, 0.f};
    bool set = false, vn = false;
    const float* a = m.verts;
    RsFace f;
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        const u64 key = s == 0 ? ka.x : s == 1 ? ka.y : s == 2 ? kb.x : kb.y;
        const long lf = (long)(0xFFFFFFFFu - (unsigned)key);
        const bool none = key == 0 || lf >= F || V <= 0;
        if (visibility) visibility[4 * (size_t)i + s] = none ? -1 : (int)lf;
        if (none) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sum[k] += 255;
            continue;
        }
        if (lf != prev) {
            prev = lf;
            const int* fi = m.faces + (size_t)(f0 + lf) * 3;
            a = mb_vertex(m, v0, V, fi[0]);
            shade = rs_shade(a, mb_vertex(m, v0, V, fi[1]), mb_vertex(m, v0, V, fi[2]), cam + (size_t)nv * 12);
            mb_face_kd(m, n, f0 + lf, kd);
            if (SMOOTH) vn = rs_has_vn(m, f0 + lf);
            if (TEX || SMOOTH) {
                if (TEX) t = mb_face_tex(m, n, f0 + lf);
                if (t >= 0 || vn) {
                    set = rs_setup<RS_AA_LO, RS_AA_HI>(m, cam, f0 + lf, n, nv, H, W, fx, fy, znear, f);     // the winner: true
                    rs_edges(f, pix % W, pix / W, centre);
                }
            }
            if (t < 0 && !vn) rs_colour_u8(kd, shade, col);
        }
        if (t >= 0 || vn) {
            float c[3], kc[3] = {kd[0], kd[1], kd[2]}, sh = shade;
            const long e[3] = {centre[0] + rs_sample_step(f, 0, s), centre[1] + rs_sample_step(f, 1, s), centre[2] + rs_sample_step(f, 2, s)};
            if (vn && set) rs_smooth_shade(m, f, f0 + lf, e, a, cam + (size_t)nv * 12, sh);
            if (t >= 0 && set && rs_texel<MIP>(m, f, f0 + lf, t, e, c)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) kc[k] = kd[k] * c[k];
            }
            rs_colour_u8(kc, sh, col);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += col[k];
    }
    uint8_t* out = image + (size_t)nv * 3 * HW + pix;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)k * HW] = (uint8_t)(sum[k] >> 2);
}

// the resolve kernel of S keys per pixel; TEX, MIP: the mode of the call; SMOOTH: the batch carries corner normals (m.face_vn); BRDF:
// it carries PBR factors (m.mat_pbr) and is coloured by the metallic-roughness BRDF
template <int S, bool TEX, bool MIP, bool SMOOTH, bool BRDF>
__global__ __launch_bounds__(RS_THREADS) void raster_resolve_kernel(MeshBatch m, const float* __restrict__ cam, int views, int H, int W, long npix,
                                                                    float fx, float fy, float znear, const u64* __restrict__ keys,
                                                                    uint8_t* __restrict__ image, int* __restrict__ visibility) {
    if (BRDF) rs_resolve_brdf<S, TEX, MIP, SMOOTH>(m, cam, views, H, W, npix, fx, fy, znear, keys, image, visibility);
    else if (S == 4) rs_resolve_aa<TEX, MIP, SMOOTH>(m, cam, views, H, W, npix, fx, fy, znear, keys, image, visibility);
    else rs_resolve<TEX, MIP, SMOOTH>(m, cam, views, H, W, npix, fx, fy, znear, keys, image, visibility);
}

// one lane per face of the whole batch: out fp32 [sumF][3], the colour the voxeliser takes for the face
__global__ __launch_bounds__(RS_THREADS) void mesh_face_colours_kernel(MeshBatch m, long sumF, float* __restrict__ out) {
    const long gf = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (gf >= sumF) return;
    const int n = mb_mesh_of(m, gf);
    float kd[3];
    mb_face_kd(m, n, gf, kd);
    const int t = mb_face_tex(m, n, gf);
    if (t >= 0) {
        const float* uv = m.face_uv + (size_t)gf * 6;
        const float bary[4][3] = {{RS_B13, RS_B13, RS_B13}, {RS_B23, RS_B16, RS_B16}, {RS_B16, RS_B23, RS_B16}, {RS_B16, RS_B16, RS_B23}};
        float c[4][3];
        bool ok = true;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            ok = mb_tex_sample(m, t, (bary[s][0] * uv[0] + bary[s][1] * uv[2]) + bary[s][2] * uv[4],
                               (bary[s][0] * uv[1] + bary[s][1] * uv[3]) + bary[s][2] * uv[5], c[s]) && ok;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) kd[k] = kd[k] * ((((c[0][k] + c[1][k]) + c[2][k]) + c[3][k]) * 0.25f);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)gf * 3 + k] = kd[k];
}

// ---- the mip pyramid (mesh_batch.h lays it out and states the texel rule) ----
#define MIP_LANE_LEVELS 3                       // levels 0 .. 2 take one lane per texel (a footprint of at most 9 x 9), the others a wave
// The part of S = sum_i sum_j wy(i) wx(j) texel0[i][j][k], k = R, G, B, of texel (y, x) of a level of size (Hl, Wl) that falls to the rows
// i0 + li, i0 + li + si, ... and the columns j0 + lj, j0 + lj + sj, ... of its footprint.  src: level 0; reads stay in [0, last].
__device__ __forceinline__ void mip_partial(const unsigned* __restrict__ texels, long src, long last, int H0, int W0, int Hl, int Wl, int y, int x,
                                            int li, int si, int lj, int sj, long* S) {
    const long ya = (long)y * H0, yb = ya + H0, xa = (long)x * W0, xb = xa + W0;    // the texel's span in units of 1 / (H0 Hl), 1 / (W0 Wl)
    const long i0 = ya / Hl, i1 = (yb - 1) / Hl, j0 = xa / Wl, j1 = (xb - 1) / Wl;
    for (long i = i0 + li; i <= i1; i += si) {
        const long wy = max(0L, min(yb, (i + 1) * Hl) - max(ya, i * Hl));
        const long row = src + i * W0;
        u64 r[3] = {0, 0, 0};
        for (long j = j0 + lj; j <= j1; j += sj) {
            const unsigned wx = (unsigned)max(0L, min(xb, (j + 1) * Wl) - max(xa, j * Wl));     // at most Wl <= 2^24: wx byte fits 32 bits
            const unsigned p = texels[min(max(row + j, 0L), last)];
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k] += (u64)(wx * ((p >> (8 * k)) & 255u));
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) S[k] += wy * (long)r[k];
    }
}

// blockIdx.y strides over the textures, the waves of blockIdx.x over the work items of a texture's chain: first the texels of levels
// 0 .. MIP_LANE_LEVELS - 1 in groups of 64, a lane each, then every texel of the coarser levels, a wave each - its lanes tile the
// footprint 8 x 8 and the integer sums, which do not depend on the order, are reduced across the wave.  One dword store per texel.
__global__ __launch_bounds__(RS_THREADS) void texture_mips_kernel(const unsigned* __restrict__ texels, const long* __restrict__ tex_off,
                                                                  const int* __restrict__ tex_size, int T, long sum_texels,
                                                                  const long* __restrict__ mip_off, long sum_mip, unsigned* __restrict__ mip) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long last = min(tex_off[T], sum_texels) - 1, end = min(mip_off[T], sum_mip);
    if (last < 0) return;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const int H0 = tex_size[2 * t], W0 = tex_size[2 * t + 1];
        if (H0 < 1 || W0 < 1) continue;
        const long src = tex_off[t], dst = mip_off[t], D = (long)H0 * W0;
        const int L = mb_mip_levels(H0, W0);
        long fine = 0, all = 0;                                         // the texels of the lane levels, of the whole chain
        for (int l = 0; l < L; ++l) {
            const long sz = (long)max(1, H0 >> l) * max(1, W0 >> l);
            all += sz;
            if (l < MIP_LANE_LEVELS) fine += sz;
        }
        const long groups = (fine + 63) >> 6, items = groups + (all - fine);
        for (long item = (long)blockIdx.x * (RS_THREADS / 64) + wave; item < items; item += (long)gridDim.x * (RS_THREADS / 64)) {
            const bool wide = item >= groups;                           // the same in every lane of the wave
            const long c = wide ? fine + (item - groups) : item * 64 + lane;        // the texel, counted from the chain's start
            if (!wide && c >= fine) continue;
            int l = 0;
            long start = 0, sz = D;
            while (l < L - 1 && c >= start + sz) {
                start += sz;
                ++l;
                sz = (long)max(1, H0 >> l) * max(1, W0 >> l);
            }
            const int Hl = max(1, H0 >> l), Wl = max(1, W0 >> l);
            const int y = (int)((c - start) / Wl), x = (int)((c - start) - (long)y * Wl);
            const long at = dst + c;
            const bool writes = (wide ? lane == 0 : true) && at >= 0 && at < end;
            if (l == 0) {                                               // level 0: the texture itself
                if (writes) mip[at] = texels[min(max(src + c, 0L), last)];
                continue;
            }
            long S[3] = {0, 0, 0};
            if (wide) {
                mip_partial(texels, src, last, H0, W0, Hl, Wl, y, x, lane >> 3, 8, lane & 7, 8, S);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    for (int o = 32; o > 0; o >>= 1) S[k] += __shfl_xor(S[k], o);
            } else {
                mip_partial(texels, src, last, H0, W0, Hl, Wl, y, x, 0, 1, 0, 1, S);
            }
            if (writes) {
                unsigned p = 0xFF000000u;
#pragma unroll
                for (int k = 0; k < 3; ++k) p |= ((unsigned)((2 * S[k] + D) / (2 * D)) & 255u) << (8 * k);
                mip[at] = p;
            }
        }
    }
}

static bool rs_sizes_ok(long sumF, int N, int views, int H, int W) {
    return N >= 0 && sumF >= 0 && views >= 0 && H >= 0 && W >= 0;
}

static bool rs_samples_ok(int samples) { return samples == 1 || samples == 4; }

// keys (samples per pixel) | queue count (padded to 16 bytes) | queue; 0 for what tri_raster_render refuses by its sizes.  Four samples
// are four keys per pixel, so fewer than 2^31 SAMPLES.
extern "C" size_t tri_raster_workspace(long sumF, int N, int views, int H, int W, int samples) {
    if (!rs_samples_ok(samples) || !rs_sizes_ok(sumF, N, views, H, W) || (double)N * views * H * W * (double)samples >= (double)RS_MAX_PIXELS) return 0;
    return (size_t)N * views * H * W * samples * 8 + 16 + (size_t)sumF * views * 8;
}

// What every launch refuses before anything runs; samples: keys per pixel, 1 or 4.
static int rs_check(int N, long sumF, int views, int H, int W, double yfov, double znear, int samples, const char* who) {
    char msg[200];
    if (!rs_sizes_ok(sumF, N, views, H, W)) { snprintf(msg, sizeof msg, "%s: negative size", who); tri_set_error(msg); return TRI_ERR_ARG; }
    if (!(yfov > 0.0 && yfov < M_PI) || !(znear > 0.0)) {
        snprintf(msg, sizeof msg, "%s: yfov must lie in (0, pi) and znear above 0", who); tri_set_error(msg); return TRI_ERR_ARG;
    }
    if (sumF >= (1L << 31)) { snprintf(msg, sizeof msg, "%s: 2^31 or more faces in a batch", who); tri_set_error(msg); return TRI_ERR_UNSUPPORTED; }
    if (views > 65535) { snprintf(msg, sizeof msg, "%s: more than 65535 views", who); tri_set_error(msg); return TRI_ERR_UNSUPPORTED; }
    if ((double)N * views * H * W * (double)samples >= (double)RS_MAX_PIXELS) {
        if (samples == 1) snprintf(msg, sizeof msg, "%s: 2^31 or more pixels (a visibility buffer of 16 GiB or more) in one launch", who);
        else snprintf(msg, sizeof msg, "%s: 2^31 or more samples (four per pixel; a visibility buffer of 16 GiB or more) in one launch - "
                      "split the batch", who);
        tri_set_error(msg);
        return TRI_ERR_UNSUPPORTED;
    }
    return TRI_OK;
}

enum { RS_PLAIN = 0, RS_TEX = 1, RS_MIP = 2 };   // which resolve kernel colours the pixels

typedef void (*RsResolve)(MeshBatch, const float*, int, int, int, long, float, float, float, const u64*, uint8_t*, int*);

// THE launch sequence: clear, faces, queue, resolve, with `samples` keys per pixel (1 or 4).  A batch without textures (T == 0) takes
// the plain resolve whatever the mode: mb_face_tex finds no texture in it.  A batch with corner normals (m.face_vn) takes the SMOOTH
// resolve of its mode, one with PBR factors (m.mat_pbr) the BRDF resolve; the three passes before it are the same kernels either way.
static int rs_render(const MeshBatch& m, int mode, int samples, const float* cam, long sumF, int views, int H, int W, double yfov, double znear,
                     void* workspace, uint8_t* image, int* visibility, void* stream, const char* who) {
#define RS_MODES(S, SMOOTH, BRDF) \
    {raster_resolve_kernel<S, false, false, SMOOTH, BRDF>, raster_resolve_kernel<S, true, false, SMOOTH, BRDF>, raster_resolve_kernel<S, true, true, SMOOTH, BRDF>}
    static const RsResolve resolve[2][2][2][3] = {{{RS_MODES(1, false, false), RS_MODES(4, false, false)}, {RS_MODES(1, true, false), RS_MODES(4, true, false)}},
                                                  {{RS_MODES(1, false, true), RS_MODES(4, false, true)}, {RS_MODES(1, true, true), RS_MODES(4, true, true)}}};
#undef RS_MODES
    const int N = m.N;
    const int bad = rs_check(N, sumF, views, H, W, yfov, znear, samples, who);
    if (bad != TRI_OK) return bad;
    const long npix = (long)N * views * H * W, nkeys = npix * samples;
    if (npix == 0) return TRI_OK;
    const bool aa = samples == 4;
    hipStream_t st = (hipStream_t)stream;
    u64* keys = (u64*)workspace;
    u64* qcount = keys + nkeys;
    uint2* queue = (uint2*)(qcount + 2);
    const u64 qcap = (u64)sumF * views;
    const double fyd = 1.0 / tan(yfov / 2.0);
    const float fy = (float)fyd, fx = (float)(fyd * (double)H / (double)W), zn = (float)znear;
    const long stores = aa ? nkeys / 2 : nkeys;
    const unsigned clear = (unsigned)min((long)RS_CLEAR_BLOCKS, (stores + RS_THREADS - 1) / RS_THREADS);
    if (aa) raster_clear_kernel<<<clear, RS_THREADS, 0, st>>>((ulonglong2*)keys, stores, qcount);      // the workspace is 16-byte aligned
    else raster_clear_kernel<<<clear, RS_THREADS, 0, st>>>(keys, stores, qcount);
    if (sumF > 0) {
        (aa ? raster_faces_kernel<4> : raster_faces_kernel<1>)<<<dim3((unsigned)((sumF + RS_THREADS - 1) / RS_THREADS), (unsigned)views),
                                                                 RS_THREADS, 0, st>>>(m, cam, sumF, views, H, W, fx, fy, zn, keys, qcount, queue, qcap);
        (aa ? raster_queue_kernel<4> : raster_queue_kernel<1>)<<<RS_QUEUE_BLOCKS, RS_THREADS, 0, st>>>(m, cam, views, H, W, fx, fy, zn, keys, qcount,
                                                                                                       queue, qcap);
    }
    resolve[m.mat_pbr != nullptr][m.face_vn != nullptr][aa][m.T > 0 ? mode : RS_PLAIN]<<<(unsigned)((npix + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0, st>>>(m, cam, views, H, W, npix, fx, fy,
                                                                                                                    zn, keys, image, visibility);
    return tri_check_launch(who);
}

// THE render entry point: the batch's declared groups choose the resolve kernel (rs_render), TRI_MESH_MIPS and TRI_MESH_TEXTURES the mode.
extern "C" int tri_raster_render(const TriMeshBatch* batch, const float* cam, long sumF, int views, int H, int W, double yfov, double znear,
                                 int samples, void* workspace, uint8_t* image, int* visibility, void* stream) {
    const char* who = "tri_raster_render";
    if (!rs_samples_ok(samples)) { tri_set_error("tri_raster_render: samples must be 1 or 4"); return TRI_ERR_ARG; }
    MeshBatch m;
    const int bad = mb_from_abi(batch, who, TRI_MESH_TEXTURES | TRI_MESH_MIPS | TRI_MESH_NORMALS | TRI_MESH_PBR, &m);
    if (bad != TRI_OK) return bad;
    const int mode = (batch->fields & TRI_MESH_MIPS) ? RS_MIP : (batch->fields & TRI_MESH_TEXTURES) ? RS_TEX : RS_PLAIN;
    return rs_render(m, mode, samples, cam, sumF, views, H, W, yfov, znear, workspace, image, visibility, stream, who);
}

extern "C" int tri_texture_mips(const uint8_t* texels, const long* tex_off, const int* tex_size, int T, long sum_texels, const long* mip_off,
                                long sum_mip, uint8_t* mip_texels, void* stream) {
    if (T < 0 || sum_texels < 0 || sum_mip < 0) { tri_set_error("tri_texture_mips: negative size"); return TRI_ERR_ARG; }
    if (T == 0 || sum_mip == 0) return TRI_OK;                          // an empty pyramid
    if (!texels || !tex_off || !tex_size || !mip_off || !mip_texels || sum_texels == 0) {
        tri_set_error("tri_texture_mips: T > 0 needs the texels, both offset tables, the sizes and the output");
        return TRI_ERR_ARG;
    }
    if (sum_mip < sum_texels) { tri_set_error("tri_texture_mips: a pyramid holds at least the texels of its level 0"); return TRI_ERR_ARG; }
    const unsigned gx = (unsigned)min(1024L, sum_mip / T / 128 + 1), gy = (unsigned)min(T, 256);
    texture_mips_kernel<<<dim3(gx, gy), RS_THREADS, 0, (hipStream_t)stream>>>((const unsigned*)texels, tex_off, tex_size, T, sum_texels, mip_off,
                                                                              sum_mip, (unsigned*)mip_texels);
    return tri_check_launch("tri_texture_mips");
}

extern "C" int tri_mesh_face_colours(const TriMeshBatch* batch, long sumF, float* colours, void* stream) {
    MeshBatch m;
    const int bad = mb_from_abi(batch, "tri_mesh_face_colours", TRI_MESH_TEXTURES, &m);
    if (bad != TRI_OK) return bad;
    if (sumF < 0) { tri_set_error("tri_mesh_face_colours: negative size"); return TRI_ERR_ARG; }
    if (sumF >= (1L << 31)) { tri_set_error("tri_mesh_face_colours: 2^31 or more faces in a batch"); return TRI_ERR_UNSUPPORTED; }
    if (sumF == 0 || m.N == 0) return TRI_OK;
    mesh_face_colours_kernel<<<(unsigned)((sumF + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0, (hipStream_t)stream>>>(m, sumF, colours);
    return tri_check_launch("tri_mesh_face_colours");
}
