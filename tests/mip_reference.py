"""An independent statement of the mip-mapped textures of csrc/raster.hip (ops.texture_mips, ops.render_views_textured(..., mips=))
for the tests.  It shares no code with tricolo_amd/data/render.py beyond what tests/texture_reference.py already shares (the vertices'
snapped integer screen positions); visibility comes from the float64 brute forces of tests/raster_reference.py (one sample) and
tests/antialias_reference.py (four), the bilinear sample and the Lambert shade from tests/texture_reference.py.

The pyramid, in Python integers and fractions from the interval-overlap definition: level l of a texture of size (H0, W0) has size
(max(1, H0 >> l), max(1, W0 >> l)); its texel (y, x) covers [y / H_l, (y + 1) / H_l] x [x / W_l, (x + 1) / W_l] of the unit square,
texel (i, j) of level 0 covers [i / H0, (i + 1) / H0] x [j / W0, (j + 1) / W0]; the value is the area-weighted mean of level 0 over
the covered rectangle, as an exact Fraction, rounded half up.

The level of detail, in float64: (u, v) at the position P, one whole pixel to the right and one whole pixel down from the
perspective-correct weights of the face's plane (extended beyond its edges), a = (u_x - u) W0, b = (v_x - v) H0, c = (u_y - u) W0,
e = (v_y - v) H0, rho = sqrt(max(a a + b b, c c + e e)) and the piecewise rule: an unbounded footprint takes the coarsest level,
rho <= 1 level 0, else l = floor(log2(rho)), g = rho / 2^l - 1, the top level alone from l >= L - 1 on, else (1 - g) c_l + g c_{l+1}."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import antialias_reference as ar
from tests import raster_reference as rr
from tests import texture_reference as tr
from tricolo_amd.data import render as R


def level_sizes(H0, W0):
    levels = int(math.floor(math.log2(max(H0, W0)))) + 1
    return [(max(1, H0 >> l), max(1, W0 >> l)) for l in range(levels)]


def overlaps(n0, nl, y):
    """[(i, length)]: the texels i of an axis of n0 texels that texel y of the same axis at nl texels overlaps, and by how much."""
    lo, hi = Fraction(y, nl), Fraction(y + 1, nl)
    out = []
    for i in range(y * n0 // nl, n0):
        a, b = max(lo, Fraction(i, n0)), min(hi, Fraction(i + 1, n0))
        if a >= hi:
            break
        if b > a:
            out.append((i, b - a))
    return out


def pyramid(tex):
    """tex uint8 [H0, W0, >= 3] -> [uint8 [H_l, W_l, 4]]: level 0 is the texture, alpha 255 above it."""
    H0, W0 = tex.shape[:2]
    t = tex.astype(np.int64)
    levels = [np.ascontiguousarray(tex[:, :, :4])]
    for Hl, Wl in level_sizes(H0, W0)[1:]:
        out = np.full((Hl, Wl, 4), 255, np.uint8)
        rows, cols = [overlaps(H0, Hl, y) for y in range(Hl)], [overlaps(W0, Wl, x) for x in range(Wl)]
        for y in range(Hl):
            for x in range(Wl):
                area = Fraction(1, Hl * Wl)
                for k in range(3):
                    mean = sum(wy * wx * int(t[i, j, k]) for i, wy in rows[y] for j, wx in cols[x]) / area
                    out[y, x, k] = math.floor(mean + Fraction(1, 2))
        levels.append(out)
    return levels


@functools.lru_cache(maxsize=64)
def _pyramid_of(key, shape):
    return pyramid(np.frombuffer(key, np.uint8).reshape(shape))


def cached_pyramid(tex):
    tex = np.ascontiguousarray(tex)
    return _pyramid_of(tex.tobytes(), tex.shape)


def chain(levels):
    """uint8 [sum H_l W_l, 4]: the levels one after the other, row major - the layout of csrc/mesh_batch.h."""
    return np.concatenate([lv.reshape(-1, 4) for lv in levels])


def lod(rho, unbounded, levels):
    """-> (lo int [P], g float64 [P]): the colour is (1 - g) c_lo + g c_{lo + 1}; g is 0 where one level is sampled alone."""
    top = levels - 1
    lo, g = np.full(rho.shape, top, dtype=np.int64), np.zeros(rho.shape)
    for p in range(rho.shape[0]):
        if unbounded[p]:
            continue
        if rho[p] <= 1.0:
            lo[p] = 0
            continue
        l = int(math.floor(math.log2(rho[p])))
        if l < top:
            lo[p], g[p] = l, rho[p] / 2.0 ** l - 1.0
    return lo, g


def render(verts, faces, face_mat, kd, face_uv, mat_tex, textures, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR, samples=1):
    """texture_reference.render with mip-mapped textures, for one sample (the pixel centre) or four.  -> (image uint8 [3, H, W],
    face int64 [H, W] or [H, W, 4], ambiguous bool like face, rho float64 like face - NaN where no textured face shows, inf where the
    footprint is unbounded)."""
    if samples == 4:
        face, ambiguous, covered = ar.visibility(verts, faces, cam, H, W, yfov, znear)
        pos = np.array(ar.POSITIONS) * 256.0
    else:
        face, ambiguous, covered = rr.visibility(verts, faces, cam, H, W, yfov, znear)
        face, ambiguous, covered, pos = face[:, :, None], ambiguous[:, :, None], covered[:, :, None], np.array([[128.0, 128.0]])
    okv, Xv, Yv, _ = R.snap_vertices(verts, cam, H, W, yfov, znear)
    X, Y = Xv.numpy().astype(np.float64), Yv.numpy().astype(np.float64)
    v, c, f = verts.numpy().astype(np.float64), cam.numpy().astype(np.float64), faces.numpy()
    inv_z = 1.0 / np.where(okv.numpy(), -((v - c[:3]) @ c[9:12]), 1.0)
    kd64, uv64 = kd.numpy().astype(np.float64), face_uv.numpy().astype(np.float64)
    mt, fm = np.asarray(mat_tex).astype(np.int64), np.asarray(face_mat).astype(np.int64)
    shade = tr.shades(v, f, c[:3])
    colours = np.full((3, H, W, pos.shape[0]), 255, np.int64)
    rho_out = np.full((H, W, pos.shape[0]), np.nan)
    py, px, ps = np.nonzero(covered)
    fw = face[py, px, ps]
    fi = f[fw]

    def uvd(Px, Py):
        bary = np.empty((fw.shape[0], 3))
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            bary[:, k] = (X[fi[:, b]] - X[fi[:, a]]) * (Py - Y[fi[:, a]]) - (Y[fi[:, b]] - Y[fi[:, a]]) * (Px - X[fi[:, a]])
        bary /= bary.sum(1, keepdims=True)
        wgt = bary * inv_z[fi]
        d = wgt.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return ((wgt / d[:, None])[:, :, None] * uv64[fw]).sum(1), d

    Px, Py = 256.0 * px + pos[ps, 0], 256.0 * py + pos[ps, 1]
    uv, _ = uvd(Px, Py)
    (uvx, dx), (uvy, dy) = uvd(Px + 256.0, Py), uvd(Px, Py + 256.0)
    colour = kd64[fm[fw]].copy()
    tex_of = mt[fm[fw]]
    tex_of = np.where(np.isnan(uv64[fw, 0, 0]) | ~np.isfinite(uv).all(1), -1, tex_of)
    for t in np.unique(tex_of[tex_of >= 0]):
        sel = np.nonzero(tex_of == t)[0]
        levels = cached_pyramid(textures[t])
        H0, W0 = textures[t].shape[:2]
        with np.errstate(over="ignore", invalid="ignore"):
            a, b = (uvx[sel, 0] - uv[sel, 0]) * W0, (uvx[sel, 1] - uv[sel, 1]) * H0
            g, e = (uvy[sel, 0] - uv[sel, 0]) * W0, (uvy[sel, 1] - uv[sel, 1]) * H0
            r2 = np.maximum(a * a + b * b, g * g + e * e)
        unbounded = ~(dx[sel] > 0) | ~(dy[sel] > 0) | ~np.isfinite(uvx[sel]).all(1) | ~np.isfinite(uvy[sel]).all(1) | ~np.isfinite(r2)
        rho = np.sqrt(np.where(unbounded, 1.0, r2))
        lo, frac = lod(rho, unbounded, len(levels))
        rho_out[py[sel], px[sel], ps[sel]] = np.where(unbounded, np.inf, rho)
        texel = np.empty((sel.shape[0], 3))
        for l in np.unique(lo):
            m = lo == l
            c_lo = tr.sample(levels[l], uv[sel[m], 0], uv[sel[m], 1])
            c_hi = tr.sample(levels[min(l + 1, len(levels) - 1)], uv[sel[m], 0], uv[sel[m], 1])
            texel[m] = (1.0 - frac[m, None]) * c_lo + frac[m, None] * c_hi
        colour[sel] *= texel
    colour = np.clip(colour * shade[fw][:, None], 0.0, 1.0)
    colours[:, py, px, ps] = np.floor(255.0 * colour + 0.5).astype(np.int64).T
    image = ((colours.sum(3) + 2) >> 2) if samples == 4 else colours[..., 0]
    if samples != 4:
        face, ambiguous, rho_out = face[:, :, 0], ambiguous[:, :, 0], rho_out[:, :, 0]
    return image.astype(np.uint8), face, ambiguous, rho_out
