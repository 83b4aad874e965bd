"""An independent statement of csrc/raster.hip's visibility for the tests: brute force in float64 numpy, every face against every
pixel centre, no boxes, no queue, no keys.  It shares with the code under test only the vertices' snapped integer screen positions
(tricolo_amd.data.render.snap_vertices: which vertices are in front of znear, and X, Y in 1/256 pixel) - coverage is a matter of
integers and must agree exactly - and takes everything else (camera transform, depths, the orientation, the fill rule, the
interpolation) its own way in float64.  Per pixel it keeps the nearest face (at equal depth the lower index) and the two nearest
depths; a pixel whose two nearest depths differ by less than REL of the nearest is `ambiguous`: there fp32 interpolation may pick
the other face, and the comparison leaves such pixels out.  The scenes used must keep them below MAX_AMBIGUOUS of the covered pixels.

Also the scenes the CPU and GPU tests share: the random soup and the procedural mesh (a sphere plus boxes)."""
import math

import numpy as np
import torch

from tricolo_amd.data import render as R

REL = 1e-5
MAX_AMBIGUOUS = 0.01
FACE_CHUNK = 512


def visibility(verts, faces, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR):
    """One mesh, one view.  verts fp32 [V, 3], faces int64 [F, 3], cam fp32 [12] (torch tensors) -> (face int64 [H, W] (-1 =
    background), ambiguous bool [H, W], covered bool [H, W])."""
    okv, Xv, Yv, _ = R.snap_vertices(verts, cam, H, W, yfov, znear)
    okv, Xv, Yv = okv.numpy(), Xv.numpy().astype(np.float64), Yv.numpy().astype(np.float64)
    v, c, f = verts.numpy().astype(np.float64), cam.numpy().astype(np.float64), faces.numpy()
    depth_v = 1.0 / np.where(okv, -((v - c[:3]) @ c[9:12]), 1.0)                        # 1 / distance along the viewing direction
    px, py = np.meshgrid(np.arange(W) * 256.0 + 128.0, np.arange(H) * 256.0 + 128.0)
    P = np.stack([px.ravel(), py.ravel(), np.ones(H * W)])                            # [3, HW]: E = coefficients . P, exact in float64
    best = np.full(H * W, -np.inf)
    second = np.full(H * W, -np.inf)
    face = np.full(H * W, -1, dtype=np.int64)
    for s in range(0, f.shape[0], FACE_CHUNK):
        fc = f[s:s + FACE_CHUNK]
        X, Y, D = Xv[fc], Yv[fc], depth_v[fc]
        A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        live = okv[fc].all(1) & (A2 != 0)
        sign = np.where(A2 < 0, -1.0, 1.0)
        inside = np.broadcast_to(live[:, None], (fc.shape[0], H * W)).copy()
        num = np.zeros((fc.shape[0], H * W))
        for k in range(3):                                                             # the edge opposite vertex k, oriented by the sign
            a, b = (k + 1) % 3, (k + 2) % 3
            dx, dy = sign * (X[:, b] - X[:, a]), sign * (Y[:, b] - Y[:, a])
            E = np.stack([-dy, dx, dy * X[:, a] - dx * Y[:, a]], 1) @ P                # dx (Py - Ya) - dy (Px - Xa)
            top_left = (dy < 0) | ((dy == 0) & (dx > 0))
            inside &= (E > 0) | ((E == 0) & top_left[:, None])
            num += E * D[:, k, None]
        depth = np.where(inside, num / np.where(A2 == 0, 1.0, np.abs(A2))[:, None], -np.inf)
        top = depth.argmax(0)                                                          # the first = the lowest index among equals
        cols = np.arange(H * W)
        d1 = depth[top, cols]
        depth[top, cols] = -np.inf
        d2 = depth.max(0)
        better = d1 > best                                                             # strictly: an earlier chunk keeps a tie
        second = np.where(better, np.maximum(best, d2), np.maximum(second, d1))
        face = np.where(better, s + top, face)
        best = np.where(better, d1, best)
    covered = np.isfinite(best)
    face[~covered] = -1
    two = covered & np.isfinite(second)
    ambiguous = two & ((np.where(two, best, 1.0) - np.where(two, second, 0.0)) < REL * np.where(two, best, 1.0))
    return face.reshape(H, W), ambiguous.reshape(H, W), covered.reshape(H, W)


def compare(vis, verts, faces, cam, H, W, what):
    """vis int32 [views, H, W] of one mesh against the brute force; returns (ambiguous, covered) pixel counts after asserting the
    scene's condition and the equality outside the ambiguous pixels."""
    amb = cov = 0
    for k in range(cam.shape[0]):
        face, ambiguous, covered = visibility(verts, faces, cam[k], H, W)
        amb, cov = amb + int(ambiguous.sum()), cov + int(covered.sum())
        got = vis[k].numpy().astype(np.int64)
        wrong = (got != face) & ~ambiguous
        assert not wrong.any(), f"{what}, view {k}: {int(wrong.sum())} pixel(s) differ from the float64 brute force, first at {np.argwhere(wrong)[0]}"
    print(f"{what}: {amb} ambiguous of {cov} covered pixels")
    assert amb <= MAX_AMBIGUOUS * cov, f"{what}: the scene has {amb} ambiguous pixels of {cov} covered ones - change the scene"
    return amb, cov


# ---------------------------------------------------------------------------------------------------- scenes
def soup(seed=11, n=200):
    """200 random triangles in the unit ball around the origin for a camera set of pack_cameras: mostly small, with slivers, two
    zero-area faces, four faces larger than the per-lane path (a box above 8 x 8 pixels at 32 x 48), and faces partly and wholly
    off screen.  -> (verts fp32 [3n, 3], faces int64 [n, 3])."""
    g = np.random.default_rng(seed)
    centre = g.uniform(-0.3, 0.3, size=(n, 1, 3))
    tri = centre + g.normal(scale=0.03, size=(n, 3, 3))
    tri[0:12, 2] = tri[0:12, 1] + 1e-3 * g.normal(size=(12, 3))                        # slivers
    tri[12, 2] = tri[12, 1]                                                            # two vertices coincide: zero area
    tri[13, 0] = tri[13, 2]                                                            # and so do another two
    tri[14:18] = g.uniform(-0.2, 0.2, size=(4, 1, 3)) + g.normal(scale=0.25, size=(4, 3, 3))      # large: the queue kernel
    tri[18:24] += np.array([0.9, 0.0, 0.0])                                            # partly / wholly off screen
    tri[24:28] += np.array([0.0, 1.6, 0.0])
    verts = torch.from_numpy(tri.reshape(-1, 3).astype(np.float32))
    return verts, torch.arange(3 * n, dtype=torch.int64).reshape(n, 3)


def _box(lo, hi):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v, np.array(f)


def procedural_mesh(rings=100):
    """A UV sphere of radius 0.3 (2 * rings * (rings - 1) faces: about 20 k at rings = 100) on a table of five boxes (60 large faces),
    inside the 0.5 ball of a model_normalized.obj; three materials.  -> (verts fp32, faces int64, face_mat int32, Kd fp32 [3, 3])."""
    lat = np.linspace(0.0, math.pi, rings + 1)[1:-1]
    lon = np.linspace(0.0, 2.0 * math.pi, rings, endpoint=False)
    r = 0.3
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.broadcast_to(np.cos(lat)[:, None], (rings - 1, rings)),
                     np.outer(np.sin(lat), np.sin(lon))], -1).reshape(-1, 3) * r + np.array([0.0, 0.12, 0.0])
    verts = [ring, np.array([[0.0, 0.12 + r, 0.0], [0.0, 0.12 - r, 0.0]])]
    top, bottom = ring.shape[0], ring.shape[0] + 1
    f = []
    for i in range(rings - 2):
        for j in range(rings):
            a, b = i * rings + j, i * rings + (j + 1) % rings
            f += [(a, b, b + rings), (a, b + rings, a + rings)]
    for j in range(rings):
        f += [(top, (j + 1) % rings, j), (bottom, (rings - 2) * rings + j, (rings - 2) * rings + (j + 1) % rings)]
    faces = [np.array(f)]
    mats = [np.where(np.arange(len(f)) % 2 == 0, 1, 2)]
    count = ring.shape[0] + 2
    boxes = [((-0.4, -0.22, -0.3), (0.4, -0.18, 0.3))] + [((sx * 0.36 - 0.03, -0.45, sz * 0.26 - 0.03), (sx * 0.36 + 0.03, -0.22, sz * 0.26 + 0.03))
                                                          for sx in (-1, 1) for sz in (-1, 1)]
    for lo, hi in boxes:
        bv, bf = _box(lo, hi)
        verts.append(bv)
        faces.append(bf + count)
        mats.append(np.zeros(len(bf), dtype=np.int64))
        count += 8
    kd = torch.tensor([[0.4, 0.4, 0.4], [0.8, 0.2, 0.1], [0.1, 0.3, 0.9]], dtype=torch.float32)
    return (torch.from_numpy(np.concatenate(verts).astype(np.float32)), torch.from_numpy(np.concatenate(faces).astype(np.int64)),
            torch.from_numpy(np.concatenate(mats).astype(np.int32)), kd)
