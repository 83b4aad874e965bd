"""An independent statement of the four-sample visibility of csrc/raster.hip (ops.render_views(..., samples=4)) for the tests: the
brute force of tests/raster_reference.visibility at the four sample positions of every pixel - float64 numpy, every face against
every sample, no boxes, no queue, no keys, no offsets added to a centre's edge value.  Like it, this shares with the code under test
only the vertices' snapped integer screen positions (tricolo_amd.data.render.snap_vertices) and takes the camera transform, the
depths, the orientation, the fill rule and the interpolation its own way.  The sample positions are written here as fractions of a
pixel, (0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875): the standard 4x rotated grid.

Per sample it keeps the nearest face (at equal depth the lower index) and the two nearest depths; a sample whose two nearest depths
differ by less than raster_reference.REL of the nearest is `ambiguous` and left out of the comparison; the scenes must keep such
samples below raster_reference.MAX_AMBIGUOUS of the covered ones."""
import numpy as np

from tests import raster_reference as rr
from tricolo_amd.data import render as R

POSITIONS = ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))


def visibility(verts, faces, cam, H, W, yfov=R.YFOV, znear=R.ZNEAR):
    """One mesh, one view.  verts fp32 [V, 3], faces int64 [F, 3], cam fp32 [12] (torch tensors) -> (face int64 [H, W, 4] (-1 = none),
    ambiguous bool [H, W, 4], covered bool [H, W, 4])."""
    okv, Xv, Yv, _ = R.snap_vertices(verts, cam, H, W, yfov, znear)
    okv, Xv, Yv = okv.numpy(), Xv.numpy().astype(np.float64), Yv.numpy().astype(np.float64)
    v, c, f = verts.numpy().astype(np.float64), cam.numpy().astype(np.float64), faces.numpy()
    depth_v = 1.0 / np.where(okv, -((v - c[:3]) @ c[9:12]), 1.0)
    sx, sy = np.array([p[0] for p in POSITIONS]), np.array([p[1] for p in POSITIONS])
    px = (np.arange(W)[None, :, None] + sx[None, None, :]) * 256.0 + np.zeros((H, 1, 1))      # [H, W, 4], exact: multiples of 32
    py = (np.arange(H)[:, None, None] + sy[None, None, :]) * 256.0 + np.zeros((1, W, 1))
    n = H * W * 4
    P = np.stack([px.ravel(), py.ravel(), np.ones(n)])                                        # [3, n]: E = coefficients . P, exact in float64
    best, second, face = np.full(n, -np.inf), np.full(n, -np.inf), np.full(n, -1, dtype=np.int64)
    for s in range(0, f.shape[0], rr.FACE_CHUNK):
        fc = f[s:s + rr.FACE_CHUNK]
        X, Y, D = Xv[fc], Yv[fc], depth_v[fc]
        A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        live = okv[fc].all(1) & (A2 != 0)
        sign = np.where(A2 < 0, -1.0, 1.0)
        inside = np.broadcast_to(live[:, None], (fc.shape[0], n)).copy()
        num = np.zeros((fc.shape[0], n))
        for k in range(3):                                                                    # the edge opposite vertex k, oriented by the sign
            a, b = (k + 1) % 3, (k + 2) % 3
            dx, dy = sign * (X[:, b] - X[:, a]), sign * (Y[:, b] - Y[:, a])
            E = np.stack([-dy, dx, dy * X[:, a] - dx * Y[:, a]], 1) @ P
            top_left = (dy < 0) | ((dy == 0) & (dx > 0))
            inside &= (E > 0) | ((E == 0) & top_left[:, None])
            num += E * D[:, k, None]
        depth = np.where(inside, num / np.where(A2 == 0, 1.0, np.abs(A2))[:, None], -np.inf)
        top = depth.argmax(0)                                                                 # the first = the lowest index among equals
        cols = np.arange(n)
        d1 = depth[top, cols]
        depth[top, cols] = -np.inf
        d2 = depth.max(0)
        better = d1 > best                                                                    # strictly: an earlier chunk keeps a tie
        second = np.where(better, np.maximum(best, d2), np.maximum(second, d1))
        face = np.where(better, s + top, face)
        best = np.where(better, d1, best)
    covered = np.isfinite(best)
    face[~covered] = -1
    two = covered & np.isfinite(second)
    ambiguous = two & ((np.where(two, best, 1.0) - np.where(two, second, 0.0)) < rr.REL * np.where(two, best, 1.0))
    return face.reshape(H, W, 4), ambiguous.reshape(H, W, 4), covered.reshape(H, W, 4)


def compare(vis, verts, faces, cam, H, W, what):
    """vis int32 [views, H, W, 4] of one mesh against the brute force -> (ambiguous, covered, mixed, touched): sample counts, and
    the pixels whose samples do not all agree among those with a covered sample; asserts the scene's condition and the equality
    outside the ambiguous samples."""
    amb = cov = mixed = touched = 0
    for k in range(cam.shape[0]):
        face, ambiguous, covered = visibility(verts, faces, cam[k], H, W)
        amb, cov = amb + int(ambiguous.sum()), cov + int(covered.sum())
        mixed += int((face != face[:, :, :1]).any(2).sum())
        touched += int(covered.any(2).sum())
        got = vis[k].numpy().astype(np.int64)
        wrong = (got != face) & ~ambiguous
        assert not wrong.any(), f"{what}, view {k}: {int(wrong.sum())} sample(s) differ from the float64 brute force, first at {np.argwhere(wrong)[0]}"
    print(f"{what}: {amb} ambiguous of {cov} covered samples; the samples of {mixed} of {touched} touched pixels disagree")
    assert amb <= rr.MAX_AMBIGUOUS * cov, f"{what}: the scene has {amb} ambiguous samples of {cov} covered ones - change the scene"
    return amb, cov, mixed, touched
