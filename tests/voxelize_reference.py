"""An independent statement of csrc/voxelize.hip for the tests, written from the definition at the head of that file and sharing no
code with tricolo_amd/data/voxelize.py.

Surface occupancy: the snapped triangle is clipped against the closed voxel box by Sutherland-Hodgman in exact rationals
(fractions.Fraction); a non-empty result - a polygon, a segment or a single point - means the box and the face overlap, which is what
the thirteen separating-axis tests decide.  It runs brute force, every face against every voxel of a small grid.  Carve and interior
colour: plain loops over the label grid.  Everything is integer or rational, so agreement is exact and no voxel is excluded.

Also the scenes the CPU and GPU tests share."""
import math
from fractions import Fraction

import numpy as np
import torch

SNAP_MAX = 2 ** 17


# ---------------------------------------------------------------------------------------------------- the reference
def snap(verts, frame):
    """verts [Vn, 3], frame [4] (numpy float32) -> (ok bool [Vn], G python ints [Vn][3]) in 1/256 voxel."""
    verts, frame = np.asarray(verts, np.float32), np.asarray(frame, np.float32)
    ok, G = [], []
    for p in verts:
        row, fine = [], True
        for a in range(3):
            d = np.float32(p[a] - frame[a])
            with np.errstate(all="ignore"):
                s = np.float32(256.0) * np.float32(np.float64(d) / np.float64(frame[3]))
            if not abs(float(s)) <= SNAP_MAX:                                          # NaN fails
                fine = False
                row.append(0)
            else:
                row.append(int(np.rint(s)))                                            # ties to even
        ok.append(fine)
        G.append(row)
    return ok, G


def clip_nonempty(tri, lo, hi):
    """Does the triangle (three integer points) meet the closed box [lo, hi]?  Sutherland-Hodgman against the six half-spaces."""
    poly = [tuple(p) for p in tri]
    for axis in range(3):
        for sign, bound in ((1, lo[axis]), (-1, hi[axis])):
            out = []
            for a, b in zip(poly, poly[1:] + poly[:1]):
                ina, inb = sign * (a[axis] - bound) >= 0, sign * (b[axis] - bound) >= 0
                if ina:
                    out.append(a)
                if ina != inb:
                    t = Fraction(bound - a[axis], b[axis] - a[axis])
                    out.append(tuple(a[c] + t * (b[c] - a[c]) for c in range(3)))
            poly = out
            if not poly:
                return False
    return True


def colour_bytes(face_mat, kd):
    """q [F][3]: floor(255 clamp(Kd, 0, 1) + 0.5) in float32, grey 0.4 without materials."""
    kd = np.asarray(kd, np.float32).reshape(-1, 3)
    out = []
    for m in np.asarray(face_mat).tolist():
        row = kd[min(m, len(kd) - 1)] if len(kd) else np.full(3, 0.4, np.float32)
        out.append([int(np.floor(np.float32(255.0) * np.float32(min(max(float(c), 0.0), 1.0)) + np.float32(0.5))) for c in row])
    return out


def surface(verts, faces, face_mat, kd, frame, K):
    """Brute force over the low K[0] x K[1] x K[2] corner of the grid -> (count int64 [*K], sums int64 [3, *K]): per voxel the faces
    that overlap its closed box and the sums of their colour bytes."""
    count, sums = np.zeros(tuple(K), np.int64), np.zeros((3,) + tuple(K), np.int64)
    fr = [float(x) for x in np.asarray(frame, np.float32)]
    if not all(math.isfinite(x) for x in fr) or not fr[3] > 0:
        return count, sums
    ok, G = snap(verts, frame)
    q = colour_bytes(face_mat, kd)
    for f, idx in enumerate(np.asarray(faces).tolist()):
        if not all(ok[v] for v in idx):
            continue
        tri = [G[v] for v in idx]
        e1, e2 = [tri[1][c] - tri[0][c] for c in range(3)], [tri[2][c] - tri[0][c] for c in range(3)]
        normal = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        if normal == (0, 0, 0):
            continue
        for i in range(K[0]):
            for j in range(K[1]):
                for k in range(K[2]):
                    if clip_nonempty(tri, (256 * i, 256 * j, 256 * k), (256 * i + 256, 256 * j + 256, 256 * k + 256)):
                        count[i, j, k] += 1
                        for c in range(3):
                            sums[c, i, j, k] += q[f][c]
    return count, sums


def resolve(count, sums, fill):
    """-> (grid uint8 [4, *K], labels uint8 [*K]) from the surface sums: the rounded mean on the surface, the carve."""
    K = count.shape
    grid, labels = np.zeros((4,) + K, np.uint8), np.zeros(K, np.uint8)
    for i, j, k in np.argwhere(count > 0):
        labels[i, j, k] = 1
        n = int(count[i, j, k])
        grid[:3, i, j, k] = [(2 * int(sums[c, i, j, k]) + n) // (2 * n) for c in range(3)]
        grid[3, i, j, k] = 255
    if not fill:
        return grid, labels
    steps = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]          # the tie order
    inside = lambda p: all(0 <= c < n for c, n in zip(p, K))
    for i in range(K[0]):
        for j in range(K[1]):
            for k in range(K[2]):
                if labels[i, j, k] == 1:
                    continue
                hits = []
                for s in steps:
                    p, d = [i + s[0], j + s[1], k + s[2]], 1
                    while inside(p) and labels[p[0], p[1], p[2]] != 1:
                        p, d = [p[0] + s[0], p[1] + s[1], p[2] + s[2]], d + 1
                    if not inside(p):
                        break                                                              # open this way: exterior
                    hits.append((d, tuple(p)))
                if len(hits) == 6:
                    nearest = min(hits, key=lambda h: h[0])                                # min keeps the first of equals
                    labels[i, j, k] = 2
                    grid[:, i, j, k] = grid[:, nearest[1][0], nearest[1][1], nearest[1][2]]
    return grid, labels


def reference(scene, V, K, fills=(1,)):
    """[(grid [4, V, V, V], labels [V, V, V]) per fill mode] with the brute force on the low K[0] x K[1] x K[2] corner and zeros
    elsewhere.  The caller checks that the snapped mesh, as far as it lies inside the grid, lies inside the corner: rays that leave
    the corner then meet nothing up to the grid boundary, so carving the corner alone is carving the grid."""
    verts, faces, fm, kd, frame = scene
    count, sums = surface(verts.numpy(), faces.numpy(), fm.numpy(), kd.numpy(), frame.numpy(), K)
    out = []
    for fill in fills:
        g, l = resolve(count, sums, fill)
        grid, labels = np.zeros((4, V, V, V), np.uint8), np.zeros((V, V, V), np.uint8)
        grid[:, :K[0], :K[1], :K[2]], labels[:K[0], :K[1], :K[2]] = g, l
        out.append((grid, labels))
    return out


# ---------------------------------------------------------------------------------------------------- scenes
# (verts fp32 [Vn, 3], faces int64 [F, 3], face_mat int32 [F], Kd fp32 [M, 3], frame fp32 [4]); the frames put the mesh into the
# low corner of a V = 32 grid, where it spans about 8 voxels.
CORNER = (12, 12, 12)
FRAME = torch.tensor([-0.1, 0.05, -0.2, 0.05], dtype=torch.float32)
GRID_FRAME = torch.tensor([0.0, 0.0, 0.0, 0.25], dtype=torch.float32)                    # exact: x = 0.75 is the plane between layers 2 and 3
KD3 = torch.tensor([[0.9, 0.2, 0.1], [0.1, 0.4, 0.8], [0.35, 1.7, -0.2]], dtype=torch.float32)   # the third is clamped


def _scene(tri, frame, mats=None, kd=None):
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    n = tri.shape[0]
    fm = torch.zeros((n,), dtype=torch.int32) if mats is None else torch.as_tensor(mats, dtype=torch.int32)
    return (torch.from_numpy(tri.reshape(-1, 3).astype(np.float32)), torch.arange(3 * n, dtype=torch.int64).reshape(n, 3), fm,
            KD3[:1].clone() if kd is None else kd, frame.clone())


def at(frame, p):
    """Grid coordinates (in voxels) -> mesh coordinates under `frame`."""
    f = frame.numpy().astype(np.float64)
    return f[:3] + f[3] * np.asarray(p, np.float64)


def one_triangle():
    return _scene([at(FRAME, [[1.3, 2.2, 1.1], [8.6, 3.4, 2.7], [4.2, 8.9, 7.5]])], FRAME)


def soup(n=60, seed=21, frame=FRAME, span=8.0, size=0.7):
    """n random triangles of about a voxel within [1, 1 + span]^3 voxels, three materials, a few slivers and larger faces."""
    g = np.random.default_rng(seed)
    centre = g.uniform(1.5, span + 0.5, size=(n, 1, 3))
    tri = centre + g.normal(scale=size, size=(n, 3, 3))
    tri[0:4, 2] = tri[0:4, 1] + 1e-2 * g.normal(size=(4, 3))                               # slivers
    tri[4:7] = g.uniform(2.0, span, size=(3, 1, 3)) + g.normal(scale=2.0, size=(3, 3, 3))  # a few voxels across
    tri = np.clip(tri, 0.2, span + 1.8)
    return _scene(at(frame, tri), frame, g.integers(0, 3, n), KD3)


def boundary_plane():
    """One face lying exactly in the plane x = 3 voxels (both layers 2 and 3 are set), one in z = 5 with an edge along y = 2."""
    return _scene([[[0.75, 0.3, 0.4], [0.75, 1.6, 0.5], [0.75, 0.7, 1.7]], [[0.3, 0.5, 1.25], [1.4, 0.5, 1.25], [0.8, 1.9, 1.25]]], GRID_FRAME, [0, 1], KD3)


def zero_area():
    """Two proper faces and three without area: two vertices equal, three on a line, and a sliver that only the snap flattens."""
    a = at(FRAME, [[2.0, 2.0, 2.0], [6.0, 3.0, 2.5], [3.0, 7.0, 5.0]])
    b = at(FRAME, [[5.0, 5.0, 1.5], [8.5, 6.0, 7.0], [6.0, 2.0, 8.0]])
    twice = at(FRAME, [[1.0, 1.0, 1.0], [7.0, 7.0, 7.0], [7.0, 7.0, 7.0]])
    line = at(FRAME, [[1.0, 8.0, 1.0], [3.0, 8.0, 3.0], [5.0, 8.0, 5.0]])
    flat = at(FRAME, [[4.0, 1.0, 4.0], [8.0, 1.0, 4.0], [6.0, 1.0 + 1e-4, 4.0]])           # 1e-4 voxel: below the 1/256 snap
    return _scene([a, twice, b, line, flat], FRAME, [0, 1, 1, 2, 2], KD3)


def outside():
    """Faces partly outside the frame (across the low faces of the grid) and wholly outside it, beside one inside."""
    inside = at(FRAME, [[2.0, 2.0, 2.0], [6.0, 3.0, 2.5], [3.0, 7.0, 5.0]])
    across = at(FRAME, [[-3.0, 2.0, 4.0], [5.0, 1.0, 6.0], [2.0, -4.0, 3.0]])
    corner = at(FRAME, [[-1.0, -1.0, 5.0], [3.0, -0.5, 0.5], [-0.5, 4.0, -2.0]])
    gone = at(FRAME, [[-5.0, 2.0, 2.0], [-2.0, 3.0, 4.0], [-3.0, 6.0, 1.0]])
    return _scene([inside, across, corner, gone], FRAME, [0, 1, 2, 1], KD3)


def touching_from_outside():
    """A face outside the grid whose one vertex lies exactly on the grid's low x face: it touches layer 0 in one point."""
    return _scene([[[-0.5, 0.3, 0.3], [0.0, 0.3, 0.8], [-0.25, 1.0, 0.5]]], GRID_FRAME)


def beyond_snap():
    """A face with one vertex 600 voxels away (the snap bound is 512) is dropped although it crosses the grid; its neighbour stays."""
    far = at(FRAME, [[2.0, 2.0, 2.0], [6.0, 3.0, 2.5], [600.0, 7.0, 5.0]])
    near = at(FRAME, [[1.5, 6.0, 3.0], [7.0, 7.5, 2.0], [4.0, 2.5, 8.0]])
    edge = at(FRAME, [[2.0, 1.0, 7.0], [5.0, 2.0, 8.0], [511.0, 3.0, 6.0]])                # inside the bound: kept, clipped by the grid
    return _scene([far, near, edge], FRAME, [0, 1, 2], KD3)


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def box_shell(lo, hi, frame, top=True, top_material=0, material=0):
    """The six (or, without the +y wall, five) walls of an axis-aligned box in voxel coordinates, two triangles each."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    walls = {"-x": _quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), "+x": _quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),
             "-y": _quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), "+y": _quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),
             "-z": _quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), "+z": _quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))}
    tri, mats = [], []
    for name, quad in walls.items():
        if name == "+y" and not top:
            continue
        tri += quad
        mats += [top_material if name == "+y" else material] * 2
    return _scene(at(frame, tri), frame, mats, torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], dtype=torch.float32))


def uv_sphere(radius, centre, frame, rings=24):
    """A UV sphere in voxel coordinates: 2 rings (rings - 1) faces, all vertices on the sphere."""
    lat = np.linspace(0.0, math.pi, rings + 1)[1:-1]
    lon = np.linspace(0.0, 2.0 * math.pi, rings, endpoint=False)
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.broadcast_to(np.cos(lat)[:, None], (rings - 1, rings)),
                     np.outer(np.sin(lat), np.sin(lon))], -1).reshape(-1, 3)
    pts = np.concatenate([ring, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]]) * radius + np.asarray(centre, np.float64)
    top, bottom = ring.shape[0], ring.shape[0] + 1
    f = []
    for i in range(rings - 2):
        for j in range(rings):
            a, b = i * rings + j, i * rings + (j + 1) % rings
            f += [(a, b, b + rings), (a, b + rings, a + rings)]
    for j in range(rings):
        f += [(top, (j + 1) % rings, j), (bottom, (rings - 2) * rings + j, (rings - 2) * rings + (j + 1) % rings)]
    faces = torch.tensor(f, dtype=torch.int64)
    return (torch.from_numpy(at(frame, pts).astype(np.float32)), faces, torch.zeros((len(f),), dtype=torch.int32), KD3[:1].clone(), frame.clone())


def spanning(V, n_small=300, seed=4):
    """One face across the whole grid (the queue path) with n_small sub-voxel faces (the in-lane path), framed for a grid of V."""
    frame = torch.tensor([-0.4, -0.3, -0.5, 1.0 / V], dtype=torch.float32)
    g = np.random.default_rng(seed)
    centre = g.uniform(1.0, V - 1.0, size=(n_small, 1, 3))
    small = centre + g.normal(scale=0.2, size=(n_small, 3, 3))
    big = np.array([[[0.3, 0.6, 0.2], [V - 0.4, 1.7, V - 0.9], [V * 0.5, V - 0.2, V * 0.4]]])
    return _scene(at(frame, np.concatenate([big, small])), frame, g.integers(0, 3, n_small + 1), KD3)
