"""Oracle of the mesh surface sampler, independent of the product code (numpy only): Philox4x32-10 from its constants on uint64
arithmetic masked to 32 bits, the float64 sampler (float64 areas and CDF from the fp32 scaled vertices, the same selection rule
and weights), the test meshes, and conditions A-D that every returned (face, point) must meet without exclusions:

  A  with t = u_f * A (A the float64 total area): cdf64[f - 1] - tau <= t <= cdf64[f] + tau, tau = 2^-22 * A.  An fp32 triangle area
     carries a few units of 2^-24 relative error and the float64 sum adds nothing visible; on these meshes the drift of the fp32-area
     CDF against the float64 one is at most 2^-28 * A, and tau is far below the narrowest face interval (2^-16 * A at 40,000 faces).
  B  no sample names a face with a repeated vertex index.
  C  every coordinate lies within 16 * 2^-24 * m of the float64 combination for the same f, m the largest absolute scaled
     coordinate of that face: one sqrtf, the weight arithmetic, three products and two sums, with a factor 2 to spare.
  D  a mesh without faces or with zero area gives zero rows and -1.
"""
import functools

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S_MAX = 10000
SAMPLE_COUNTS = (1, 255, 257, 10000)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays of 32-bit words, key: two ints -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & MASK for c in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                 # below 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms(n, S, seed):
    """(u_f, u1, u2) of mesh n, samples 0 .. S - 1: (x >> 8) * 2^-24, exact in fp32 and float64 alike."""
    s = np.arange(S, dtype=np.uint64)
    z = np.zeros(S, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((s, z + np.uint64(n), z, z), (seed & 0xFFFFFFFF, seed >> 32))
    return [(w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 for w in x[:3]]


# ------------------------------------------------------------------------------------------------ meshes
def _grid_faces(nu, nv):
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    return np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int64)


def torus(nu, nv, R=1.0, r=0.35, shift=0.0):
    u, v = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3) + shift
    return p.astype(np.float32), _grid_faces(nu, nv)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7],
                  [1, 7, 3]], dtype=np.int64)
    return v, f


def chain(F):
    """A strip of F triangles (i, i + 1, i + 2) with uneven areas."""
    rng = np.random.default_rng(F)
    x = np.cumsum(0.2 + rng.random(F + 2))
    v = np.stack([x, np.arange(F + 2) % 2 * (0.5 + rng.random(F + 2)), 0.1 * np.sin(x)], -1).astype(np.float32)
    i = np.arange(F, dtype=np.int64)
    return v, np.stack([i, i + 1, i + 2], -1)


def torus_degenerate():
    v, f = torus(64, 40)
    rows = []
    at = set(np.linspace(0, f.shape[0] - 1, 20).astype(int).tolist())             # 20 faces with a repeated index, spread through the list
    for i, face in enumerate(f):
        if i in at:
            k = len(rows) % 3
            rows.append([face[0], face[1], face[1]] if k == 0 else [face[0], face[0], face[2]] if k == 1 else [face[2], face[1], face[2]])
        rows.append(face)
    return v, np.array(rows, dtype=np.int64)


SCAN_CHUNK = 2048                                                                  # csrc/mesh_sample.hip's MS_CHUNK (the product exports it too)
MESHES = {
    "triangle": lambda: (np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0.5]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int64)),
    "two_1_3": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 0, 2]], dtype=np.float32),      # areas 0.5 and 1.5 ... 1 : 3
                        np.array([[0, 1, 2], [0, 3, 2]], dtype=np.int64)),
    "cube": cube,
    "torus_8x4": lambda: torus(8, 4),
    "torus_64x40": lambda: torus(64, 40),
    "torus_64x40_degenerate": torus_degenerate,
    "torus_64x40_plus50": lambda: torus(64, 40, shift=50.0),
    "torus_200x100": lambda: torus(200, 100),
    "chain_1": lambda: chain(1),
    "chain_255": lambda: chain(255),
    "chain_256": lambda: chain(256),
    "chain_257": lambda: chain(257),
    "chain_chunk_minus_1": lambda: chain(SCAN_CHUNK - 1),
    "chain_chunk": lambda: chain(SCAN_CHUNK),
    "chain_chunk_plus_1": lambda: chain(SCAN_CHUNK + 1),
    "empty": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32), np.zeros((0, 3), dtype=np.int64)),
}
FACE_COUNTS = {"triangle": 1, "two_1_3": 2, "cube": 12, "torus_8x4": 64, "torus_64x40": 5120, "torus_64x40_degenerate": 5140,
               "torus_64x40_plus50": 5120, "torus_200x100": 40000, "chain_1": 1, "chain_255": 255, "chain_256": 256, "chain_257": 257,
               "chain_chunk_minus_1": SCAN_CHUNK - 1, "chain_chunk": SCAN_CHUNK, "chain_chunk_plus_1": SCAN_CHUNK + 1, "empty": 0}
SMALL = [k for k, v in FACE_COUNTS.items() if v <= 5140]                          # the agreement cap applies to these


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f = MESHES[name]()
    assert f.shape[0] == FACE_COUNTS[name], (name, f.shape)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def scaled_verts(v, scale):
    return v if scale is None else (v * np.float32(scale)).astype(np.float32)


def areas64(v32, f):
    a, b, c = (v32[f[:, k]].astype(np.float64) for k in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)


def areas32(v32, f):
    """The fp32 areas in the product's order of operations (for the check of tri_mesh_face_cdf)."""
    a, b, c = (v32[f[:, k]] for k in range(3))
    u, w = b - a, c - a
    cx, cy, cz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return (np.float32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)).astype(np.float32)


def oracle(v, f, n, S, seed, scale=None):
    """The float64 sampler: dict of t, A, cdf (float64 [F]), face [S], points (float64 [S, 3]), w (the three weights)."""
    vs = scaled_verts(v, scale)
    uf, u1, u2 = uniforms(n, S, seed)
    if f.shape[0] == 0:
        return {"A": 0.0, "cdf": np.zeros(0), "t": uf * 0, "face": np.full(S, -1), "points": np.zeros((S, 3)), "vs": vs}
    cdf = np.cumsum(areas64(vs, f))
    A = cdf[-1]
    if not A > 0:
        return {"A": 0.0, "cdf": cdf, "t": uf * 0, "face": np.full(S, -1), "points": np.zeros((S, 3)), "vs": vs}
    t = uf * A
    face = np.minimum(np.searchsorted(cdf, t, side="right"), f.shape[0] - 1)
    r = np.sqrt(u1)
    w = np.stack([1 - r, r * (1 - u2), r * u2], -1)
    return {"A": A, "cdf": cdf, "t": t, "face": face, "w": w, "vs": vs, "points": combine(vs, f, face, w)}


def combine(vs, f, face, w):
    tri = vs[f[face]].astype(np.float64)                                            # [S, 3 corners, 3]
    return (w[:, :, None] * tri).sum(1)


@functools.lru_cache(maxsize=None)
def oracle_named(name, n, seed, scale=None):
    v, f = mesh(name)
    return oracle(v, f, n, S_MAX, seed, scale)


def near_boundary(o):
    """Samples whose t lies within tau of a CDF boundary (where an fp32-area CDF may legitimately pick the neighbouring face)."""
    tau = 2.0 ** -22 * o["A"]
    edges = np.concatenate([[0.0], o["cdf"]])
    k = np.searchsorted(edges, o["t"])
    d = np.minimum(np.abs(edges[np.clip(k, 0, edges.size - 1)] - o["t"]), np.abs(edges[np.clip(k - 1, 0, edges.size - 1)] - o["t"]))
    return d <= tau


def check_samples(v, f, o, points, face_idx, what):
    """Conditions A-D for the first S rows of the oracle record o (S = points.shape[0]); prints the worst figures before asserting."""
    points, face_idx = np.asarray(points), np.asarray(face_idx)
    S = points.shape[0]
    assert points.shape == (S, 3) and face_idx.shape == (S,) and points.dtype == np.float32 and face_idx.dtype == np.int64, what
    if S == 0:
        return
    if not o["A"] > 0:                                                              # D
        assert (points == 0).all() and (face_idx == -1).all(), f"{what}: an invalid mesh must give zero rows and -1"
        return
    F = f.shape[0]
    assert (face_idx >= 0).all() and (face_idx < F).all(), f"{what}: face index outside 0 .. {F - 1}"
    A, cdf, t = o["A"], o["cdf"], o["t"][:S]
    tau = 2.0 ** -22 * A
    lo = np.where(face_idx > 0, cdf[np.maximum(face_idx - 1, 0)], 0.0)
    slack = np.maximum(lo - tau - t, t - (cdf[face_idx] + tau))
    print(f"{what}: S={S} F={F} worst interval excess {slack.max() / A:.3e} A (tau = {2.0 ** -22:.3e} A)")
    assert (slack <= 0).all(), f"{what}: condition A fails for {(slack > 0).sum()} samples, worst excess {slack.max() / A:.3e} A"
    fv = f[face_idx]
    degenerate = (fv[:, 0] == fv[:, 1]) | (fv[:, 1] == fv[:, 2]) | (fv[:, 0] == fv[:, 2])
    assert not degenerate.any(), f"{what}: condition B fails, {degenerate.sum()} samples on faces with a repeated index"
    want = combine(o["vs"], f, face_idx, o["w"][:S])
    m = np.abs(o["vs"][fv].astype(np.float64)).max(axis=(1, 2))
    err = np.abs(points.astype(np.float64) - want).max(axis=1)
    bound = 16 * 2.0 ** -24 * m
    print(f"{what}: worst position error {np.max(err / np.maximum(m, 1e-300)) / 2.0 ** -24:.2f} x 2^-24 m (bound 16)")
    assert (err <= bound).all(), f"{what}: condition C fails for {(err > bound).sum()} samples"


def write_obj(path, v, f, newline="\n"):
    with open(path, "w", newline="") as fh:
        fh.write("# generated" + newline)
        for p in v:
            fh.write("v %r %r %r%s" % (float(p[0]), float(p[1]), float(p[2]), newline))
        for t in f:
            fh.write("f %d %d %d%s" % (t[0] + 1, t[1] + 1, t[2] + 1, newline))
