"""OBJ meshes to surface point clouds: the front half of the reference's calculate_f1.py (pytorch3d's load_obj, Meshes.
get_bounding_boxes / scale_verts and sample_points_from_meshes), so that the shape F1 can start from ShapeNet's
model_normalized.obj files instead of an existing point_cache/*.npy.

On GPU tensors the bounding boxes, the float64 CDF of the fp32 face areas and the samples come from csrc/mesh_sample.hip
(ops.mesh_bbox / mesh_face_cdf / mesh_sample_points: six launches from a packed batch to [N, S, 3] points).  On CPU tensors the
same functions run a per-mesh torch fallback with the same arithmetic and the same random stream; it exists for checking and for
machines without a GPU and is not tuned.

The generator is counter-based (Philox4x32-10, key = seed, counter = (sample, batch index, 0, 0)): row (n, s) of the result
depends on (seed, n, s) and on mesh n, not on num_samples, the batch size or the other meshes.  A mesh sampled alone therefore
equals its row of a batch only where it sits at the same batch index n.

One deliberate difference from the reference.  calculate_f1.py caches one cloud per model id and scales a retrieved shape by the
"gt-10" factor of whichever ground truth it met first, in 10 worker processes: the scale of a cached retrieved shape is a race.
Here a cached cloud always carries its OWN gt-10 factor (longest bounding-box edge 10): deterministic, and equal to what the
reference writes for every shape that occurs as a ground truth.  compare_meshes keeps the reference's exact pair semantics
(prediction scaled by the ground truth's factor) for whoever wants them.
"""
import torch

from ..meshes import cross, load_obj, pack_meshes  # noqa: F401  (load_obj: part of what this module offers the shape-F1 command)
from . import shape_f1 as _sf

_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF
SCAN_CHUNK = 2048                  # faces per chunk of the GPU scan (csrc/mesh_sample.hip MS_CHUNK): fixed, part of the CDF's bits


# ------------------------------------------------------------------------------------------------ bounding boxes and scale
def _bbox(verts, vert_off):
    if verts.is_cuda:
        from .. import ops
        return ops.mesh_bbox(verts, vert_off)
    off = vert_off.tolist()
    out = torch.zeros((len(off) - 1, 3, 2), dtype=torch.float32)
    for n, (a, b) in enumerate(zip(off, off[1:])):
        if b > a:
            out[n, :, 0], out[n, :, 1] = verts[a:b].amin(0), verts[a:b].amax(0)
    return out


def bounding_boxes(verts_list, device=None):
    """[N, 3, 2] per-axis (min, max) over all vertices of every mesh, referenced by a face or not (pytorch3d's get_bounding_boxes)."""
    empty = [torch.zeros((0, 3), dtype=torch.int64)] * len(verts_list)
    verts, _, voff, _, _ = pack_meshes(verts_list, empty, device)
    return _bbox(verts, voff)


def _verts_of(mesh):
    return mesh if torch.is_tensor(mesh) else mesh[0]


def resolve_scale(scale, verts, vert_off, gt=None):
    """None | number | tensor [N] | "gt-<x>" -> None or a float32 [N] tensor on verts' device.  "gt-<x>": x / (longest bounding-box
    edge) of the mesh given as gt (a verts tensor, a (verts, faces) pair, or a list of N of either; one mesh serves the whole batch),
    of every mesh's own box when gt is None - the reference's _scale_meshes, in fp32 like it."""
    N = vert_off.numel() - 1
    if scale is None:
        return None
    if isinstance(scale, str):
        if not scale.startswith("gt-"):
            raise ValueError("Invalid scale: %r" % scale)
        target = float(scale[3:])
        if gt is None:
            bbox = _bbox(verts, vert_off)
        else:
            gts = [_verts_of(g) for g in gt] if isinstance(gt, list) else [_verts_of(gt)]
            if len(gts) not in (1, N):
                raise ValueError(f"gt holds {len(gts)} meshes for a batch of {N}")
            bbox = bounding_boxes(gts, verts.device)
        long_edge = (bbox[:, :, 1] - bbox[:, :, 0]).max(dim=1)[0]
        return (target / long_edge).expand(N).contiguous()
    if torch.is_tensor(scale):
        if scale.shape != (N,):
            raise ValueError(f"scale must have shape ({N},)")
        return scale.to(device=verts.device, dtype=torch.float32).contiguous()
    return torch.full((N,), float(scale), dtype=torch.float32, device=verts.device)


# ------------------------------------------------------------------------------------------------ CPU fallback
def _mulhilo(m, c):
    """(high, low) 32 bits of m * c for a 32-bit constant m and int64 tensor c < 2^32, without leaving int64."""
    p_lo, p_hi = m * (c & 0xFFFF), m * (c >> 16)                                    # both below 2^48
    return (p_hi + (p_lo >> 16)) >> 16, (((p_hi & 0xFFFF) << 16) + p_lo) & _M32


def philox4x32_10(counter, key):
    """Philox4x32-10 on int64 tensors holding 32-bit words: counter = (c0, c1, c2, c3), key = (k0, k1) -> (x0, x1, x2, x3)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        hi0, lo0 = _mulhilo(_PHILOX_M0, c0)
        hi1, lo1 = _mulhilo(_PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def _uniforms(n, S, seed):
    s = torch.arange(S, dtype=torch.int64)
    zero = torch.zeros_like(s)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((s, zero + (n & _M32), zero, zero), (seed & _M32, seed >> 32))
    return [(w >> 8).to(torch.float32) * 2.0 ** -24 for w in x[:3]]


def _scaled(verts, s):
    return verts if s is None else verts * s


def face_areas(verts, faces):
    """0.5 * |(b - a) x (c - a)| in fp32, every operation rounded on its own (the order of csrc/mesh_batch.h)."""
    cx, cy, cz = cross(verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]])
    return 0.5 * torch.sqrt((cx * cx + cy * cy) + cz * cz)


def _sample_cpu(verts, faces, vert_off, face_off, scale, S, seed):
    voff, foff = vert_off.tolist(), face_off.tolist()
    N = len(voff) - 1
    points = torch.zeros((N, S, 3), dtype=torch.float32)
    idx = torch.full((N, S), -1, dtype=torch.int64)
    for n in range(N):
        v = _scaled(verts[voff[n]:voff[n + 1]], None if scale is None else scale[n])
        f = faces[foff[n]:foff[n + 1]].to(torch.int64)
        if f.shape[0] == 0 or v.shape[0] == 0 or S == 0:
            continue
        cdf = torch.cumsum(face_areas(v, f).to(torch.float64), dim=0)
        total = cdf[-1]
        if not (bool(total > 0) and bool(torch.isfinite(total))):
            continue
        uf, u1, u2 = _uniforms(n, S, seed)
        pick = torch.searchsorted(cdf, uf.to(torch.float64) * total, right=True).clamp(max=f.shape[0] - 1)   # smallest f: cdf[f] > t
        a, b, c = v[f[pick, 0]], v[f[pick, 1]], v[f[pick, 2]]
        r = torch.sqrt(u1)
        w0, w1, w2 = (1.0 - r)[:, None], (r * (1.0 - u2))[:, None], (r * u2)[:, None]
        points[n] = (w0 * a + w1 * b) + w2 * c
        idx[n] = pick
    return points, idx


# ------------------------------------------------------------------------------------------------ the public calls
def sample_points_from_meshes(verts_list, faces_list, num_samples=10000, seed=0, scale=None, return_face_idx=False, device=None, gt=None):
    """num_samples area-weighted surface points of every mesh -> float32 [N, S, 3] (with return_face_idx also the int64 [N, S] face
    of every point, local to its mesh): pytorch3d's sample_points_from_meshes without normals, on meshes scaled by `scale` first
    (resolve_scale: None, a number, a tensor [N], or "gt-<x>" with the optional gt=).  A mesh without faces or with total area 0 gives
    zero rows and -1.  Row (n, s) depends on (seed, n, s) and mesh n only; a mesh sampled alone equals its row in a batch only at
    the same batch index n.  Inputs are validated on the host before anything runs.  device=None: where verts_list[0] lives."""
    S = int(num_samples)
    if S < 0:
        raise ValueError("num_samples must not be negative")
    verts, faces, voff, foff, max_faces = pack_meshes(verts_list, faces_list, device)
    sc = resolve_scale(scale, verts, voff, gt)
    if verts.is_cuda:
        from .. import ops
        cdf, total = ops.mesh_face_cdf(verts, faces, voff, foff, sc, max_faces)
        out = ops.mesh_sample_points(verts, faces, voff, foff, cdf, total, S, seed, sc, return_face_idx)
        return out
    points, idx = _sample_cpu(verts, faces, voff, foff, sc, S, seed)
    return (points, idx) if return_face_idx else points


def compare_meshes(pred_meshes, gt_mesh, num_samples=10000, scale="gt-10", thresholds=(0.1,), seed=0, device=None):
    """The reference's compare_meshes without its cache: pred_meshes (a list of (verts, faces)) and gt_mesh (one (verts, faces)) are
    scaled by the SAME factor - with "gt-<x>" the ground truth's, so that its longest bounding-box edge becomes x - sampled, and go
    through compute_sampling_metrics (the ground truth's cloud shared by all predictions).  seed: an int s samples the predictions
    with s and the ground truth with s + 1 (the reference draws them independently); a pair gives both."""
    seed_pred, seed_gt = (seed, seed + 1) if isinstance(seed, int) else seed
    pv, pf = [m[0] for m in pred_meshes], [m[1] for m in pred_meshes]
    gt_for_scale = gt_mesh if isinstance(scale, str) else None
    pred = sample_points_from_meshes(pv, pf, num_samples, seed_pred, scale, device=device, gt=gt_for_scale)
    gt = sample_points_from_meshes([gt_mesh[0]], [gt_mesh[1]], num_samples, seed_gt, scale, device=device, gt=gt_for_scale)
    return _sf.compute_sampling_metrics(pred, gt, thresholds=thresholds)
