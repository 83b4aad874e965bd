"""Shape F1 of the top-1 retrieved shape (the reference's calculate_f1.py, the one consumer of nearest.jsonl).

For every query the point cloud of the first retrieved shape is compared with the ground-truth shape's: nearest-neighbour
distances both ways, precision / recall = the share of points closer than a threshold, F1 from the two.  On GPU tensors the
nearest-neighbour search, the counts and the F1 arithmetic run in csrc/chamfer.hip (ops.nn_dist2 / f1_counts / f1_finalize:
five launches from points to F1, nothing comes back to the host in between).  On CPU tensors the same functions run a plain
chunked torch fallback with the same arithmetic (fp32, distances from the differences); it exists so that the interface and
the F1 formula can be used and tested without a GPU and is not tuned.

Clouds come from the reference's point_cache/*.npy format.  A shape without a cached cloud is loaded from its
model_normalized.obj, scaled and sampled by tricolo_amd.evaluation.mesh (csrc/mesh_sample.hip on the GPU) and written to the cache
when --mesh-root / --category-map are given; without them only an existing cache is read, as before.

One deliberate difference from the reference: it scales a retrieved shape by the gt-10 factor of whichever ground truth it met
first (10 worker processes race for the cache); here a cached cloud always carries its OWN gt-10 factor - deterministic, and what the
reference writes for every shape that occurs as a ground truth.  mesh.compare_meshes keeps the reference's pair semantics.

    python -m tricolo_amd.evaluation.shape_f1 nearest.jsonl --point-cache DIR [--mesh-root ShapeNetCore.v2 --category-map val_map.json]
"""
import argparse
import json
import os

import numpy as np
import torch

_CPU_CHUNK = 1 << 22          # point pairs per step of the CPU fallback


def _check_clouds(p, q):
    for name, x in (("pred_points", p), ("gt_points", q)):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[-1] != 3 or x.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor of shape [N, S, 3]")
    if p.device != q.device:
        raise ValueError(f"both clouds must be on one device, got {p.device} and {q.device}")
    N = max(p.shape[0], q.shape[0])
    if min(p.shape[0], q.shape[0]) == 0 or p.shape[0] not in (1, N) or q.shape[0] not in (1, N):
        raise ValueError(f"batch sizes {p.shape[0]} and {q.shape[0]} do not match (one side may be 1)")
    return N


def _check_lengths(lengths, N, S, device):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths, dtype=torch.int64, device=device).contiguous()
    if lengths.shape != (N,):
        raise ValueError(f"lengths must have shape ({N},)")
    return lengths if lengths.is_cuda else lengths.clamp(0, S)          # the kernels clamp themselves


def _nn_dist2_cpu(p, q, lengths_p, lengths_q, return_idx):
    N, S1, S2 = max(p.shape[0], q.shape[0]), p.shape[1], q.shape[1]
    d2 = torch.zeros((N, S1), dtype=torch.float32)
    idx = torch.full((N, S1), -1, dtype=torch.int64)
    rows = max(1, _CPU_CHUNK // max(S2, 1))
    for n in range(N):
        lp = S1 if lengths_p is None else int(lengths_p[n])
        lq = S2 if lengths_q is None else int(lengths_q[n])
        pn, qn = p[n if p.shape[0] > 1 else 0, :lp], q[n if q.shape[0] > 1 else 0, :lq]
        if lq == 0:
            d2[n, :lp] = float("inf")
            continue
        for i0 in range(0, lp, rows):
            a = pn[i0:i0 + rows, None, :]
            dx, dy, dz = a[..., 0] - qn[None, :, 0], a[..., 1] - qn[None, :, 1], a[..., 2] - qn[None, :, 2]
            m = (dx * dx + dy * dy + dz * dz).min(dim=1)
            i1 = min(i0 + rows, lp)
            d2[n, i0:i1], idx[n, i0:i1] = m.values, m.indices
    return (d2, idx) if return_idx else d2


def nn_dist2(p, q, lengths_p=None, lengths_q=None, return_idx=False):
    """p [N, S1, 3], q [N, S2, 3] float32 (either may have batch 1 and is then shared by all N) -> d2 [N, S1]: for every valid point
    of p[n] the smallest squared distance (ax-bx)^2 + (ay-by)^2 + (az-bz)^2, in fp32, to a valid point of q[n]; with return_idx also
    the int64 index of a point that attains it.  lengths_* (int64 [N]): rows at and beyond a length are padding - never read, written
    as 0 / -1.  An empty q[n] gives +inf / -1.  Non-contiguous inputs are copied; mixed devices and other dtypes raise."""
    N = _check_clouds(p, q)
    lengths_p, lengths_q = _check_lengths(lengths_p, N, p.shape[1], p.device), _check_lengths(lengths_q, N, q.shape[1], p.device)
    if p.is_cuda:
        from .. import ops
        return ops.nn_dist2(p.contiguous(), q.contiguous(), lengths_p, lengths_q, return_idx)
    return _nn_dist2_cpu(p, q, lengths_p, lengths_q, return_idx)


def _counts_cpu(d2, thresholds, lengths):
    N, S = d2.shape
    valid = torch.ones((N, S), dtype=torch.bool) if lengths is None else torch.arange(S)[None, :] < lengths[:, None]
    d = d2.sqrt()
    counts = torch.stack([((d < torch.tensor(t, dtype=torch.float32)) & valid).sum(1) for t in thresholds], dim=1).to(torch.int32)
    return counts, torch.where(valid, d2, torch.zeros(())).sum(1)


def f1_from_counts(count_p, count_q, len_p, len_q, eps=1e-8):
    """The reference's expression in torch fp32: count_* int [N, T], len_* [N] (or a number) -> (precision, recall, f1) [T, N]."""
    lp = torch.as_tensor(len_p, device=count_p.device).to(torch.float32).reshape(-1, 1)
    lq = torch.as_tensor(len_q, device=count_p.device).to(torch.float32).reshape(-1, 1)
    precision = (100.0 * (count_p.to(torch.float32) / lp)).t()
    recall = (100.0 * (count_q.to(torch.float32) / lq)).t()
    f1 = (2.0 * precision * recall) / (precision + recall + eps)
    return precision, recall, f1


def sampling_counts(pred_points, gt_points, thresholds=(0.1,), lengths_pred=None, lengths_gt=None):
    """Both directions' (counts int32 [N, T], sum of d2 fp32 [N]): (count_pred, sum_pred, count_gt, sum_gt)."""
    N = _check_clouds(pred_points, gt_points)
    lp = _check_lengths(lengths_pred, N, pred_points.shape[1], pred_points.device)
    lg = _check_lengths(lengths_gt, N, gt_points.shape[1], pred_points.device)
    d2p = nn_dist2(pred_points, gt_points, lp, lg)
    d2g = nn_dist2(gt_points, pred_points, lg, lp)
    if pred_points.is_cuda:
        from .. import ops
        return (*ops.f1_counts(d2p, thresholds, lp), *ops.f1_counts(d2g, thresholds, lg))
    return (*_counts_cpu(d2p, thresholds, lp), *_counts_cpu(d2g, thresholds, lg))


def compute_sampling_metrics(pred_points, gt_points, thresholds=(0.1,), eps=1e-8, lengths_pred=None, lengths_gt=None):
    """The reference's _compute_sampling_metrics with every metric kept: a dict of (N,) fp32 tensors "F1@%f" % t, "Precision@%f" % t,
    "Recall@%f" % t for every threshold and "Chamfer-L2" (mean d2 pred -> gt + mean d2 gt -> pred).  A cloud of length 0 gives NaN
    (the mean of nothing), as the reference's expression would."""
    thresholds = [float(t) for t in thresholds]
    if not 1 <= len(thresholds) <= 8:
        raise ValueError("1 to 8 thresholds")
    N = _check_clouds(pred_points, gt_points)
    S1, S2 = pred_points.shape[1], gt_points.shape[1]
    lp = _check_lengths(lengths_pred, N, S1, pred_points.device)
    lg = _check_lengths(lengths_gt, N, S2, pred_points.device)
    cp, sp, cg, sg = sampling_counts(pred_points, gt_points, thresholds, lp, lg)
    if pred_points.is_cuda:
        from .. import ops
        precision, recall, f1, chamfer = ops.f1_finalize(cp, cg, sp, sg, S1, S2, eps, lp, lg)
    else:
        flp = torch.full((N,), S1) if lp is None else lp
        flg = torch.full((N,), S2) if lg is None else lg
        precision, recall, f1 = f1_from_counts(cp, cg, flp, flg, eps)
        chamfer = sp / flp.to(torch.float32) + sg / flg.to(torch.float32)
    metrics = {}
    for k, t in enumerate(thresholds):
        metrics["F1@%f" % t], metrics["Precision@%f" % t], metrics["Recall@%f" % t] = f1[k], precision[k], recall[k]
    metrics["Chamfer-L2"] = chamfer
    return metrics


def f1_score(pred_points, gt_points, threshold=0.1):
    """What the reference function returns: the (N,) F1 at one threshold."""
    return compute_sampling_metrics(pred_points, gt_points, thresholds=(threshold,))["F1@%f" % threshold]


def scale_to_gt(pred_points, gt_points, target=10.0):
    """The reference's scale="gt-10" rule on point clouds: both clouds of a pair times target / (longest bounding-box edge of the
    ground-truth cloud).  Opt-in: cached clouds of the reference were sampled from meshes that were already scaled."""
    long_edge = (gt_points.amax(dim=1) - gt_points.amin(dim=1)).amax(dim=1)
    scale = (target / long_edge)[:, None, None]
    return pred_points * scale, gt_points * scale


def _load_cloud(path):
    a = np.load(path)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{path}: expected [1, S, 3] or [S, 3], got {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _load_category_map(category_map):
    if category_map is None or isinstance(category_map, dict):
        return category_map or {}
    with open(category_map) as f:                                                   # the reference's val_map.json
        return {item["model_id"]: item["category"] for item in json.load(f)}


def fill_point_cache(model_ids, point_cache_dir, mesh_root, category_map, num_samples=10000, seed=0, batch=64, device=None):
    """Sample <mesh_root>/<category_map[id]>/<id>/models/model_normalized.obj for every id that has a mesh but no <dir>/<id>.npy
    and write the cloud as float32 [1, S, 3] (the reference's format), scaled to a longest bounding-box edge of 10 ("gt-10" on the
    mesh's own box).  Ids are taken in sorted order, `batch` meshes per launch; returns the ids written."""
    from . import mesh as _mesh
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    amap = _load_category_map(category_map)
    todo = []
    for mid in sorted(set(model_ids)):
        if mid in amap and not os.path.exists(os.path.join(point_cache_dir, mid + ".npy")):
            obj = os.path.join(mesh_root, amap[mid], mid, "models", "model_normalized.obj")
            if os.path.exists(obj):
                todo.append((mid, obj))
    if todo:
        os.makedirs(point_cache_dir, exist_ok=True)
    for b0 in range(0, len(todo), batch):
        chunk = todo[b0:b0 + batch]
        meshes = [_mesh.load_obj(obj) for _, obj in chunk]
        points = _mesh.sample_points_from_meshes([m[0] for m in meshes], [m[1] for m in meshes], num_samples, seed, "gt-10",
                                                 device=device).cpu().numpy()
        for i, (mid, _) in enumerate(chunk):
            np.save(os.path.join(point_cache_dir, mid + ".npy"), points[i:i + 1])
    return [mid for mid, _ in todo]


def shape_f1_from_nearest(nearest_path, point_cache_dir, threshold=0.1, batch=64, rescale=False, device=None, mesh_root=None,
                          category_map=None, num_samples=10000, seed=0):
    """What calculate_f1.py's main does: for every record of nearest.jsonl (as compute_metrics(nearest_path=...) writes it) the F1 of
    <dir>/<retrieved_models[0]>.npy against <dir>/<groundtruth.split("-")[0]>.npy.  With mesh_root (and category_map: a dict
    model id -> category, or the path of the reference's val_map.json) a shape without a cloud is first sampled from its
    model_normalized.obj into the directory (fill_point_cache).  Records with a shape that has neither a cloud nor a mesh are skipped
    and counted.  Returns {"mean_f1", "f1" (one value per record kept), "records" (their line numbers), "skipped"}."""
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    pairs = []
    with open(nearest_path) as f:
        for line_no, line in enumerate(f):
            if line.strip():
                rec = json.loads(line)
                pairs.append((line_no, rec["retrieved_models"][0], rec["groundtruth"].split("-")[0]))
    if mesh_root is not None:
        fill_point_cache([mid for pr in pairs for mid in pr[1:]], point_cache_dir, mesh_root, category_map, num_samples, seed, batch, device)
    have = lambda mid: os.path.exists(os.path.join(point_cache_dir, mid + ".npy"))            # noqa: E731
    kept = [pr for pr in pairs if have(pr[1]) and have(pr[2])]
    clouds, values = {}, []

    def cloud(mid):
        if mid not in clouds:
            clouds[mid] = _load_cloud(os.path.join(point_cache_dir, mid + ".npy"))
        return clouds[mid]

    def padded(items):
        S = max(c.shape[0] for c in items)
        out = torch.zeros((len(items), S, 3), dtype=torch.float32)
        for i, c in enumerate(items):
            out[i, :c.shape[0]] = c
        same = all(c.shape[0] == S for c in items)
        return out.to(device), None if same else torch.tensor([c.shape[0] for c in items], dtype=torch.int64, device=device)

    for b0 in range(0, len(kept), batch):
        chunk = kept[b0:b0 + batch]
        pred, lp = padded([cloud(pr[1]) for pr in chunk])
        gt, lg = padded([cloud(pr[2]) for pr in chunk])
        if rescale:
            if lp is not None or lg is not None:
                raise ValueError("rescale=True needs clouds of one size per batch (the bounding box would see the padding)")
            pred, gt = scale_to_gt(pred, gt)
        m = compute_sampling_metrics(pred, gt, thresholds=(threshold,), lengths_pred=lp, lengths_gt=lg)
        values += m["F1@%f" % threshold].cpu().tolist()
    return {"mean_f1": sum(values) / len(values) if values else float("nan"), "f1": values, "records": [pr[0] for pr in kept],
            "skipped": len(pairs) - len(kept)}


def main(argv=None):
    ap = argparse.ArgumentParser(description="mean shape F1 of the top-1 retrieved shapes of a nearest.jsonl")
    ap.add_argument("nearest")
    ap.add_argument("--point-cache", required=True, help="directory of <model_id>.npy clouds ([1, S, 3] or [S, 3] float32)")
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rescale", action="store_true", help="apply the gt-10 scale to the clouds (cached clouds already carry it)")
    ap.add_argument("--mesh-root", default=None, help="ShapeNetCore.v2 directory: shapes without a cloud are sampled from "
                    "<root>/<category>/<id>/models/model_normalized.obj into the point cache")
    ap.add_argument("--category-map", default=None, help="val_map.json of the reference: a list of {model_id, category}")
    ap.add_argument("--num-samples", type=int, default=10000, help="points per sampled mesh")
    ap.add_argument("--seed", type=int, default=0, help="seed of the surface sampler")
    a = ap.parse_args(argv)
    r = shape_f1_from_nearest(a.nearest, a.point_cache, a.threshold, a.batch, a.rescale, mesh_root=a.mesh_root,
                              category_map=a.category_map, num_samples=a.num_samples, seed=a.seed)
    if r["skipped"]:
        print(f"skipped {r['skipped']} of {r['skipped'] + len(r['f1'])} records: neither a point cloud in {a.point_cache} nor a mesh")
    print(r["mean_f1"])


if __name__ == "__main__":
    main()
