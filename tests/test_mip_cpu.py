"""CPU: mip-mapped textures - ops.texture_mips and ops.render_views_textured(..., mips=) on CPU tensors, the torch restatements of
csrc/raster.hip's pyramid kernel and mip resolve kernels - against the integer pyramid and the float64 level of detail of
tests/mip_reference.py; what the feature is for (a minified checker renders as its mean, which the plain textured call cannot
form); the identities that tie the mode to the existing calls byte for byte; the refusals; and python -m
tricolo_amd.data.preprocess --textures mip end to end on the host.

The scenes are those of tests/test_texture_cpu.py (random UVs in [-2, 3] on faces a few pixels across) with random-noise textures
of 1 x 1, 2 x 3, 5 x 7, 16 x 16, 1 x 9 and 64 x 64 texels; visibility is not touched by the feature, so the pixels left out of a
comparison are raster_reference's `ambiguous` ones, under its 1 % cap.  Colours may differ from float64 by 1 LSB, the allowance of
tests/test_texture_cpu.py: the level rule is continuous in rho (at rho = 1, at every octave, at the top level), so the fp32 error
of the footprint - some 1e-5 of a texel after the cancellation in u_x - u with |u| <= 3 and 64 texels - moves the blend weight by
1e-5 and a colour across a rounding boundary of floor(255 c + 0.5) at most.

check_mip_identities(device) and check_refusals(device) run here on the host and from tests/test_gpu_mip.py on the GPU."""
import os

import numpy as np
import pytest
import torch

from tests import mip_reference as mr
from tests import test_preprocess as tp
from tests import test_texture_cpu as tc
from tricolo_amd import _C, ops
from tricolo_amd import config as tcfg
from tricolo_amd.data import preprocess as pp
from tricolo_amd.data import render as R
from tricolo_amd.meshes import MeshBatch, check_texture_mips, mip_level_sizes

MIP_SIZES = [(1, 1), (2, 3), (5, 7), (16, 16), (1, 9), (64, 64)]                       # (height, width)
CHAIN = [1, 6 + 1, 35 + 6 + 1, 256 + 64 + 16 + 4 + 1, 9 + 4 + 2 + 1, 4096 + 1024 + 256 + 64 + 16 + 4 + 1]


def mip_textures(seed=21):
    return tc.noise_textures(seed, MIP_SIZES)


def scene(name, shift=0):
    """tests/test_texture_cpu.scene with the six textures of MIP_SIZES: material j takes texture (j + shift) % 6."""
    s = tc.scene(name, shift)
    s["texs"] = mip_textures()
    s["mt"] = torch.tensor([(j + shift) % 6 for j in range(s["kd"].shape[0])], dtype=torch.int32)
    return s


def mipped(batch, cam, H, W, yfov=R.YFOV, samples=1, **fields):
    """(image, vis) of ops.render_views_textured with the pyramid of the batch's textures, on the CPU; fields: texture tensors that
    replace the batch's (the pyramid is built from the replaced ones), or mips= itself."""
    tex = dict(zip(("face_uv", "mat_tex", "texels", "tex_off", "tex_size"), batch.texture_tensors))
    mips = fields.pop("mips", None)
    tex.update(fields)
    if mips is None:
        mips = ops.texture_mips(tex["texels"], tex["tex_off"], tex["tex_size"])
    img, vis = ops.render_views_textured(*batch.tensors, *tex.values(), cam.to(batch.verts.device), H, W, yfov, R.ZNEAR, return_visibility=True,
                                         samples=samples, mips=mips)
    return img.cpu(), vis.cpu()


def plain(batch, cam, H, W, yfov=R.YFOV, samples=1, mat_kd=None):
    t = list(batch.tensors)
    if mat_kd is not None:
        t[5] = mat_kd.to(batch.verts.device)
    img, vis = ops.render_views(*t, cam.to(batch.verts.device), H, W, yfov, R.ZNEAR, return_visibility=True, samples=samples)
    return img.cpu(), vis.cpu()


def textured(batch, cam, H, W, yfov=R.YFOV, samples=1, **fields):
    tex = dict(zip(("face_uv", "mat_tex", "texels", "tex_off", "tex_size"), batch.texture_tensors))
    tex.update(fields)
    img, vis = ops.render_views_textured(*batch.tensors, *tex.values(), cam.to(batch.verts.device), H, W, yfov, R.ZNEAR, return_visibility=True,
                                         samples=samples)
    return img.cpu(), vis.cpu()


# ---------------------------------------------------------------------------------------------------- 1. the pyramid
def packed_textures(texs, device="cpu"):
    tri = tc.scene("triangle", 0)
    tri["texs"], tri["mt"] = texs, torch.tensor([0], dtype=torch.int32)
    return tc.pack([tri], device)


def check_pyramids(device="cpu"):
    texs = mip_textures()
    batch = packed_textures(texs, device)
    mip_texels, mip_off = ops.texture_mips(batch.texels, batch.tex_off, batch.tex_size)
    assert mip_texels.dtype == torch.uint8 and mip_off.dtype == torch.int64 and mip_texels.device.type == mip_off.device.type == torch.device(device).type
    assert mip_off.tolist() == [0] + np.cumsum(CHAIN).tolist() and tuple(mip_texels.shape) == (sum(CHAIN), 4)       # offsets of a batch of six
    check_texture_mips(mip_texels, mip_off, batch.tex_size)
    got, off = mip_texels.cpu().numpy(), mip_off.tolist()
    for t, tex in enumerate(texs):
        levels = mr.cached_pyramid(tex)
        sizes = mip_level_sizes(*tex.shape[:2])
        assert [lv.shape[:2] for lv in levels] == sizes and len(sizes) == int(np.floor(np.log2(max(tex.shape[:2])))) + 1
        assert np.array_equal(got[off[t]:off[t] + tex.shape[0] * tex.shape[1]], tex.reshape(-1, 4)), f"texture {t}: level 0 is the texture"
        assert np.array_equal(got[off[t]:off[t + 1]], mr.chain(levels)), f"texture {t} against the integer reference"
    assert mip_level_sizes(1, 9) == [(1, 9), (1, 4), (1, 2), (1, 1)] and mip_level_sizes(5, 7) == [(5, 7), (2, 3), (1, 1)]
    t16 = texs[3][:, :, :3].astype(np.int64)                                             # 16 x 16: the rounded mean of the 2^l x 2^l block
    at = off[3]
    for l in range(5):
        n, b = 16 >> l, 1 << l
        want = (2 * t16.reshape(n, b, n, b, 3).sum((1, 3)) + b * b) // (2 * b * b)
        assert np.array_equal(got[at:at + n * n, :3].astype(np.int64), want.reshape(-1, 3)), f"16 x 16, level {l}"
        assert (got[at:at + n * n, 3] == 255).all()
        at += n * n
    colour = np.array([200, 17, 255, 255], np.uint8)                                     # a constant texture is constant at every level
    const = packed_textures([np.broadcast_to(colour, (h, w, 4)).copy() for h, w in MIP_SIZES], device)
    flat = ops.texture_mips(const.texels, const.tex_off, const.tex_size)[0].cpu().numpy()
    assert flat.shape == (sum(CHAIN), 4) and (flat == colour).all()
    empty = ops.texture_mips(batch.texels[:0].contiguous(), batch.tex_off[:1].contiguous(), batch.tex_size[:0].contiguous())        # T == 0
    assert tuple(empty[0].shape) == (0, 4) and empty[1].tolist() == [0]


def test_pyramids_match_the_integer_reference():
    check_pyramids()


def test_a_batch_carries_its_pyramid():
    s = scene("triangle", 2)
    batch = tc.pack([s])
    assert batch.mip_tensors is None and batch.mip_texels is None
    with_mips = batch.with_texture_mips()
    assert with_mips.mip_tensors is not None and with_mips.texture_tensors[2] is batch.texels and len(with_mips.texture_tensors) == 5
    assert with_mips.mip_off.tolist() == [0] + np.cumsum(CHAIN).tolist()
    a = R.render_batch(with_mips, 2, 16, textures="mip")
    b = R.render_batch(batch, 2, 16, textures="mip")                                     # builds the pyramid itself
    assert torch.equal(a, b) and not torch.equal(a, R.render_batch(batch, 2, 16, textures=True))
    with pytest.raises(ValueError, match="packed without textures"):
        MeshBatch.pack([s["verts"]], [s["faces"]], [s["fm"]], [s["kd"]]).with_texture_mips()
    with pytest.raises(ValueError, match="textures must be"):
        R.render_batch(batch, 2, 16, textures="trilinear")


# ---------------------------------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("name,shift", [("triangle", 0), ("triangle", 1), ("triangle", 2), ("triangle", 3), ("triangle", 4), ("triangle", 5),
                                        ("soup", 0), ("soup", 3), ("quads", 1), ("quads", 4)])
def test_restatement_matches_the_float64_reference(name, shift, samples):
    s = scene(name, shift)
    if name == "soup":
        s["uv"][5] = float("nan")                                                        # a face without texture coordinates among the others
        s["cam"] = s["cam"][:2]
    img, vis = mipped(tc.pack([s]), s["cam"][None], s["H"], s["W"], s["yfov"], samples)
    compared = worst = 0
    seen = set()
    for k in range(s["cam"].shape[0]):
        want, face, ambiguous, rho = mr.render(s["verts"], s["faces"], s["fm"], s["kd"], s["uv"], s["mt"], s["texs"], s["cam"][k], s["H"], s["W"],
                                               s["yfov"], samples=samples)
        keep = ~ambiguous
        assert np.array_equal(vis[0, k].numpy()[keep], face[keep])
        assert ambiguous.sum() <= 0.01 * (face >= 0).sum()
        clean = keep if samples == 1 else keep.all(-1)                                   # a pixel is compared when none of its samples is ambiguous
        diff = np.abs(img[0, k].numpy().astype(int) - want.astype(int))[:, clean]
        compared, worst = compared + int((face[keep] >= 0).sum()), max(worst, int(diff.max()))
        seen |= {"magnified" if r <= 1 else "unbounded" if np.isinf(r) else "minified" for r in rho[np.isfinite(rho) | np.isinf(rho)].ravel()}
    print(f"{name}, textures shifted by {shift}, {samples} sample(s): {compared} covered compared, largest colour difference {worst}, footprints {sorted(seen)}")
    assert compared > (100 if name == "soup" else 20) and worst <= 1


# ---------------------------------------------------------------------------------------------------- 3. the point of the feature
def checker_scene():
    """A camera-facing quad over about 12 x 12 pixels of a 16 x 16 image; its 64 x 64 texture alternates 0 and 255 from texel to
    texel, so every pyramid level from 1 up is exactly 128 (the mean 127.5, half rounded up).  The flat camera's quad is edge-on
    to the light, shade 0.1: a Kd of 10, 6, 8 brings the colours back into the u8 range.  The quad starts 72/256 of a pixel left of
    and above the centre of pixel 2, so that 64 / 12 texels per pixel put every third pixel centre exactly on a texel centre: there
    the plain bilinear tap returns one texel, 0 or 255, and the aliasing shows at full contrast."""
    lo, hi = 2.0 + 56 / 256, 14.0 + 56 / 256                                             # the centre of pixel 2 lies on a texel centre (see above)
    pts = [(lo, lo), (hi, lo), (hi, hi), (lo, hi)]
    verts = tp.flat_vertices(pts, 16, 16)
    ij = np.add.outer(np.arange(64), np.arange(64)) % 2
    tex = np.stack([255 * ij, 255 * ij, 255 * ij, np.full_like(ij, 255)], 2).astype(np.uint8)
    uv = torch.tensor([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], dtype=torch.float32)
    return dict(verts=verts, faces=torch.tensor([[0, 1, 2], [0, 2, 3]]), fm=torch.zeros(2, dtype=torch.int32), kd=torch.tensor([[10.0, 6.0, 8.0]]), uv=uv,
                mt=torch.zeros(1, dtype=torch.int32), texs=[tex], cam=tp.FLAT_CAM[0], H=16, W=16, yfov=tp.FLAT_YFOV)


def check_checker(device="cpu"):
    s = checker_scene()
    batch = tc.pack([s], device)
    mips = ops.texture_mips(batch.texels, batch.tex_off, batch.tex_size)
    assert (mips[0][64 * 64:, :3] == 128).all() and mips[0].shape[0] == CHAIN[5]
    cam = s["cam"][None]
    _, face, ambiguous, rho = mr.render(s["verts"], s["faces"], s["fm"], s["kd"], s["uv"], s["mt"], s["texs"], s["cam"][0], 16, 16, s["yfov"])
    inside = torch.from_numpy((face >= 0) & ~ambiguous & (rho >= 2.0))
    assert inside.sum() >= 100 and 4.0 < np.nanmax(rho) < 8.0                            # 64 texels over 12 pixels: rho about 5.3
    got = mipped(batch, cam, 16, 16, s["yfov"], mips=mips)
    want = plain(batch, cam, 16, 16, s["yfov"], mat_kd=s["kd"] * torch.tensor(128.0 / 255.0, dtype=torch.float32))
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0][0, 0][:, inside], want[0][0, 0][:, inside])                # byte for byte the mean colour
    bare = textured(batch, cam, 16, 16, s["yfov"])[0][0, 0][:, inside].to(torch.int32)
    spread = int(bare[0].max() - bare[0].min())
    print(f"checker: {int(inside.sum())} interior pixels; without mips their red channel spans {spread} of 255, with mips it is {int(got[0][0, 0, 0][inside].max())}")
    assert spread > 128                                                                  # without mips: texels picked at random


def test_a_minified_checker_renders_as_its_mean():
    check_checker()


# ---------------------------------------------------------------------------------------------------- 4. identities, byte for byte
def check_mip_identities(device="cpu"):
    soup, tri = tc.scene("soup", 1), tc.scene("triangle", 3)
    tri["cam"] = R.pack_cameras([R.bbox_center(tri["verts"])], 3)[0]
    batch = tc.pack([soup, tri], device)
    cam, H, W = torch.stack([soup["cam"], tri["cam"]]), 32, 48
    for samples in (1, 4):
        base = plain(batch, cam, H, W, samples=samples)
        assert (base[1] >= 0).sum() > 100
        ref = mipped(batch, cam, H, W, samples=samples)
        on = textured(batch, cam, H, W, samples=samples)
        assert torch.equal(ref[1], base[1]) and not torch.equal(ref[0], base[0]) and not torch.equal(ref[0], on[0])
        # every footprint below one texel: the colours of the call without mips.  The soup has slivers a fraction of a pixel wide whose
        # UVs still change by several texels per pixel at 1 / 64 (7 pixels there keep rho > 1), so the UVs are scaled down by 2^-12
        small = batch.face_uv * 2.0 ** -12
        got, want = mipped(batch, cam, H, W, samples=samples, face_uv=small), textured(batch, cam, H, W, samples=samples, face_uv=small)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(want[0], base[0]), f"magnified, {samples} sample(s)"
        # no material has a texture; no face has texture coordinates; no texture in the batch at all
        none = torch.full_like(batch.mat_tex, -1)
        for what, img in (("mat_tex -1", mipped(batch, cam, H, W, samples=samples, mat_tex=none)),
                          ("NaN face_uv", mipped(batch, cam, H, W, samples=samples, face_uv=torch.full_like(batch.face_uv, float("nan")))),
                          ("T == 0", mipped(batch, cam, H, W, samples=samples, mat_tex=none, texels=batch.texels[:0].contiguous(),
                                            tex_off=batch.tex_off[:1].contiguous(), tex_size=batch.tex_size[:0].contiguous()))):
            assert torch.equal(img[0], base[0]) and torch.equal(img[1], base[1]), f"{what}, {samples} sample(s)"
        # a constant texture of colour c under Kd = 1 is Kd = fl32(c) / 255, at any size and any UV scale
        colour = np.array([200, 17, 255], np.uint8)
        kd = (torch.tensor([200.0, 17.0, 255.0]) / 255.0).expand(batch.mat_kd.shape[0], 3).contiguous()
        want = plain(batch, cam, H, W, samples=samples, mat_kd=kd)
        uv = batch.face_uv.clone()
        uv[0:40] = uv[0:40] * 1e6
        uv[40:80] = -uv[40:80] - 7.25
        uv[80:120] = uv[80:120] * 1e-4
        s2, t2 = dict(soup), dict(tri)
        for s in s2, t2:
            s["texs"] = [np.broadcast_to(np.concatenate([colour, [255]]).astype(np.uint8), (h, w, 4)).copy() for h, w in tc.TEXTURE_SIZES]
            s["kd"] = torch.ones_like(s["kd"])
        got = mipped(tc.pack([s2, t2], device), cam, H, W, samples=samples, face_uv=uv.to(device))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"constant texture, {samples} sample(s)"
        # the winding of a face, its UVs permuted alike; the order of the faces, their UVs and materials with them
        s3 = tc.scene("soup", 1)
        flip = torch.arange(s3["faces"].shape[0]) % 2 == 0
        order = torch.where(flip[:, None], torch.tensor([0, 2, 1]), torch.tensor([0, 1, 2]))
        s3["faces"], s3["uv"] = s3["faces"].gather(1, order), s3["uv"].gather(1, order[:, :, None].expand(-1, 3, 2))
        got = mipped(tc.pack([s3, tri], device), cam, H, W, samples=samples)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"winding, {samples} sample(s)"
        s4 = tc.scene("soup", 1)
        perm = torch.from_numpy(np.random.default_rng(8).permutation(s4["faces"].shape[0]))
        for key in ("faces", "uv", "fm"):
            s4[key] = s4[key][perm]
        got = mipped(tc.pack([s4, tri], device), cam, H, W, samples=samples)
        assert torch.equal(got[0], ref[0]), f"face order, {samples} sample(s)"
        vis = got[1][0].to(torch.int64)
        assert torch.equal(torch.where(vis >= 0, perm[vis.clamp(min=0)], vis), ref[1][0].to(torch.int64)), f"face order, {samples} sample(s)"


def test_identities():
    check_mip_identities()


# ---------------------------------------------------------------------------------------------------- 5. refusals
def check_refusals(device="cpu", elsewhere="meta"):
    """elsewhere: a device that is not the batch's - a pyramid there is refused before any of its bytes is looked at."""
    s = scene("triangle", 3)
    batch = tc.pack([s], device)
    m, o = ops.texture_mips(batch.texels, batch.tex_off, batch.tex_size)
    cam = s["cam"][None]
    for bad, match in (((m[:-1].contiguous(), o), "hold .* texels"), ((torch.cat([m, m[:1]]), o), "hold .* texels"),
                       ((m.to(torch.int32), o), "mip_texels"), ((m[:, :3].contiguous(), o), "mip_texels"), ((m, o.to(torch.int32)), "mip_off"),
                       ((m, o[:-1].contiguous()), "mip_off"), ((m, torch.cat([o[:1], o[1:2] + 1, o[2:]])), "running sum"), ((m,), "pair"), (m, "pair"),
                       ((m.to(elsewhere), o.to(elsewhere)), "one device"), ((m, o.to(elsewhere)), "one device")):
        with pytest.raises(ValueError, match=match):
            mipped(batch, cam, 8, 8, mips=bad)
    with pytest.raises(ValueError, match="samples"):
        mipped(batch, cam, 8, 8, samples=2, mips=(m, o))
    other = ops.texture_mips(*packed_textures(tc.noise_textures(5, MIP_SIZES[:5] + [(32, 32)]), device).texture_tensors[2:])      # of other textures
    with pytest.raises(ValueError, match="another batch"):
        mipped(batch, cam, 8, 8, mips=other)
    with pytest.raises(ValueError, match="mip_off must be the running sum"):
        check_texture_mips(m, o + 1, batch.tex_size)
    with pytest.raises(ValueError, match="mip_texels"):
        check_texture_mips(m.to(torch.int16), o, batch.tex_size)
    for bad, match in (((batch.texels[:-1].contiguous(), batch.tex_off, batch.tex_size), "texels"),
                       ((batch.texels, batch.tex_off[:-1].contiguous(), batch.tex_size), "tex_off"),
                       ((batch.texels, batch.tex_off, batch.tex_size.to(torch.int64)), "tex_size"),
                       ((batch.texels, batch.tex_off, torch.zeros_like(batch.tex_size)), "H, W")):
        with pytest.raises(ValueError, match=match):
            ops.texture_mips(*bad)


def test_refusals_before_anything_runs():
    check_refusals()
    # the C entry points themselves: sizes and counts are checked before any pointer is touched, so null pointers and no GPU will do
    lib = _C.lib()
    tail = [None, None, None, None]                                                      # workspace, image, visibility, stream

    def null(N, T, fields=_C.TRI_MESH_TEXTURES | _C.TRI_MESH_MIPS):                      # every pointer null, textures and pyramid declared
        return _C.TriMeshBatch(N=N, T=T, fields=fields)

    rc = lib.tri_raster_render(null(1, 0), None, 200, 3, 13378, 13378, R.YFOV, R.ZNEAR, 4, *tail)
    assert rc == _C.TRI_ERR_UNSUPPORTED
    message = lib.tri_last_error().decode()
    assert "tri_raster_render" in message and "2^31 or more samples" in message and "split the batch" in message
    assert lib.tri_raster_render(null(1, -1), None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 1, *tail) == _C.TRI_ERR_ARG       # a negative texture count
    assert lib.tri_raster_render(null(1, 0), None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 2, *tail) == _C.TRI_ERR_ARG        # two samples
    assert "samples must be 1 or 4" in lib.tri_last_error().decode()
    assert lib.tri_raster_render(null(1, 3), None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 1, *tail) == _C.TRI_ERR_ARG        # textures without their fields
    assert "both pyramid fields" in lib.tri_last_error().decode()
    assert lib.tri_raster_render(null(1, 0), None, 200, 3, 8, 8, 4.0, R.ZNEAR, 4, *tail) != 0                       # yfov beyond pi
    for samples in (1, 4):
        assert lib.tri_raster_render(null(0, 0), None, 0, 3, 8, 8, R.YFOV, R.ZNEAR, samples, *tail) == 0            # nothing to draw: nothing runs
    assert lib.tri_texture_mips(None, None, None, -1, 0, None, 0, None, None) == _C.TRI_ERR_ARG
    assert lib.tri_texture_mips(None, None, None, 2, -1, None, 3, None, None) == _C.TRI_ERR_ARG
    assert lib.tri_texture_mips(None, None, None, 2, 5, None, 7, None, None) == _C.TRI_ERR_ARG                                    # sizes without arrays
    assert "tri_texture_mips" in lib.tri_last_error().decode()
    assert lib.tri_texture_mips(None, None, None, 0, 0, None, 0, None, None) == 0                                                 # an empty pyramid: nothing runs


def test_the_batch_descriptor_is_checked_by_one_rule_set_for_every_mesh_call():
    """csrc/mesh_batch.h mb_from_abi: a null descriptor, a negative N, a group the callee does not take and a pyramid without textures are
    TRI_ERR_ARG before anything runs (null pointers and no GPU will do), and the message begins with the callee's name."""
    lib = _C.lib()
    tail = [None, None, None, None]                                                      # workspace, image / grid, visibility / labels, stream

    def null(N, T, fields):
        return _C.TriMeshBatch(N=N, T=T, fields=fields)

    assert lib.tri_raster_render(null(1, 0, _C.TRI_MESH_MIPS), None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 1, *tail) == _C.TRI_ERR_ARG     # a pyramid without textures
    assert lib.tri_last_error().decode().startswith("tri_raster_render: ") and "TRI_MESH_TEXTURES" in lib.tri_last_error().decode()
    assert lib.tri_raster_render(None, None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 1, *tail) == _C.TRI_ERR_ARG                             # no descriptor
    assert lib.tri_last_error().decode().startswith("tri_raster_render: ")
    assert lib.tri_raster_render(null(1, 0, 16), None, 200, 3, 8, 8, R.YFOV, R.ZNEAR, 1, *tail) == _C.TRI_ERR_ARG                   # a bit no call takes
    assert lib.tri_voxelize_meshes(null(1, 0, _C.TRI_MESH_PBR), None, 5, 32, 1, *tail) == _C.TRI_ERR_ARG                             # a group this call does not take
    assert lib.tri_last_error().decode().startswith("tri_voxelize_meshes: ")
    assert lib.tri_voxelize_meshes(None, None, 5, 32, 1, *tail) == _C.TRI_ERR_ARG
    assert lib.tri_last_error().decode().startswith("tri_voxelize_meshes: ")
    assert lib.tri_mesh_face_colours(null(1, 0, _C.TRI_MESH_TEXTURES | _C.TRI_MESH_MIPS), 5, None, None) == _C.TRI_ERR_ARG           # colours take textures, no pyramid
    assert lib.tri_last_error().decode().startswith("tri_mesh_face_colours: ")
    assert lib.tri_mesh_face_colours(null(1, 3, _C.TRI_MESH_TEXTURES), 5, None, None) == _C.TRI_ERR_ARG
    assert "T > 0 needs all five texture fields" in lib.tri_last_error().decode() and "pyramid" not in lib.tri_last_error().decode()
    for call in (lambda b: lib.tri_mesh_bbox(b, None, None), lambda b: lib.tri_mesh_face_cdf(b, None, 5, None, None, None),
                 lambda b: lib.tri_mesh_sample_points(b, None, None, None, 5, 0, None, None, None),
                 lambda b: lib.tri_mesh_vertex_normals(b, 5, 5, 0, None, None, None, None)):
        assert call(None) == _C.TRI_ERR_ARG and call(null(1, 0, _C.TRI_MESH_NORMALS)) == _C.TRI_ERR_ARG
        assert call(null(-1, 0, 0)) == _C.TRI_ERR_ARG and "negative size" in lib.tri_last_error().decode()


# ---------------------------------------------------------------------------------------------------- 6. the command line
def test_preprocess_with_mips_end_to_end_on_the_host(tmp_path):
    """Two models, chairA with a 128 x 128 noise texture over its top (minified in a 224 x 224 view) and tableB without one:
    --textures mip writes what render_meshes(..., textures="mip") gives, changes chairA's images against --textures on and leaves
    tableB's images and every voxel grid exactly as --textures on writes them."""
    pytest.importorskip("PIL")
    from PIL import Image

    from tests import test_texture_parser as ttp
    from tricolo_amd.data.dataset import PackedDataset
    from tricolo_amd.data.materials import load_obj_textured
    runs = {}
    for mode in ("on", "mip"):
        root = str(tmp_path / mode)
        overrides = [o for o in tp.write_dataset(root) if not o.startswith("data.ignored_models")]
        overrides.append("data.ignored_models=[04379243/ignoredD,03001627/chairC]")
        obj_root = os.path.join(root, "text2shape-data", "ShapeNetCore.v2")
        ttp.textured_model(obj_root, *tp.MODELS[0])
        noise = np.random.default_rng(2).integers(0, 256, (128, 128, 3), dtype=np.uint8)
        Image.fromarray(noise).save(os.path.join(obj_root, *tp.MODELS[0], "images", "texture0.png"))
        stats = pp.main(overrides + ["--device", "cpu", "--voxels", "mesh", "--textures", mode], log=lambda *a: None)
        assert stats["train"] == {"models": 2, "written": 2, "skipped": 0, "textured_models": 1, "texture_failures": 1}
        cfg = tcfg.compose(overrides=overrides)
        runs[mode] = {m: dict(np.load(os.path.join(cfg.data.exp_data_root_path, c, f"{m}.npz"))) for c, m in tp.MODELS[:2]}
    meshes = [load_obj_textured(os.path.join(obj_root, c, m, "models", "model_normalized.obj")) for c, m in tp.MODELS[:2]]
    lists = [[m[j] for m in meshes] for j in range(4)]
    want = R.render_meshes(*lists, num_views=int(cfg.data.num_views), textures="mip", face_uv_list=[m[5] for m in meshes],
                           mat_tex_list=[m[6] for m in meshes], textures_list=[m[7] for m in meshes])
    for k, (_, m) in enumerate(tp.MODELS[:2]):
        assert runs["mip"][m]["images"].dtype == np.uint8 and np.array_equal(runs["mip"][m]["images"], want[k].numpy()), m
        for name in ("voxel32", "voxel64", "voxel128"):
            assert np.array_equal(runs["mip"][m][name], runs["on"][m][name]), (m, name)       # the voxel colours are those of --textures on
    assert np.array_equal(runs["mip"]["tableB"]["images"], runs["on"]["tableB"]["images"])
    changed = (runs["mip"]["chairA"]["images"] != runs["on"]["chairA"]["images"]).any(1).mean()
    print(f"--textures mip changes {100 * changed:.1f} % of chairA's pixels against --textures on")
    assert changed > 0.005
    ds = PackedDataset(cfg, "train", device="cpu")                                        # the mip files, written last
    assert next(iter(ds.batches(2)(0)))["images"].dtype == torch.uint8
    assert "--textures off|on|mip" in pp.__doc__ and pp.TEXTURE_MODES == ("off", "on", "mip")
    with pytest.raises(SystemExit):
        pp.main(overrides + ["--textures", "trilinear"], log=lambda *a: None)
