"""Float64 model of the bicubic antialiased u8 resize (torchvision Resize(BICUBIC, antialias=True) on a uint8 tensor = float32,
ATen's _upsample_bicubic2d_aa, clamp(0, 255), round half to even, uint8), the geometries / plane counts / image contents the tests
share, and the acceptance rule.

Acceptance rule, on EVERY pixel: with y64 the float64 model value and TAU = 1e-3, a result must equal rint(clip(y64, 0, 255))
exactly where |frac(y64) - 0.5| >= TAU and may differ from it by at most 1 elsewhere (a value that close to a rounding boundary may
land on either side in fp32); identity geometries must return the input's bits.

Where TAU comes from: torch's own fp32 CPU result (F.interpolate before the clamp) differs from y64 by at most 2.4e-4 over the full
geometry list below with the random and the stripe contents at 3 planes (observed maxima: 224x224->128x128 6.6e-5,
224x224->224x224 0, 37x29->16x20 2.2e-4, 24x24->17x17 2.4e-4, 16x16->40x40 1.9e-4, 5x7->3x2 3.4e-5;
tests/test_resize_dataset.py re-measures them and asserts the largest stays below 5e-4, the point from which TAU would have to
become twice the observed maximum), and its u8 output has no mismatch outside the band.  TAU is ~4x the largest of these: room for
another fp32 summation order and fp32-rounded weights, while a wrong tap or weight moves values by 1e-2 and more.  Exact ties do
occur (y64 = k + 0.5 up to float64 rounding: the stripes and the ramp when upsampling, hundreds of pixels), and torch's own u8
result differs from rint(y64) by 1 on about a third of them - which is why the band allows 1 and no more.
"""
import functools

import numpy as np

TAU = 1e-3
TAU_REFERENCE_LIMIT = 5e-4                          # the measured fp32 deviation of torch must stay below this for TAU = 1e-3 to stand

# (Hin, Win, Hout, Wout)
GEOMETRIES = [
    (224, 224, 128, 128),                           # the real one
    (224, 224, 224, 224),                           # identity
    (37, 29, 16, 20),                               # odd, rectangular, no width a multiple of 4 or 16
    (24, 24, 17, 17),                               # non-integer ratio, windows clipped at both borders
    (16, 16, 40, 40),                               # upsampling, support 2
    (5, 7, 3, 2),                                   # window wider than the image
]
PLANES = [3, 21]                                    # 1 and 7 images: band and grid remainders
CONTENTS = ["random", "stripes", "const255", "const0", "ramp"]


def geom_id(g):
    return f"{g[0]}x{g[1]}to{g[2]}x{g[3]}"


def w(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def matrix(n_in, n_out):
    s = n_in / n_out
    sup = 2.0 * max(s, 1.0)
    inv = 1.0 / max(s, 1.0)
    M = np.zeros((n_out, n_in))
    for i in range(n_out):
        c = s * (i + 0.5)
        lo = max(int(c - sup + 0.5), 0)
        hi = min(int(c + sup + 0.5), n_in)
        j = np.arange(lo, hi)
        ww = w((j - c + 0.5) * inv)
        M[i, j] = ww / ww.sum()
    return M


def model64(x_u8, Hout, Wout):
    """x_u8 [..., Hin, Win] -> y64 [..., Hout, Wout] before the clamp."""
    x = np.asarray(x_u8)
    Hin, Win = x.shape[-2:]
    # = einsum("oi,...ij,pj->...op", My, x, Mx), as two matrix products (the one-step einsum walks all five indices at once)
    return np.matmul(matrix(Hin, Hout), np.matmul(x.astype(np.float64), matrix(Win, Wout).T))


def expected_u8(y64):
    return np.rint(np.clip(y64, 0, 255)).astype(np.uint8)


def band(y64):
    """True where y64 is within TAU of a rounding boundary."""
    return np.abs((y64 - np.floor(y64)) - 0.5) < TAU


def make_image(content, planes, H, W, seed=0):
    """u8 [planes // 3, 3, H, W] (planes is a multiple of 3)."""
    assert planes % 3 == 0
    shape = (planes // 3, 3, H, W)
    if content == "random":
        return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, size=shape, dtype=np.uint8)
    if content == "stripes":                        # one-pixel 0 / 255 stripes: bicubic overshoot, both clamps; rows, columns, checkers by plane
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pats = [(xx % 2), (yy % 2), ((xx + yy) % 2), ((xx // 2 + yy) % 2)]
        out = np.empty((planes, H, W), dtype=np.uint8)
        for p in range(planes):
            out[p] = (pats[p % 4] ^ (p // 4 % 2)) * 255
        return out.reshape(shape)
    if content == "const255":
        return np.full(shape, 255, dtype=np.uint8)
    if content == "const0":
        return np.zeros(shape, dtype=np.uint8)
    if content == "ramp":                           # horizontal ramp 0..255 across the width, the same in every row
        ramp = (np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)
        return np.broadcast_to(ramp, shape).copy()
    raise KeyError(content)


@functools.lru_cache(maxsize=None)
def case(geom, planes, content):
    """(x u8 [planes // 3, 3, Hin, Win], y64 [.., Hout, Wout]) - computed once per session, shared; treat as read-only."""
    Hin, Win, Hout, Wout = geom
    x = make_image(content, planes, Hin, Win)
    y = model64(x, Hout, Wout)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def check(result_u8, y64, what=""):
    """The acceptance rule on every pixel; returns (pixels in the band, pixels in the band that differ by 1) for reporting."""
    r = np.asarray(result_u8)
    assert r.dtype == np.uint8 and r.shape == y64.shape, f"{what}: {r.dtype} {r.shape} against {y64.shape}"
    want = expected_u8(y64)
    diff = np.abs(r.astype(np.int32) - want.astype(np.int32))
    near = band(y64)
    bad = (diff > 0) & ~near
    assert not bad.any(), (f"{what}: {int(bad.sum())} pixel(s) away from a rounding boundary differ from rint(clip(y64)); first at "
                           f"{tuple(np.argwhere(bad)[0])}: got {r[bad][0]}, y64 {y64[bad][0]:.6f}")
    assert diff.max(initial=0) <= 1, f"{what}: a pixel within TAU of a rounding boundary differs by {int(diff.max())}"
    return int(near.sum()), int((diff > 0).sum())
