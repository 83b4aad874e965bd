"""Generate tests/golden/conv_plan.npz: what the conv planner answers for a sweep of layer shapes.  TEST INFRASTRUCTURE.

    python tools/make_conv_plan_golden.py            # record the table of the library that is built now
    python tools/make_conv_plan_golden.py --sha256   # print the SHA-256s of the table under the current environment

The planner (conv_make_plan / wgrad_make_plan and the queries on top of them) answers without a GPU: the compute-unit count falls back
to 256, the MI355X's.  The file pins those answers so that a change to the routing code shows as a changed cell, not as a slower or
wrong layer somewhere else.  It holds

    desc            int32 [N, 16]   the descriptors, fields in TriConvDesc order, built as ops.ConvGeom builds them
    columns         str   [C]       name of each column (COLUMNS below)
    table           int64 [N, C]    every query's answer with no TRICOLO_* variable set
    switches        str   [S]       "NAME=value" A/B settings (SWITCHES below)
    switch_sha256   str   [S]       SHA-256 of the table recomputed with that one variable set
    route_columns   str   [R]       name of each column of the weight-gradient route table (ROUTE_COLUMNS below)
    route_table     int64 [N, R]    tri_conv_wgrad_route's answers with no TRICOLO_* variable set
    switch_sha256_all str [S]       SHA-256 of table and route_table side by side, recomputed with that one variable set

tests/test_conv_plan.py recomputes all of it.  Re-record only when a plan is MEANT to change, and say so in the commit.
"""
import argparse
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "conv_plan.npz")

SWITCHES = ["TRICOLO_NO_HALO=1", "TRICOLO_HALO_ROWS=0", "TRICOLO_HALO_ROWS=2", "TRICOLO_HALO_TM3=0", "TRICOLO_NO_DMA=1", "TRICOLO_NO_STEM=1",
            "TRICOLO_NO_VOX0=1", "TRICOLO_NO_VOXG=1", "TRICOLO_NO_VOXB=1", "TRICOLO_VOXB_32=1", "TRICOLO_NO_S2G=1", "TRICOLO_NO_C64_CONV=1",
            "TRICOLO_NO_S2D_CONV=1", "TRICOLO_NO_PW_CONV=1", "TRICOLO_VOXG_CT=16", "TRICOLO_VOXG_SPU=1", "TRICOLO_NO_KROW_WGRAD=1",
            "TRICOLO_NO_STEM_WGRAD=1"]

COLUMNS = ([f"family_{'dgrad' if tr else 'fwd'}_m{m}" for tr in (0, 1) for m in (0, 1, 2)] +
           [f"num_mtiles_m{m}" for m in (0, 1, 2)] + [f"num_records_rows_m{m}" for m in (0, 1, 2)] +
           ["workspace_fwd", "workspace_dgrad"] +
           [f"dgrad_bn_records_acc{a}_fmt{f}" for a in (0, 1) for f in (0, 1, 2)] +
           ["wgrad_workspace", "plan_bytes", "wgrad_family_fmt0", "wgrad_family_fmt1"] +
           [f"wgrad_group_{k}_fmt{f}" for f in (0, 1, 2) for k in ("rc", "family", "tiles", "steps")])
# tri_conv_wgrad_route per storage format and call features (ops.WGRAD_MASK / WGRAD_ROWS); the last three: the 3-product split on fp32
# storage.  A table of their own (route_table), recorded later than `table`: switch_sha256 stays the hash of `table` alone,
# switch_sha256_all is the hash of the two side by side.
ROUTE_FEATURES = (("dense", 0), ("mask", 1), ("rows", 2))
ROUTE_COLUMNS = ([f"wgrad_route_fmt{f}_{k}" for f in (0, 1, 2) for k, _ in ROUTE_FEATURES] +
                 [f"wgrad_route_fmt0_split3_{k}" for k, _ in ROUTE_FEATURES])


def _desc(B, grid, cin_stored, cout, kernel, stride, pad):
    """The sixteen TriConvDesc fields of a layer, output grid as ops.ConvGeom derives it."""
    out = [(i + 2 * p - k) // stride + 1 for i, k, p in zip(grid, kernel, pad)]
    return (B, *grid, cin_stored, *out, cout, *kernel, stride, *pad)


def descriptors():
    d = []
    for B in (1, 2, 5, 12, 24, 96, 192, 384, 768):                                             # 2D layers of the ResNet trunks
        for S in (4, 7, 8, 12, 14, 16, 28, 32, 56, 64, 112):
            for cin, cout in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (64, 256), (32, 64)):
                for k, s, p in ((3, 1, 1), (3, 2, 1), (1, 2, 0), (1, 1, 0)):
                    d.append(_desc(B, (1, S, S), cin, cout, (1, k, k), s, (0, p, p)))
    for B in (1, 2, 12, 24, 96, 192):                                                          # stems: 3 image channels stored as 4
        for k in (7, 5, 3):
            for H, W in ((32, 32), (64, 64), (128, 128), (224, 224), (48, 32)):
                d.append(_desc(B, (1, H, W), 4, 64, (1, k, k), 2, (0, k // 2, k // 2)))
    for B, H, W in ((5, 12, 32), (2, 10, 320)):                                                # odd shapes of tests/test_gpu_ops.py
        d.append(_desc(B, (1, H, W), 64, 64, (1, 3, 3), 1, (0, 1, 1)))
    for B in (1, 2, 3, 8, 32, 64, 128):                                                        # SubMConv3d levels of the voxel tower
        for D in (2, 4, 6, 8, 16, 32, 64, 128):
            for cin, cout in ((4, 32), (32, 64), (64, 128), (128, 256), (256, 512), (64, 64), (64, 32), (128, 64), (256, 128), (512, 256)):
                if B * D ** 3 * max(cin, cout) * 4 >= 8 << 30:                                 # an fp32 tensor of 8 GiB or more
                    continue
                d.append(_desc(B, (D, D, D), cin, cout, (3, 3, 3), 1, (1, 1, 1)))
    for M in (1, 2, 32, 64, 128, 512, 3072, 6144):                                             # linear layers as 1x1x1
        for K in (64, 256, 512, 768, 1024):
            for N in (128, 256, 384, 512, 768, 1536):
                d.append(_desc(M, (1, 1, 1), K, N, (1, 1, 1), 1, (0, 0, 0)))
    return np.asarray(d, dtype=np.int32)


def compute_table(desc):
    """int64 [N, len(COLUMNS)]: every plan query of the library, under the environment of this process."""
    import ctypes as C

    from tricolo_amd import _C
    lib = _C.lib()
    table = np.zeros((len(desc), len(COLUMNS)), dtype=np.int64)
    fam, tiles, steps = C.c_int(), C.c_int(), C.c_int()
    for i, row in enumerate(desc):
        d = C.byref(_C.make_desc(*(int(v) for v in row)))
        r = [lib.tri_conv_kernel_family(d, tr, m) for tr in (0, 1) for m in (0, 1, 2)]
        r += [lib.tri_conv_num_mtiles(d, m) for m in (0, 1, 2)]
        r += [lib.tri_conv_num_records(d, m, 1) for m in (0, 1, 2)]
        r += [lib.tri_conv_workspace(d, 0), lib.tri_conv_workspace(d, 1)]
        r += [lib.tri_conv_dgrad_bn_records(d, a, f) for a in (0, 1) for f in (0, 1, 2)]
        r += [lib.tri_conv_wgrad_workspace(d), lib.tri_conv_plan_bytes(d)]
        r += [lib.tri_conv_wgrad_kernel_family(d, 0), lib.tri_conv_wgrad_kernel_family(d, 1)]
        for f in (0, 1, 2):
            fam.value = tiles.value = steps.value = -1
            rc = lib.tri_conv_wgrad_group_info(d, f, C.byref(fam), C.byref(tiles), C.byref(steps))
            r += [rc, fam.value, tiles.value, steps.value]
        table[i] = r
    return table


def compute_routes(desc):
    """int64 [N, len(ROUTE_COLUMNS)]: tri_conv_wgrad_route's word (negative: the call is refused), under the environment of this process."""
    import ctypes as C

    from tricolo_amd import _C
    lib = _C.lib()
    table = np.zeros((len(desc), len(ROUTE_COLUMNS)), dtype=np.int64)
    for i, row in enumerate(desc):
        d = C.byref(_C.make_desc(*(int(v) for v in row)))
        table[i] = ([lib.tri_conv_wgrad_route(d, f, feat) for f in (0, 1, 2) for _, feat in ROUTE_FEATURES] +
                    [lib.tri_conv_wgrad_route(d, 0, feat | 4) for _, feat in ROUTE_FEATURES])
    return table


def table_sha256(table):
    return hashlib.sha256(np.ascontiguousarray(table, dtype=np.int64).tobytes()).hexdigest()


def switch_sha256(switch, all_columns=False):
    """SHA-256 of the table (or of table and route table side by side) in a fresh process with `switch` ("NAME=value") as its
    only TRICOLO_* variable."""
    return _switch_sha256s(switch)[1 if all_columns else 0]


@functools.lru_cache(maxsize=None)
def _switch_sha256s(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TRICOLO_")}
    name, value = switch.split("=", 1)
    env[name] = value
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--sha256"], env=env, check=True, capture_output=True, text=True)
    return tuple(out.stdout.split()[-2:])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sha256", action="store_true", help="print the table's SHA-256s (table; table and route table) under the current environment and exit")
    args = ap.parse_args()
    desc = descriptors()
    if args.sha256:
        table = compute_table(desc)
        print(table_sha256(table), table_sha256(np.hstack([table, compute_routes(desc)])))
        return
    if any(k.startswith("TRICOLO_") for k in os.environ):
        sys.exit("unset every TRICOLO_* variable before recording the default table")
    table = compute_table(desc)
    default = table_sha256(table)
    shas = [_switch_sha256s(s) for s in SWITCHES]
    same = [s for s, h in zip(SWITCHES, shas) if h[0] == default]
    if same:
        sys.exit(f"switches that do not change the table (drop them or extend the sweep): {same}")
    np.savez_compressed(OUT, desc=desc, columns=np.asarray(COLUMNS), table=table, switches=np.asarray(SWITCHES),
                        switch_sha256=np.asarray([h[0] for h in shas]), route_columns=np.asarray(ROUTE_COLUMNS),
                        route_table=compute_routes(desc), switch_sha256_all=np.asarray([h[1] for h in shas]))
    fams = sorted(set((table[:, :6] & 255).ravel().tolist()))
    print(f"{len(desc)} descriptors x {len(COLUMNS)} columns -> {OUT} ({os.path.getsize(OUT)} bytes); conv families {fams}")


if __name__ == "__main__":
    main()
