"""A reader for the NRRD voxel grids of Text2Shape (nrrd_256_filter_div_{32,64,128}_solid/<id>/<id>.nrrd), in place of pynrrd's
nrrd.read(path)[0] in the reference's data/preprocess_all_data.py:93-96.

Supported is what those files need: magic NRRD000x, type uint8 / unsigned char / uchar, dimension 4, sizes `4 V V V`, encoding raw
or gzip / gz, data in the same file.  pynrrd returns the array with the header's sizes as its shape in Fortran order,
np.frombuffer(...).reshape(sizes, order="F") - the first header axis runs fastest - and so does this reader.  That is restated from
pynrrd's documentation: pynrrd is not installed where this was written, so no array has been compared with its output.  Anything else
raises ValueError naming the file and the field."""
from __future__ import annotations

import zlib

import numpy as np

_UINT8 = ("uint8", "unsigned char", "uchar", "uint8_t")


def read_nrrd(path, voxel_size=None):
    """-> uint8 [4, V, V, V], indexed [channel, x, y, z] as pynrrd's array is.  voxel_size: the V the caller expects (optional)."""
    with open(path, "rb") as f:
        raw = f.read()
    first, _, rest = raw.partition(b"\n")
    magic = first.rstrip(b"\r")
    if len(magic) != 8 or not magic.startswith(b"NRRD000") or not magic[7:8].isdigit():
        raise ValueError(f"{path}: magic: not an NRRD file (the first line is {magic[:20]!r})")
    fields, pos, ended = {}, len(first) + 1, False
    while pos < len(raw):
        end = raw.find(b"\n", pos)
        if end < 0:
            break
        line = raw[pos:end].rstrip(b"\r")
        pos = end + 1
        if not line:                                                                # the blank line: data follows
            ended = True
            break
        if line.startswith(b"#") or b":=" in line:
            continue
        key, sep, value = line.partition(b":")
        if sep:
            fields[key.strip().lower().decode(errors="replace")] = value.strip().decode(errors="replace")
    if not ended:
        raise ValueError(f"{path}: header: no blank line ends it")
    for key in ("type", "dimension", "sizes", "encoding"):
        if key not in fields:
            raise ValueError(f"{path}: {key}: the header has no such field")
    if "data file" in fields or "datafile" in fields:
        raise ValueError(f"{path}: data file: a detached data file is not supported")
    if fields["type"].lower() not in _UINT8:
        raise ValueError(f"{path}: type: {fields['type']!r} is not uint8")
    if fields["dimension"] != "4":
        raise ValueError(f"{path}: dimension: {fields['dimension']!r}, expected 4")
    try:
        sizes = [int(t) for t in fields["sizes"].split()]
    except ValueError:
        sizes = []
    if len(sizes) != 4 or sizes[0] != 4 or sizes[1] < 1 or len(set(sizes[1:])) != 1 or (voxel_size is not None and sizes[1] != int(voxel_size)):
        want = "4 V V V" if voxel_size is None else f"4 {voxel_size} {voxel_size} {voxel_size}"
        raise ValueError(f"{path}: sizes: {fields['sizes']!r}, expected {want}")
    enc = fields["encoding"].lower()
    body = raw[pos:]
    if enc in ("gzip", "gz"):
        try:
            body = zlib.decompress(body, 47)                                        # gzip or zlib wrapper
        except zlib.error as e:
            raise ValueError(f"{path}: encoding: the gzip stream does not decompress ({e})") from None
    elif enc != "raw":
        raise ValueError(f"{path}: encoding: {fields['encoding']!r} is not raw or gzip")
    count = int(np.prod(sizes))
    if len(body) < count:
        raise ValueError(f"{path}: sizes: {fields['sizes']!r} needs {count} bytes of data, the file holds {len(body)}")
    return np.ascontiguousarray(np.frombuffer(body, dtype=np.uint8, count=count).reshape(sizes, order="F"))
