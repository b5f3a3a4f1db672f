"""PLY triangle meshes: vertices float32 x/y/z, triangles int32, binary
little-endian or ASCII. Deformation moves the vertices only; the faces pass
through untouched."""
from __future__ import annotations

import numpy as np


def write_ply(path, xyz, faces=None, *, binary: bool = True) -> None:
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    faces = np.zeros((0, 3), np.int32) if faces is None else np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= xyz.shape[0]):
        raise ValueError("face index outside the vertices")
    head = ("ply\nformat {} 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
            "element face {}\nproperty list uchar int vertex_indices\nend_header\n").format(
                "binary_little_endian" if binary else "ascii", xyz.shape[0], faces.shape[0])
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if binary:
            f.write(xyz.astype("<f4").tobytes())
            rec = np.zeros(faces.shape[0], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            rec["n"], rec["v"] = 3, faces
            f.write(rec.tobytes())
        else:
            for v in xyz:  # nine significant digits read back to the same float32
                f.write(("%.9g %.9g %.9g\n" % tuple(v)).encode("ascii"))
            for t in faces:
                f.write(("3 %d %d %d\n" % tuple(t)).encode("ascii"))


_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


def read_ply(path):
    """Returns (xyz float32 [V, 3], faces int32 [F, 3]). Reads the files
    write_ply writes and their kin: a vertex element with x, y, z among its
    scalar properties (others are skipped) and a face element with one list
    property of triangles."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    fmt, elements = None, []
    for ln in lines[1:]:
        tok = ln.split()
        if not tok or tok[0] == "comment":
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("property before element")
            elements[-1][2].append(tok[1:])
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"PLY format {fmt!r} is not read (ascii and binary_little_endian are)")
    xyz, faces = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    pos = 0
    text = body.decode("ascii").split("\n") if fmt == "ascii" else None
    for name, count, props in elements:
        is_list = [p[0] == "list" for p in props]
        if name == "vertex":
            if any(is_list):
                raise ValueError("list property on vertices")
            names = [p[1] for p in props]
            if fmt == "ascii":
                rows = np.array([text[pos + i].split() for i in range(count)], dtype=object).reshape(count, len(props))
                pos += count
                cols = {n: rows[:, j] for j, n in enumerate(names)}
                xyz = np.stack([np.array([np.float32(s) for s in cols[c]], np.float32) for c in "xyz"], 1) \
                    if count else xyz
            else:
                dt = np.dtype([(p[1], "<" + _TYPES[p[0]]) for p in props])
                rec = np.frombuffer(body, dt, count, pos)
                pos += count * dt.itemsize
                xyz = np.stack([rec[c].astype(np.float32) for c in "xyz"], 1)
        elif name == "face":
            if len(props) != 1 or not is_list[0]:
                raise ValueError("faces: one list property is read")
            ct, it = _TYPES[props[0][1]], _TYPES[props[0][2]]
            if fmt == "ascii":
                rows = [text[pos + i].split() for i in range(count)]
                pos += count
                if any(int(r[0]) != 3 for r in rows):
                    raise ValueError("only triangles are read")
                faces = np.array([[int(x) for x in r[1:4]] for r in rows], np.int32).reshape(count, 3)
            else:
                dt = np.dtype([("n", "<" + ct), ("v", "<" + it, (3,))])
                rec = np.frombuffer(body, dt, count, pos)
                pos += count * dt.itemsize
                if count and (rec["n"] != 3).any():
                    raise ValueError("only triangles are read")
                faces = rec["v"].astype(np.int32).reshape(count, 3)
        else:
            raise ValueError(f"PLY element {name!r} is not read")
    return np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), np.ascontiguousarray(faces)
