"""Mesh export of the validation loop (runner.py:231-240): the reference builds a `trimesh.Trimesh(vertices, triangles)`,
applies the scene's `scale_mat` (normalised unit-sphere frame -> world frame, datasets/dtu.py:204-240) and exports a PLY.
trimesh is not a dependency here: `transform_vertices` is `Trimesh.apply_transform` for a point set and `write_ply` writes
the same binary little-endian PLY layout trimesh 3.22 exports (float32 x y z, faces as `list uchar int vertex_indices`).
Optional per-vertex attributes (ImplicitSurface.vertex_attributes): float32 normals `nx ny nz`, uint8 colours `red green blue`."""
import os

import numpy as np


def transform_vertices(vertices, matrix):
    """(V,3) points through a 4x4 homogeneous matrix: trimesh.Trimesh.apply_transform (runner.py:236)."""
    v = np.asarray(vertices, dtype=np.float64)
    m = np.asarray(matrix, dtype=np.float64).reshape(4, 4)
    out = v @ m[:3, :3].T + m[:3, 3][None, :]
    w = v @ m[3, :3] + m[3, 3]
    if not np.allclose(w, 1.0):
        out = out / w[:, None]
    return out


def transform_normals(normals, matrix, rtol=1e-4):
    """(V,3) unit normals through the linear part of a 4x4 similarity transform (rotation times uniform scale, what scale_mat is
    for the DTU and the Tanks readers), re-normalised; zero rows stay zero.  A similarity has A A^T = s^2 I: checked to `rtol`
    relative to s^2, ValueError otherwise (normals would need the inverse transpose, and the mesh would be sheared)."""
    m = np.asarray(matrix, dtype=np.float64).reshape(4, 4)
    a = m[:3, :3]
    gram = a @ a.T
    s2 = np.trace(gram) / 3.0
    if not (np.isfinite(gram).all() and s2 > 0 and np.abs(gram - s2 * np.eye(3)).max() <= rtol * s2
            and np.abs(m[3, :3]).max() <= rtol * abs(m[3, 3])):
        raise ValueError("transform_normals: the matrix is not a rotation times a uniform scale")
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3) @ a.T
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0).astype(np.float32)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: `element vertex N` (float x, y, z [, float nx, ny, nz] [, uchar red, green, blue]) +
    `element face M` (list uchar int vertex_indices).  normals: (N,3) float32, colors: (N,3) uint8, both optional; without them
    the file is the bare-geometry file, byte for byte."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f4").reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(triangles, dtype="<i4").reshape(-1, 3))
    if t.size and (t.min() < 0 or t.max() >= max(len(v), 1)):
        raise ValueError("triangle index out of range")
    fields, props = [("xyz", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        normals = np.asarray(normals, dtype="<f4")
        if normals.shape != v.shape:
            raise ValueError("normals: expected one (x, y, z) row per vertex")
        fields.append(("n", "<f4", (3,)))
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8 or colors.shape != v.shape:
            raise ValueError("colors: expected one uint8 (red, green, blue) row per vertex")
        fields.append(("rgb", "u1", (3,)))
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = ("ply\nformat binary_little_endian 1.0\ncomment surf_amd mesh export\n"
              f"element vertex {len(v)}\n{props}"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    if len(fields) > 1:
        rows = np.empty(len(v), dtype=fields)               # packed: 12 [+ 12] [+ 3] bytes per vertex
        rows["xyz"] = v
        if normals is not None:
            rows["n"] = normals
        if colors is not None:
            rows["rgb"] = colors
        v = rows
    faces = np.empty(len(t), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    faces["n"] = 3
    faces["idx"] = t
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def write_ply_points(path, points, colors=None, normals=None):
    """A point cloud (fusion.fuse_points) as write_ply's file with `element face 0`: points (N,3), colors (N,3) uint8 or None,
    normals (N,3) float32 or None (point_filter.estimate_normals: nx ny nz, what a viewer shades by and a Poisson reconstructor
    needs).  datasets.mvs_io.read_ply_points and read_ply read it back."""
    write_ply(path, points, np.zeros((0, 3), dtype=np.int32), normals=normals, colors=colors)


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1",
              "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4",
              "uint": "<u4", "uint32": "<u4"}


def read_ply(path, attributes=False):
    """Reads back what write_ply (or trimesh's binary PLY export of a plain triangle mesh) wrote: (vertices, triangles).
    attributes=True: (vertices, triangles, {"normals": (N,3) float32, "colors": (N,3) uint8}) with the properties the file has
    (nx ny nz / red green blue); vertex properties beyond those are skipped."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in head:
        raise ValueError("only binary little-endian PLY is supported")
    nv = nt = 0
    element, vprops = None, []
    for l in head:
        w = l.split()
        if l.startswith("element"):
            element = w[1]
        if l.startswith("element vertex"):
            nv = int(w[-1])
        if l.startswith("element face"):
            nt = int(w[-1])
        if l.startswith("property") and element == "vertex":
            if w[1] == "list" or w[1] not in _PLY_TYPES:
                raise ValueError(f"unsupported vertex property: {l}")
            vprops.append((w[2], _PLY_TYPES[w[1]]))
    vdt = np.dtype(vprops)
    if [n for n, _ in vprops[:3]] != ["x", "y", "z"] or any(vdt[n] != np.dtype("<f4") for n in ("x", "y", "z")):
        raise ValueError("expected float x, y, z as the first vertex properties")
    rows = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    v = np.stack([rows["x"], rows["y"], rows["z"]], axis=1).reshape(nv, 3)
    faces = np.frombuffer(data, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nt, offset=end + nv * vdt.itemsize)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("not a triangle mesh")
    if not attributes:
        return v.copy(), faces["idx"].copy()
    attrs = {}
    names = set(vdt.names)
    if {"nx", "ny", "nz"} <= names:
        attrs["normals"] = np.stack([rows["nx"], rows["ny"], rows["nz"]], axis=1).reshape(nv, 3).astype(np.float32)
    if {"red", "green", "blue"} <= names:
        attrs["colors"] = np.stack([rows["red"], rows["green"], rows["blue"]], axis=1).reshape(nv, 3).astype(np.uint8)
    return v.copy(), faces["idx"].copy(), attrs


def read_ply_mesh(path):
    """(vertices (V,3) float64, faces (F,3) int64) of an ascii or binary little-endian PLY triangle mesh, as this project writes
    them (write_ply; mvs_io.read_ply_points reads the points only): scalar vertex properties of which x, y, z are taken, then one
    face element with a single list property of three indices per face.  What trimesh.load returns for such a file, minus its
    merging of duplicate vertices."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header") + len(b"end_header")
    end = data.index(b"\n", end) + 1
    fmt, element, nv, nt, vprops, fprop = None, None, 0, 0, [], None
    for l in data[:end].decode("ascii", "ignore").splitlines():
        w = l.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            elif element == "face":
                nt = int(w[2])
            elif int(w[2]):
                raise ValueError(f"unsupported PLY element: {l}")
        elif w[0] == "property" and element == "vertex":
            if w[1] == "list" or w[1] not in _PLY_TYPES:
                raise ValueError(f"unsupported vertex property: {l}")
            vprops.append((w[2], _PLY_TYPES[w[1]]))
        elif w[0] == "property" and element == "face":
            if fprop is not None or w[1] != "list" or w[2] not in _PLY_TYPES or w[3] not in _PLY_TYPES:
                raise ValueError(f"unsupported face property: {l}")
            fprop = (_PLY_TYPES[w[2]], _PLY_TYPES[w[3]])
    names = [n for n, _ in vprops]
    if not all(a in names for a in "xyz") or (nt and fprop is None):
        raise ValueError("expected x, y, z vertex properties and a face list property")
    if fmt == "ascii":
        lines = data[end:].decode("ascii").split("\n")
        rows = np.array([l.split() for l in lines[:nv]], dtype=np.float64).reshape(nv, len(names))
        v = np.stack([rows[:, names.index(a)] for a in "xyz"], axis=1).reshape(nv, 3)
        faces = np.array([l.split() for l in lines[nv:nv + nt]], dtype=np.int64).reshape(nt, -1)
        if nt and (faces.shape[1] != 4 or not (faces[:, 0] == 3).all()):
            raise ValueError("not a triangle mesh")
        return v, faces[:, 1:].copy() if nt else np.zeros((0, 3), dtype=np.int64)
    if fmt != "binary_little_endian":
        raise ValueError("only ascii and binary little-endian PLY are supported")
    vdt = np.dtype(vprops)
    rows = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    v = np.stack([rows[a].astype(np.float64) for a in "xyz"], axis=1).reshape(nv, 3)
    if not nt:
        return v, np.zeros((0, 3), dtype=np.int64)
    faces = np.frombuffer(data, dtype=[("n", fprop[0]), ("idx", fprop[1], (3,))], count=nt, offset=end + nv * vdt.itemsize)
    if not (faces["n"] == 3).all():
        raise ValueError("not a triangle mesh")
    return v, faces["idx"].astype(np.int64)


def write_obj(path, vertices, faces, uv, atlas, normals=None):
    """A textured mesh (mesh_texture.bake_texture) as Wavefront OBJ: <name>.obj (`mtllib`, `v` with 9 significant digits, `vt` one
    per face corner, optional `vn`, `f a/ta b/tb c/tc` or `a/ta/na ...`, indices from 1), <name>.mtl (one material with `map_Kd`)
    and <name>.png (the atlas, row 0 at the top: v = 1) side by side.  uv (3m, 2) fp32, atlas (Ha, Wa, 3) uint8, normals (n, 3)
    fp32 per vertex or None.  Returns the three paths."""
    from PIL import Image
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    atlas = np.asarray(atlas)
    if f.size and (f.min() < 0 or f.max() >= max(len(v), 1)):
        raise ValueError("triangle index out of range")
    if len(uv) != 3 * len(f):
        raise ValueError(f"uv: expected one (u, v) row per face corner, {3 * len(f)} rows, got {len(uv)}")
    if atlas.dtype != np.uint8 or atlas.ndim != 3 or atlas.shape[2] != 3 or atlas.size == 0:
        raise ValueError("atlas: expected a uint8 (Ha, Wa, 3) image")
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32)
        if normals.shape != v.shape:
            raise ValueError("normals: expected one (x, y, z) row per vertex")
    stem = os.path.splitext(os.path.abspath(path))[0]
    name = os.path.basename(stem)
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    Image.fromarray(atlas).save(stem + ".png")
    with open(stem + ".mtl", "w") as out:
        out.write(f"# surf_amd mesh export\nnewmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    corner = np.arange(1, 3 * len(f) + 1, dtype=np.int64).reshape(-1, 3)
    with open(stem + ".obj", "w") as out:
        out.write(f"# surf_amd mesh export\nmtllib {name}.mtl\nusemtl {name}\n")
        out.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v.tolist()))
        out.write("".join(f"vt {a:.9g} {b:.9g}\n" for a, b in uv.tolist()))
        if normals is None:
            out.write("".join(f"f {a}/{ta} {b}/{tb} {c}/{tc}\n" for (a, b, c), (ta, tb, tc) in zip((f + 1).tolist(), corner.tolist())))
        else:
            out.write("".join(f"vn {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in normals.tolist()))
            out.write("".join(f"f {a}/{ta}/{a} {b}/{tb}/{b} {c}/{tc}/{c}\n"
                              for (a, b, c), (ta, tb, tc) in zip((f + 1).tolist(), corner.tolist())))
    return stem + ".obj", stem + ".mtl", stem + ".png"


def read_obj(path):
    """Reads back what write_obj wrote: {"vertices" (n, 3) fp32, "faces" (m, 3) int32, "uv" (3m, 2) fp32 in face-corner order,
    "normals" (n, 3) fp32 or None, "atlas" (Ha, Wa, 3) uint8 or None (the `map_Kd` image of the `mtllib`, found beside the file)}.
    9 significant digits return every fp32 to the bit."""
    v, vt, vn, fv, ft, mtl = [], [], [], [], [], None
    with open(path) as src:
        for line in src:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "v":
                v.append(w[1:4])
            elif w[0] == "vt":
                vt.append(w[1:3])
            elif w[0] == "vn":
                vn.append(w[1:4])
            elif w[0] == "mtllib":
                mtl = w[1]
            elif w[0] == "f":
                if len(w) != 4:
                    raise ValueError("not a triangle mesh")
                parts = [c.split("/") for c in w[1:]]
                fv.append([int(p[0]) - 1 for p in parts])
                ft.append([int(p[1]) - 1 for p in parts])
    vt = np.array(vt, dtype=np.float64).reshape(-1, 2).astype(np.float32)
    atlas = None
    if mtl is not None:
        here = os.path.dirname(os.path.abspath(path))
        with open(os.path.join(here, mtl)) as src:
            maps = [l.split()[1] for l in src if l.split()[:1] == ["map_Kd"]]
        if maps:
            from PIL import Image
            atlas = np.asarray(Image.open(os.path.join(here, maps[0])).convert("RGB"))
    return {"vertices": np.array(v, dtype=np.float64).reshape(-1, 3).astype(np.float32),
            "faces": np.array(fv, dtype=np.int32).reshape(-1, 3), "uv": vt[np.array(ft, dtype=np.int64).reshape(-1)],
            "normals": np.array(vn, dtype=np.float64).reshape(-1, 3).astype(np.float32) if vn else None, "atlas": atlas}


def export_mesh(path, vertices, triangles, scale_mat=None, normals=None, colors=None):
    """runner.py:231-240: optional scale_mat transform, then PLY export.  Returns the transformed vertices.  normals / colors
    (per vertex, optional): written as nx ny nz / red green blue; normals go through scale_mat's linear part (transform_normals:
    scale_mat must then be a rotation times a uniform scale, ValueError otherwise)."""
    v = np.asarray(vertices, dtype=np.float64)
    if scale_mat is not None:
        scale_mat = scale_mat.detach().cpu().numpy() if hasattr(scale_mat, "detach") else scale_mat
        v = transform_vertices(v, scale_mat)
        if normals is not None:
            normals = transform_normals(normals, scale_mat)
    write_ply(path, v, triangles, normals=normals, colors=colors)
    return v
