"""Minimal PLY reader / writer for the reference's point-cloud checkpoints (scene/gaussian_model.py:231-347).

The reference goes through the `plyfile` package (PlyData([PlyElement.describe(elements, 'vertex')]).write(path)): a
`binary_little_endian 1.0` file with ONE element `vertex` whose properties are all `float` (numpy 'f4'), in the order of
GaussianModel.construct_list_of_attributes (:231-248).  plyfile is not a dependency here; this module writes the same
bytes layout and reads binary-little-endian and ascii PLY files with scalar properties (list properties, as faces
have, are not needed and are rejected)."""
import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}
_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}


def write_vertices(path, elements):
    """elements: numpy structured array (one record per vertex)."""
    names = elements.dtype.names
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(elements)]
    for n in names:
        dt = elements.dtype[n]
        lines.append("property %s %s" % (_NAMES[dt.str[1:]], n))
    lines.append("end_header")
    le = elements.astype(elements.dtype.newbyteorder("<"), copy=False)
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
        f.write(le.tobytes())


def read_vertices(path):
    """Returns the `vertex` element as a numpy structured array."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elems, cur = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header is not terminated" % path)
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment" or tok[0] == "obj_info":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                cur = (tok[1], int(tok[2]), [])
                elems.append(cur)
            elif tok[0] == "property":
                if tok[1] == "list":
                    if cur[0] == "vertex":
                        raise ValueError("%s: list property on the vertex element" % path)
                    cur[2].append(None)
                else:
                    cur[2].append((tok[2], _TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if not elems or elems[0][0] != "vertex":
            raise ValueError("%s: the first element must be `vertex`" % path)
        name, count, props = elems[0]
        if fmt == "binary_little_endian":
            dt = np.dtype([(n, "<" + t) for n, t in props])
            data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        elif fmt == "binary_big_endian":
            dt = np.dtype([(n, ">" + t) for n, t in props])
            data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        elif fmt == "ascii":
            dt = np.dtype([(n, t) for n, t in props])
            rows = [f.readline().split() for _ in range(count)]
            data = np.array([tuple(float(v) for v in r) for r in rows], dtype=dt)
        else:
            raise ValueError("%s: unsupported PLY format %r" % (path, fmt))
    return data


def attribute_names(n_dc, n_rest, n_scale, n_rot, n_embedding, exclude_filter=False):
    """GaussianModel.construct_list_of_attributes (:231-248)."""
    l = ["x", "y", "z", "nx", "ny", "nz"]
    l += ["f_dc_%d" % i for i in range(n_dc)]
    l += ["f_rest_%d" % i for i in range(n_rest)]
    l.append("opacity")
    l += ["scale_%d" % i for i in range(n_scale)]
    l += ["rot_%d" % i for i in range(n_rot)]
    l += ["embedding_%d" % i for i in range(n_embedding)]
    l.append("tongue_class")
    if not exclude_filter:
        l.append("filter_3D")
    return l


def read_mesh(path):
    """(vertices [V,3] float32, faces [F,3] int64) of a binary little-endian triangle mesh whose vertex element holds
    float x, y, z and whose face element holds one `list uchar int` property (the layout mesh.write_mesh_ply writes)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elems = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header is not terminated" % path)
            tok = line.decode("ascii").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elems.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elems[-1][2].append(tuple(tok[1:]))
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian" or [e[0] for e in elems] != ["vertex", "face"]:
            raise ValueError("%s: expected a binary little-endian vertex + face mesh" % path)
        (_, nv, vp), (_, nf, fp) = elems
        if [p[-1] for p in vp] != ["x", "y", "z"] or any(p[0] not in ("float", "float32") for p in vp):
            raise ValueError("%s: vertex element must be float x, y, z" % path)
        if len(fp) != 1 or fp[0][:3] not in (("list", "uchar", "int"), ("list", "uint8", "int32")):
            raise ValueError("%s: face element must be one `list uchar int` property" % path)
        v = np.frombuffer(f.read(nv * 12), dtype="<f4", count=nv * 3).reshape(nv, 3).astype(np.float32)
        body = np.frombuffer(f.read(nf * 13), dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf)
        if nf and (body["n"] != 3).any():
            raise ValueError("%s: only triangles are supported" % path)
    return v, body["i"].astype(np.int64).reshape(nf, 3)
