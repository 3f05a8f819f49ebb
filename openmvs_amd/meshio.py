"""Triangle meshes in PLY files, as far as `Mesh::LoadPLY` / `Mesh::SavePLY` (libs/MVS/Mesh.cpp:1212-1303) use them: positions and faces.

`load_ply(path) -> (vertices (n, 3) float32, faces (m, 3) uint32)`, `save_ply(path, vertices, faces, binary=True)`.

Read: `format binary_little_endian 1.0` and `format ascii 1.0`; element `vertex` with float `x`, `y`, `z` (every other scalar vertex property -- normals, colours --
is skipped); element `face` with the list `vertex_indices` or `vertex_index`, a uchar count and int or uint indices, three per face (its other properties -- texture
coordinates, texture numbers -- are skipped); other elements are skipped, as `ply.get_other_element()` does.  Everything else raises ValueError naming what it met: the
reference's reader converts any scalar type to any other, this one takes what MeshLab, CloudCompare and the reference itself write."""
from __future__ import annotations

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
          "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_FACE_LISTS = ("vertex_indices", "vertex_index")


def _header(f, path):
    """-> (format, [(element, count, [(name, type) | (name, count type, item type)])])"""
    if f.readline().strip() != b"ply":
        raise ValueError("%s: not a PLY file" % path)
    fmt, elements = None, []
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError("%s: the header does not end" % path)
        w = raw.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "end_header":
            break
        if w[0] == "format" and len(w) == 3:
            fmt = w[1]
            if fmt not in ("binary_little_endian", "ascii") or w[2] != "1.0":
                raise ValueError("%s: format %s %s (binary_little_endian 1.0 and ascii 1.0 are read)" % (path, w[1], w[2]))
        elif w[0] == "element" and len(w) == 3:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) == 3:
            if w[1] not in _TYPES:
                raise ValueError("%s: property %s of unknown type %s" % (path, w[2], w[1]))
            elements[-1][2].append((w[2], _TYPES[w[1]]))
        elif w[0] == "property" and elements and len(w) == 5 and w[1] == "list":
            if w[2] not in _TYPES or w[3] not in _TYPES:
                raise ValueError("%s: list %s of unknown type %s %s" % (path, w[4], w[2], w[3]))
            elements[-1][2].append((w[4], _TYPES[w[2]], _TYPES[w[3]]))
        else:
            raise ValueError("%s: header line '%s'" % (path, " ".join(w)))
    if fmt is None:
        raise ValueError("%s: no format line" % path)
    return fmt, elements


def _check(path, name, props):
    """What this reader takes of the two elements it reads."""
    if name == "vertex":
        for p in props:
            if len(p) == 3:
                raise ValueError("%s: vertex property %s is a list" % (path, p[0]))
        have = dict(props)
        for c in "xyz":
            if c not in have:
                raise ValueError("%s: vertex has no property %s" % (path, c))
            if have[c] != "f4":
                raise ValueError("%s: vertex property %s is %s, not float" % (path, c, [k for k, v in _TYPES.items() if v == have[c]][0]))
    else:
        lists = [p for p in props if len(p) == 3 and p[0] in _FACE_LISTS]
        if len(lists) != 1:
            raise ValueError("%s: face has no list vertex_indices (or vertex_index); its properties are %s" % (path, ", ".join(p[0] for p in props) or "none"))
        _, ct, it = lists[0]
        if ct != "u1" or it not in ("i4", "u4"):
            raise ValueError("%s: face list %s has a %s count and %s indices (uchar and int or uint are read)" % (path, lists[0][0], ct, it))


def _read_binary(f, path, name, count, props):
    scalar = all(len(p) == 2 for p in props)
    if scalar:
        dt = np.dtype([(p[0], "<" + p[1]) for p in props])
        buf = f.read(dt.itemsize * count)
        if len(buf) != dt.itemsize * count:
            raise ValueError("%s: element %s ends after %d of %d bytes" % (path, name, len(buf), dt.itemsize * count))
        return np.frombuffer(buf, dt, count) if name == "vertex" else None
    if name == "face" and len(props) == 1:                       # the common case: records of 1 + 3 * 4 bytes, unless a face is no triangle
        dt = np.dtype([("n", "u1"), ("v", "<" + props[0][2], 3)])
        pos = f.tell()
        buf = f.read(dt.itemsize * count)
        if len(buf) == dt.itemsize * count:
            a = np.frombuffer(buf, dt, count)
            if (a["n"] == 3).all():
                return a["v"]
        f.seek(pos)
    rows = []
    for i in range(count):                                       # lists of any length, properties of any kind: one record at a time
        for p in props:
            if len(p) == 2:
                v = f.read(np.dtype(p[1]).itemsize)
                if len(v) != np.dtype(p[1]).itemsize:
                    raise ValueError("%s: element %s ends inside record %d" % (path, name, i))
                continue
            c = f.read(np.dtype(p[1]).itemsize)
            if len(c) != np.dtype(p[1]).itemsize:
                raise ValueError("%s: element %s ends inside record %d" % (path, name, i))
            n = int(np.frombuffer(c, "<" + p[1])[0])
            v = f.read(np.dtype(p[2]).itemsize * n)
            if len(v) != np.dtype(p[2]).itemsize * n:
                raise ValueError("%s: element %s ends inside record %d" % (path, name, i))
            if name == "face" and p[0] in _FACE_LISTS:
                if n != 3:
                    raise ValueError("%s: face %d has %d vertices (triangle meshes only)" % (path, i, n))
                rows.append(np.frombuffer(v, "<" + p[2]))
    return np.array(rows).reshape(-1, 3) if name == "face" else None


def _read_ascii(f, path, name, count, props):
    out = np.zeros((count, 3), np.float32 if name == "vertex" else np.int64)
    want = {c: k for k, c in enumerate("xyz")}
    for i in range(count):
        w = f.readline().split()
        if not w and count:
            raise ValueError("%s: element %s ends after %d of %d lines" % (path, name, i, count))
        at = 0
        try:
            for p in props:
                if len(p) == 2:
                    if name == "vertex" and p[0] in want:
                        out[i, want[p[0]]] = np.float32(float(w[at]))
                    at += 1
                    continue
                n = int(w[at]); at += 1
                if name == "face" and p[0] in _FACE_LISTS:
                    if n != 3:
                        raise ValueError("%s: face %d has %d vertices (triangle meshes only)" % (path, i, n))
                    if len(w) < at + 3:
                        raise IndexError
                    out[i] = [int(v) for v in w[at:at + 3]]
                at += n
            if at > len(w):
                raise IndexError
        except IndexError:
            raise ValueError("%s: %s %d has too few values" % (path, name, i)) from None
    return out if name in ("vertex", "face") else None


def load_ply(path):
    """-> (vertices (n, 3) float32, faces (m, 3) uint32).  ValueError for anything this reader does not take (see the module's text), naming it; a face index outside
    the vertices is one of them."""
    with open(path, "rb") as f:
        fmt, elements = _header(f, path)
        names = [e[0] for e in elements]
        for need in ("vertex", "face"):
            if names.count(need) != 1:
                raise ValueError("%s: %d elements named %s" % (path, names.count(need), need))
        for name, count, props in elements:                      # the header is judged before any record is read
            if name in ("vertex", "face"):
                _check(path, name, props)
        V = F = None
        for name, count, props in elements:
            got = (_read_binary if fmt == "binary_little_endian" else _read_ascii)(f, path, name, count, props)
            if name == "vertex":
                V = np.stack([got[c] for c in "xyz"], 1).astype(np.float32) if fmt != "ascii" else got
            elif name == "face":
                F = np.asarray(got).reshape(-1, 3)
    if len(F) and (int(F.min()) < 0 or int(F.max()) >= len(V)):
        raise ValueError("%s: a face names vertex %d of %d" % (path, int(F.max()) if int(F.max()) >= len(V) else int(F.min()), len(V)))
    return np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(F, np.uint32).reshape(-1, 3)


def save_ply(path, vertices, faces, binary=True):
    """The mesh as `Mesh::SavePLY` writes an untextured one without normals: float x y z, `property list uchar int vertex_indices`."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces).reshape(-1, 3)
    if len(F) and (int(F.min()) < 0 or int(F.max()) >= len(V)):
        raise ValueError("a face names a vertex the mesh does not have")
    head = "ply\nformat %s 1.0\ncomment generated by openmvs_amd\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" \
           "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % ("binary_little_endian" if binary else "ascii", len(V), len(F))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if binary:
            f.write(V.astype("<f4").tobytes())
            rec = np.zeros(len(F), np.dtype([("n", "u1"), ("v", "<i4", 3)]))
            rec["n"] = 3; rec["v"] = F
            f.write(rec.tobytes())
        else:
            for v in V:
                f.write(("%s %s %s\n" % tuple(repr(float(c)) for c in v)).encode("ascii"))       # repr of the double of a float: reads back to the same float
            for t in F:
                f.write(("3 %d %d %d\n" % tuple(int(i) for i in t)).encode("ascii"))
