"""Point-cloud PLY files as the reference writes them: `PointCloud::Save`, `SaveNViews` and `SaveWithScale` (libs/MVS/PointCloud.cpp:361-539) and the per-view clouds of
`MVS::ExportPointCloud` (libs/MVS/DepthMap.cpp:1753-1870).  Binary little endian, the header text of `PLY::header_complete` (libs/IO/PLY.cpp:315-367) with the
non-legacy type names (float32, uint8, uint32; PLY.cpp:29-31).  ASCII files are not written.  `load_point_cloud` reads back what these writers write."""
from __future__ import annotations

import os

import numpy as np

from . import mapexport

_TYPES = {"float32": "<f4", "uint8": "u1", "uint32": "<u4"}


def _header(n, props):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n]
    lines += [("property list %s %s %s" % p[1:]) if p[0] == "list" else ("property %s %s" % p) for p in props]
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


def save_point_cloud(path, cloud, views: bool = True, min_views: int = 0, scales=None) -> bool:
    """`cloud`: the dict of `PatchMatchHIP.scene_fuse` / `scene_cloud_get` (points, viewStart / views / weights as CSR, colors B, G, R or None, normals or None; `weights`
    None or absent: a cloud without weights).  Properties and their order are those of `InitSaveProps` (PointCloud.cpp:265-304):
      scales None, min_views 0   PointCloud::Save(fileName, bViews = views): x y z [red green blue] [nx ny nz] [view_indices] [view_weights], the lists `list uint8`;
      min_views > 0              PointCloud::SaveNViews: the points with at least that many views, x y z red green blue [nx ny nz], white without colours;
      scales = (scale, conf)     PointCloud::SaveWithScale: x y z [red green blue] [nx ny nz] confidence value (`mapexport.point_scales` / `scene_cloud_scale`).
    A cloud with no points -- or none with `min_views` views -- writes no file and returns False, as the reference does."""
    pts = np.asarray(cloud["points"], np.float32).reshape(-1, 3)
    n = len(pts)
    if n == 0:
        return False
    vs = np.asarray(cloud["viewStart"], np.int64)
    cnt = vs[1:] - vs[:-1]
    col = cloud.get("colors"); nrm = cloud.get("normals"); wts = cloud.get("weights")
    keep = np.ones(n, bool)
    if scales is None and min_views > 0:
        keep = cnt >= int(min_views)
        if not keep.any():
            return False
        col = np.full((n, 3), 255, np.uint8) if col is None else col
    props = [("float32", "x"), ("float32", "y"), ("float32", "z")]
    fields = [("p", "<f4", 3)]
    if col is not None:
        props += [("uint8", "red"), ("uint8", "green"), ("uint8", "blue")]; fields.append(("c", "u1", 3))
    if nrm is not None:
        props += [("float32", "nx"), ("float32", "ny"), ("float32", "nz")]; fields.append(("n", "<f4", 3))
    fixed = np.zeros(n, np.dtype(fields + ([("conf", "<f4"), ("scale", "<f4")] if scales is not None else [])))
    fixed["p"] = pts
    if col is not None:
        fixed["c"] = np.asarray(col, np.uint8).reshape(n, 3)[:, ::-1]                # Pixel8U is B, G, R in memory; the file has red first
    if nrm is not None:
        fixed["n"] = np.asarray(nrm, np.float32).reshape(n, 3)
    lists = scales is None and min_views <= 0 and views
    if scales is not None:
        props += [("float32", "confidence"), ("float32", "value")]
        fixed["scale"] = np.asarray(scales[0], np.float32); fixed["conf"] = np.asarray(scales[1], np.float32)
    if lists:
        if (cnt > 255).any():
            raise ValueError("save_point_cloud: a point with more than 255 views (the lists are counted in a uint8)")
        props.append(("list", "uint8", "uint32", "view_indices"))
        if wts is not None:
            props.append(("list", "uint8", "float32", "view_weights"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(_header(int(keep.sum()), props))
        if not lists:
            f.write(fixed[keep].tobytes())
            return True
        # a record of its own length per point: fixed part, then count + indices, then count + weights
        nv = int(vs[-1])
        fb = fixed.dtype.itemsize
        per = fb + (1 + 4 * cnt) * (2 if wts is not None else 1)
        start = np.concatenate([[0], np.cumsum(per)])
        buf = np.zeros(int(start[-1]), np.uint8)
        buf[(start[:-1, None] + np.arange(fb)[None, :]).ravel()] = fixed.view(np.uint8).reshape(n, fb).ravel()
        owner = np.repeat(np.arange(n), cnt); rank = np.arange(nv) - vs[owner]
        buf[start[:-1] + fb] = cnt.astype(np.uint8)
        at = start[owner] + fb + 1 + 4 * rank
        buf[(at[:, None] + np.arange(4)[None, :]).ravel()] = np.ascontiguousarray(cloud["views"], "<u4").view(np.uint8)
        if wts is not None:
            w0 = start[:-1] + fb + 1 + 4 * cnt
            buf[w0] = cnt.astype(np.uint8)
            at = w0[owner] + 1 + 4 * rank
            buf[(at[:, None] + np.arange(4)[None, :]).ravel()] = np.ascontiguousarray(wts, "<f4").view(np.uint8)
        f.write(buf.tobytes())
    return True


def save_view_cloud(path, records, with_normals: bool) -> bool:
    """The file `MVS::ExportPointCloud` writes from the records of `PatchMatchHIP.scene_view_cloud` / `mapexport.view_point_cloud`: the property tables of
    DepthMap.cpp:1764-1771 (x y z red green blue) and :1818-1828 (x y z nx ny nz red green blue).  No record: no file, False."""
    dt = mapexport.VIEW_VERTEX_N if with_normals else mapexport.VIEW_VERTEX
    rec = np.ascontiguousarray(records)
    rec = rec.view(np.uint8).reshape(-1, dt.itemsize) if rec.dtype != dt else rec
    if len(rec) == 0:
        return False
    props = [("float32", k) for k in "xyz"] + ([("float32", k) for k in ("nx", "ny", "nz")] if with_normals else []) + [("uint8", k) for k in ("red", "green", "blue")]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(_header(len(rec), props))
        f.write(rec.tobytes())
    return True


def load_point_cloud(path) -> dict:
    """A binary little-endian PLY of one `vertex` element, scalar and `list uint8` properties -> {name: array}; a list property gives (counts, flat values)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0" or not lines[2].startswith("element vertex "):
        raise ValueError("%s: not a binary little-endian PLY of vertices" % path)
    n = int(lines[2].split()[2])
    props = [ln.split()[1:] for ln in lines[3:] if ln.startswith("property ")]
    body = np.frombuffer(data, np.uint8, offset=end)
    if not any(p[0] == "list" for p in props):
        rec = body.view(np.dtype([(p[1], _TYPES[p[0]]) for p in props]))
        assert len(rec) == n
        return {p[1]: rec[p[1]].copy() for p in props}
    out = {p[-1]: [] for p in props}
    at = 0
    for _ in range(n):
        for p in props:
            if p[0] != "list":
                dt = np.dtype(_TYPES[p[0]])
                out[p[1]].append(body[at:at + dt.itemsize].view(dt)[0]); at += dt.itemsize
            else:
                c = int(body[at]); dt = np.dtype(_TYPES[p[2]])
                out[p[3]].append((c, body[at + 1:at + 1 + c * dt.itemsize].view(dt).copy())); at += 1 + c * dt.itemsize
    assert at == len(body)
    res = {}
    for p in props:
        if p[0] != "list":
            res[p[1]] = np.asarray(out[p[1]], _TYPES[p[0]])
        else:
            res[p[3]] = (np.asarray([c for c, _ in out[p[3]]], np.uint8), np.concatenate([v for _, v in out[p[3]]]) if n else np.zeros(0, _TYPES[p[2]]))
    return res
