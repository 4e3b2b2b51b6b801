"""Truncated signed distance volumes on the device (`roma_op_tsdf_integrate`, `roma_op_tsdf_extract_mesh`, `roma_op_points_bounds`,
csrc/tsdf.hip): depth maps - `DenseFusion.depth` as it is, or a sensor's - are integrated into a volume that the caller owns, and
the zero level set of the volume comes out as a coloured, oriented triangle mesh.  Integration is additive: a volume that a second
call keeps adding to has no limit on the number of views, and the depth maps of a second reconstruction, once `apply_similarity`
has moved its cameras, integrate into the first.  The steps are spelled out in include/roma_hip_tsdf.h and restated in numpy by
tools/tsdf_ref.py; every result is bit-identical from run to run and independent of the batch.  Device tensors only, nothing read
back - `write_ply` is the one host read of the module."""
from __future__ import annotations

from functools import partial
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _valid

MAX_VIEWS = 8           # csrc/tsdf.hip: TSDF_MAX_VIEWS, the views of one integrate call
MAX_COLOR_VIEWS = 128   # TSDF_MAX_COLOR_VIEWS: B * V with a colour source


class TSDFVolume(NamedTuple):
    tsdf: torch.Tensor             # [.., nz, ny, nx] float32 in units of trunc, in [-1, 1]; 1 where nothing was seen
    weight: torch.Tensor           # [.., nz, ny, nx] float32, 0 where nothing was seen
    color: Optional[torch.Tensor]  # [.., nz, ny, nx, 3] float32 in 0 .. 255 (None: a volume without colour)
    origin: torch.Tensor           # [.., 3] float64: the corner of voxel (0, 0, 0); its centre is origin + 0.5 voxel_size
    voxel_size: torch.Tensor       # [..] float64
    trunc: torch.Tensor            # [..] float64: the truncation distance in world units


class Mesh(NamedTuple):
    vertices: torch.Tensor         # [.., max_vertices, 3] float32 world coordinates in (grid point, edge class) order, NaN padding
    normals: torch.Tensor          # [.., max_vertices, 3] float32 unit normals towards the outside, NaN where the gradient is not known
    colors: Optional[torch.Tensor]  # [.., max_vertices, 3] uint8 (None without a colour volume), 0 padding
    faces: torch.Tensor            # [.., max_faces, 3] int32 in (cell, tetrahedron, triangle) order, -1 padding
    counts: torch.Tensor           # [.., 2] int32: vertices and faces written
    totals: torch.Tensor           # [.., 2] int32: vertices and faces there are
    stats: torch.Tensor            # [.., 8] int32: valid voxels, inside ones, vertices, faces, rim vertices, cut faces, cells with a face, 0


_device_tensor = partial(_lib._device_tensor, module="tsdf")


def _dims(dims):
    if not isinstance(dims, (tuple, list)) or len(dims) != 3 or any(int(d) != d or int(d) < 1 for d in dims):
        raise ValueError("roma_amd.tsdf: dims must be three positive integers (nz, ny, nx)")
    nz, ny, nx = (int(d) for d in dims)
    if 7 * nz * ny * nx >= 2 ** 31:
        raise ValueError("roma_amd.tsdf: 7 nz ny nx must be below 2^31")
    return nz, ny, nx


def _per_problem(x, name, B, tail, dev):
    """a float64 contiguous device tensor [B, *tail] of x, which must be on the device already (it may come from a kernel)"""
    x = _device_tensor(x, name).to(device=dev, dtype=torch.float64)
    if x.numel() != B * int(np.prod(tail, dtype=np.int64)):
        raise ValueError(f"roma_amd.tsdf: {name} must hold {[B] + list(tail)} values, got {tuple(x.shape)}")
    return x.reshape([B] + list(tail)).contiguous()


def tsdf_volume(dims, origin, voxel_size, trunc, *, color=False):
    """A fresh volume: tsdf 1, weight 0, color 0.  dims = (nz, ny, nx); origin [3] or [B, 3], voxel_size and trunc scalars or [B]:
    float64 tensors ON THE DEVICE (`tsdf_bounds` makes the first two without a host read).  [B, 3] gives a batch of B volumes."""
    nz, ny, nx = _dims(dims)
    origin = _device_tensor(origin, "origin")
    if origin.dim() not in (1, 2) or origin.shape[-1] != 3:
        raise ValueError("roma_amd.tsdf: origin must be [3] or [B, 3]")
    single = origin.dim() == 1
    B, dev = (1 if single else int(origin.shape[0])), origin.device
    if B * nz * ny * nx >= 2 ** 31:
        raise ValueError("roma_amd.tsdf: B nz ny nx must be below 2^31")
    origin = _per_problem(origin, "origin", B, [3], dev)
    voxel_size, trunc = _per_problem(voxel_size, "voxel_size", B, [], dev), _per_problem(trunc, "trunc", B, [], dev)
    tsdf = torch.ones((B, nz, ny, nx), device=dev, dtype=torch.float32)
    weight = torch.zeros((B, nz, ny, nx), device=dev, dtype=torch.float32)
    col = torch.zeros((B, nz, ny, nx, 3), device=dev, dtype=torch.float32) if color else None
    out = TSDFVolume(tsdf, weight, col, origin, voxel_size, trunc)
    return TSDFVolume(*(None if o is None else o[0] for o in out)) if single else out


def volume_from_bounds(bounds, dims, margin=0.05):
    """(origin [.., 3], voxel_size [..]) float64 of a volume of dims = (nz, ny, nx) with cubic voxels around the boxes bounds
    [.., 2, 3]: the box grown by `margin` times its largest extent on every side, the voxel the largest of the three quotients, the
    box centred.  Plain tensor arithmetic on whatever device bounds live on."""
    nz, ny, nx = _dims(dims)
    bounds = bounds.to(torch.float64)
    lo, hi = bounds[..., 0, :], bounds[..., 1, :]
    n = torch.tensor([nx, ny, nz], dtype=torch.float64, device=bounds.device)
    ext = hi - lo
    pad = float(margin) * ext.max(dim=-1, keepdim=True).values
    vs = ((ext + 2.0 * pad) / n).max(dim=-1).values
    return (lo + hi) * 0.5 - 0.5 * n * vs[..., None], vs


def points_bounds(points, counts=None):
    """The box of the finite rows of points [B, N, 3] float32 below counts [B] (`roma_op_points_bounds`): [B, 2, 3] float64 = (min,
    max), NaN for a problem without a finite row; [N, 3] gives [2, 3].  One kernel, order-independent, no host read."""
    points = _device_tensor(points, "points")
    if points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError("roma_amd.tsdf: points must be [N, 3] or [B, N, 3]")
    single = points.dim() == 2
    B, N, dev = (1 if single else int(points.shape[0])), int(points.shape[-2]), points.device
    if B > 65535 or 3 * B * N >= 2 ** 31:
        raise ValueError("roma_amd.tsdf: at most 65535 problems and 3 B N below 2^31")
    points = points.to(torch.float32).contiguous()
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if counts.shape[0] != B:
            raise ValueError(f"roma_amd.tsdf: counts has {counts.shape[0]} entries for {B} problems")
    out = torch.full((B, 2, 3), float("nan"), device=dev, dtype=torch.float64)
    if B > 0:
        lib = _lib.load()
        nws = int(lib.roma_op_points_bounds_workspace(B))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_points_bounds(_ptr(points), _ptr(counts), B, N, _ptr(out), _ptr(ws), nws, _stream(dev)))
    return out[0] if single else out


def tsdf_bounds(points, counts, dims, margin=0.05):
    """(origin, voxel_size) device tensors of a volume of dims = (nz, ny, nx) that holds the finite rows of points below counts -
    `DenseFusion.points` and `.counts` as they are: `points_bounds`, then `volume_from_bounds`.  No host read."""
    _dims(dims)
    return volume_from_bounds(points_bounds(points, counts), dims, margin)


def _batched(volume):
    """(the volume with a batch axis, single)"""
    if not isinstance(volume, TSDFVolume):
        raise ValueError("roma_amd.tsdf: volume must be a TSDFVolume (tsdf_volume makes one)")
    tsdf = _device_tensor(volume.tsdf, "volume.tsdf")
    if tsdf.dim() not in (3, 4):
        raise ValueError("roma_amd.tsdf: volume.tsdf must be [nz, ny, nx] or [B, nz, ny, nx]")
    single = tsdf.dim() == 3
    vol = TSDFVolume(*(None if o is None else o[None] for o in volume)) if single else volume
    B, dev = int(vol.tsdf.shape[0]), tsdf.device
    nz, ny, nx = _dims(tuple(vol.tsdf.shape[1:]))
    if B > 65535 or B * nz * ny * nx >= 2 ** 31:
        raise ValueError("roma_amd.tsdf: at most 65535 problems and B nz ny nx below 2^31")
    for name, want, dtype in (("tsdf", (B, nz, ny, nx), torch.float32), ("weight", (B, nz, ny, nx), torch.float32),
                              ("color", (B, nz, ny, nx, 3), torch.float32), ("origin", (B, 3), torch.float64),
                              ("voxel_size", (B,), torch.float64), ("trunc", (B,), torch.float64)):
        x = getattr(vol, name)
        if x is None and name == "color":
            continue
        x = _device_tensor(x, "volume." + name)
        if tuple(x.shape) != want or x.dtype != dtype or x.device != dev or not x.is_contiguous():
            raise ValueError(f"roma_amd.tsdf: volume.{name} must be a contiguous {dtype} tensor {list(want)} on {dev}: the state is updated in place")
    return vol, single


def integrate_depth_maps(volume, depth, K, R, t, *, depth_weight=None, images=None, view_valid=None, valid=None, max_weight=64.0,
                         near=1e-6):
    """V <= 8 depth maps into a volume, in place (`roma_op_tsdf_integrate`); more views are more calls, and the result is the same
    in every bit whether views come in one call or in several.

    volume: a TSDFVolume; depth [B, V, H, W] float32 ([V, H, W] with a single volume), NaN or <= 0 where there is none -
    `DenseFusion.depth` as it is; depth_weight of the same shape (default 1; `DenseFusion.weight` fits); K [V, 3, 3], [3, 3] or
    [B, V, 3, 3] IN GRID UNITS (the centre of cell (r, c) is (c + 0.5, r + 0.5)) as `fuse_depth_maps` takes them; R [B, V, 3, 3],
    t [B, V, 3] with x_cam = R X + t; view_valid [B, V] or [V], valid [B]; images: V uint8 device tensors [H_img, W_img, 3] (per
    problem: a list of B such lists), required exactly when the volume has colour.

    A voxel takes the views in view order; for each, its centre is projected, the cell that holds it gives d and w, and with
    sdf = d - z >= -trunc the voxel's tsdf becomes the weighted mean with min(1, sdf / trunc), its weight grows by w up to
    max_weight, and with sdf <= trunc its colour takes the same update from the image pixel that holds the cell's centre.

    Returns the same TSDFVolume (its tensors are updated).  No host synchronisation."""
    vol, single = _batched(volume)
    B, (nz, ny, nx), dev = int(vol.tsdf.shape[0]), tuple(int(d) for d in vol.tsdf.shape[1:]), vol.tsdf.device
    depth = _device_tensor(depth, "depth")
    if depth.dim() != (3 if single else 4) or (not single and int(depth.shape[0]) != B):
        raise ValueError(f"roma_amd.tsdf: depth must be [V, H, W] for one volume and [B, V, H, W] for a batch, got {tuple(depth.shape)}")
    V, H, W = (int(d) for d in depth.shape[-3:])
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"roma_amd.tsdf: need 1 <= V <= {MAX_VIEWS} views a call, got {V}")
    if H < 1 or W < 1 or B * V * H * W >= 2 ** 31:
        raise ValueError("roma_amd.tsdf: the depth maps must not be empty and B V H W must be below 2^31")
    max_weight, near = float(max_weight), float(near)
    if not max_weight > 0 or not near >= 0:
        raise ValueError("roma_amd.tsdf: max_weight must be positive and near must not be negative")
    if (images is not None) != (vol.color is not None):
        raise ValueError("roma_amd.tsdf: images go with a volume that has colour, and such a volume needs them")
    depth = depth.to(device=dev, dtype=torch.float32).reshape(B, V, H, W).contiguous()
    if depth_weight is not None:
        depth_weight = _device_tensor(depth_weight, "depth_weight")
        if depth_weight.numel() != depth.numel():
            raise ValueError(f"roma_amd.tsdf: depth_weight must have the shape of depth, got {tuple(depth_weight.shape)}")
        depth_weight = depth_weight.to(device=dev, dtype=torch.float32).reshape(B, V, H, W).contiguous()
    R, t = _device_tensor(R, "R"), _device_tensor(t, "t")
    if R.numel() != B * V * 9 or t.numel() != B * V * 3:
        raise ValueError(f"roma_amd.tsdf: R and t must hold {B} x {V} poses, got {tuple(R.shape)} and {tuple(t.shape)}")
    R = R.to(device=dev, dtype=torch.float64).reshape(B, V, 3, 3).contiguous()
    t = t.to(device=dev, dtype=torch.float64).reshape(B, V, 3).contiguous()
    if K is None:
        raise ValueError("roma_amd.tsdf: K is required (the cameras in grid units)")
    from .bundle import _view_cameras
    from .depth_fusion import _colour_source
    K = _view_cameras(K, B, V, dev)
    if view_valid is not None:
        view_valid = torch.as_tensor(view_valid).to(device=dev)
        view_valid = view_valid[None].expand(B, V) if tuple(view_valid.shape) == (V,) else view_valid
        if tuple(view_valid.shape) != (B, V):
            raise ValueError(f"roma_amd.tsdf: view_valid must be [{V}] or [{B}, {V}], got {tuple(view_valid.shape)}")
        view_valid = (view_valid != 0).to(torch.uint8).contiguous()
    valid = _valid(valid, B, dev)
    packed = offsets = sizes = None
    if images is not None:
        packed, offsets, sizes = _colour_source(images, B, V, single, dev)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_tsdf_integrate(
                _ptr(depth), _ptr(depth_weight), _ptr(K), _ptr(R), _ptr(t), _ptr(view_valid), _ptr(valid), _ptr(packed),
                offsets.ctypes.data if offsets is not None else None, sizes.ctypes.data if sizes is not None else None,
                _ptr(vol.origin), _ptr(vol.voxel_size), _ptr(vol.trunc), B, V, H, W, nz, ny, nx, max_weight, near,
                _ptr(vol.tsdf), _ptr(vol.weight), _ptr(vol.color), _stream(dev)))
    return volume


def default_mesh_sizes(dims):
    """(max_vertices, max_faces) = (16 (nx ny + ny nz + nx nz), twice that).  A heuristic: a closed surface takes about 4.5
    vertices per cell^2 of its area and 2 V - 4 faces, so this holds a surface of about 3.5 times the area of the three mid-planes
    of the volume.  `Mesh.totals` says what there was: compare it with `Mesh.counts`."""
    nz, ny, nx = _dims(dims)
    max_vertices = 16 * (nx * ny + ny * nz + nx * nz)
    return max_vertices, 2 * max_vertices


def extract_mesh(volume, *, min_weight=1.0, max_vertices=None, max_faces=None, valid=None):
    """The zero level set of a volume as a triangle mesh (`roma_op_tsdf_extract_mesh`), by marching tetrahedra on the Kuhn split
    of every cell: a voxel counts when its weight is at least min_weight and is inside when tsdf < 0; an edge between an inside
    and an outside voxel carries one vertex at the linear zero crossing, with the interpolated colour and the normalised
    interpolated gradient of tsdf as its normal; triangles are wound so that their normal points to the outside.  The mesh is
    watertight where the volume was observed and open at the rim of it; `stats` counts the rim vertices no triangle uses.  Rows
    beyond max_vertices / max_faces (default: `default_mesh_sizes`) are not written and `totals` says how many there were; a face
    that names a cut vertex is (-1, -1, -1).  Returns Mesh; a single volume gives it without the batch axis.  No host read."""
    vol, single = _batched(volume)
    B, (nz, ny, nx), dev = int(vol.tsdf.shape[0]), tuple(int(d) for d in vol.tsdf.shape[1:]), vol.tsdf.device
    max_vertices = default_mesh_sizes((nz, ny, nx))[0] if max_vertices is None else int(max_vertices)
    max_faces = 2 * max_vertices if max_faces is None else int(max_faces)
    min_weight = float(min_weight)
    if not min_weight > 0:
        raise ValueError("roma_amd.tsdf: min_weight must be positive (a voxel of weight 0 holds nothing)")
    if max_vertices < 0 or max_faces < 0 or 3 * B * max(max_vertices, max_faces) >= 2 ** 31:
        raise ValueError("roma_amd.tsdf: max_vertices and max_faces must not be negative and 3 B times either below 2^31")
    valid = _valid(valid, B, dev)
    f32 = dict(device=dev, dtype=torch.float32)
    vertices, normals = torch.empty((B, max_vertices, 3), **f32), torch.empty((B, max_vertices, 3), **f32)
    colors = torch.empty((B, max_vertices, 3), device=dev, dtype=torch.uint8) if vol.color is not None else None
    faces = torch.empty((B, max_faces, 3), device=dev, dtype=torch.int32)
    counts, totals = (torch.zeros((B, 2), device=dev, dtype=torch.int32) for _ in range(2))
    stats = torch.zeros((B, 8), device=dev, dtype=torch.int32)
    if B > 0:
        lib = _lib.load()
        nws = int(lib.roma_op_tsdf_extract_mesh_workspace(B, nz, ny, nx, max_vertices))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_tsdf_extract_mesh(
                _ptr(vol.tsdf), _ptr(vol.weight), _ptr(vol.color), _ptr(valid), _ptr(vol.origin), _ptr(vol.voxel_size), B, nz, ny, nx,
                min_weight, max_vertices, max_faces, _ptr(vertices), _ptr(normals), _ptr(colors), _ptr(faces), _ptr(counts),
                _ptr(totals), _ptr(stats), _ptr(ws), nws, _stream(dev)))
    out = Mesh(vertices, normals, colors, faces, counts, totals, stats)
    return Mesh(*(None if o is None else o[0] for o in out)) if single else out


def mesh_from_fusion(fusion, K, R, t, images=None, *, dims=(128, 128, 128), trunc_voxels=4.0, margin=0.05, use_weight=True,
                     view_valid=None, max_weight=64.0, near=1e-6, min_weight=None, max_vertices=None, max_faces=None):
    """A `DenseFusion` to a mesh: `tsdf_bounds` of its cloud -> `tsdf_volume` (trunc = trunc_voxels voxels, with colour when images
    are given) -> `integrate_depth_maps` of its fused depth maps (weighted by `fusion.weight` with use_weight) -> `extract_mesh`.
    K in grid units, R, t and images as `fuse_depth_maps` took them.  min_weight defaults to the smallest positive float32: every
    voxel that a view touched counts.  Returns (Mesh, TSDFVolume); composition only, no host read."""
    from .depth_fusion import DenseFusion
    if not isinstance(fusion, DenseFusion):
        raise ValueError("roma_amd.tsdf: fusion must be the DenseFusion that fuse_depth_maps returned")
    _device_tensor(fusion.points, "fusion.points")
    trunc_voxels = float(trunc_voxels)
    if not trunc_voxels > 0:
        raise ValueError("roma_amd.tsdf: trunc_voxels must be positive")
    origin, voxel_size = tsdf_bounds(fusion.points, fusion.counts, dims, margin)
    volume = tsdf_volume(dims, origin, voxel_size, voxel_size * trunc_voxels, color=images is not None)
    integrate_depth_maps(volume, fusion.depth, K, R, t, depth_weight=fusion.weight if use_weight else None, images=images,
                         view_valid=view_valid, max_weight=max_weight, near=near)
    tiny = float(np.finfo(np.float32).tiny)
    return extract_mesh(volume, min_weight=tiny if min_weight is None else min_weight, max_vertices=max_vertices, max_faces=max_faces), volume


def ply_bytes(vertices, normals, colors, faces):
    """A binary little-endian PLY of host arrays: vertices, normals float32 [n, 3], colors uint8 [n, 3] or None, faces int32 [m, 3]"""
    vertices, normals = np.asarray(vertices, dtype="<f4").reshape(-1, 3), np.asarray(normals, dtype="<f4").reshape(-1, 3)
    faces = np.asarray(faces, dtype="<i4").reshape(-1, 3)
    if len(normals) != len(vertices) or (colors is not None and len(colors) != len(vertices)):
        raise ValueError("roma_amd.tsdf: vertices, normals and colors must have the same number of rows")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vertices)}"]
    head += [f"property {'float' if kind == '<f4' else 'uchar'} {name}" for name, kind in fields]
    head += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    rows = np.zeros(len(vertices), dtype=fields)
    for a, name in enumerate(("x", "y", "z")):
        rows[name], rows["n" + name] = vertices[:, a], normals[:, a]
    if colors is not None:
        colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
        rows["red"], rows["green"], rows["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
    tri = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    tri["n"], tri["v"] = 3, faces
    return ("\n".join(head) + "\n").encode("ascii") + rows.tobytes() + tri.tobytes()


def write_ply(path, mesh):
    """Write one mesh (no batch axis) as binary little-endian PLY: the vertices, normals and colours below counts[0] and the faces
    below counts[1] that name no cut vertex.  The module's only host read."""
    if not isinstance(mesh, Mesh) or mesh.vertices.dim() != 2:
        raise ValueError("roma_amd.tsdf: write_ply takes one Mesh without a batch axis")
    nv, nf = (int(c) for c in mesh.counts.cpu())
    faces = mesh.faces[:nf].cpu().numpy()
    faces = faces[(faces >= 0).all(axis=1)]
    data = ply_bytes(mesh.vertices[:nv].cpu().numpy(), mesh.normals[:nv].cpu().numpy(),
                     None if mesh.colors is None else mesh.colors[:nv].cpu().numpy(), faces)
    with open(path, "wb") as f:
        f.write(data)
    return nv, len(faces)
