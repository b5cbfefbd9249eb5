"""Device-side input preparation for the eval loop.

``get_bbox`` is the host integer arithmetic of tools/eval_ycb.py:54-90 (snap the detector ROI to the
border list, keep it inside the 480x640 frame); ``preprocess_objects`` runs everything the reference
then does in numpy per object (tools/eval_ycb.py:150-181) as one HIP launch over B objects of one
crop size: mask, ``choose`` sampling, depth back-projection, normalised colour crop.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib

BORDER_LIST = [-1, 40, 80, 120, 160, 200, 240, 280, 320, 360, 400, 440, 480, 520, 560, 600, 640, 680]
IMG_WIDTH, IMG_LENGTH = 480, 640            # eval_ycb.py:43-44 (rows, columns)
YCB_CAM = dict(cx=312.9869, cy=241.3109, fx=1066.778, fy=1067.487, scale=10000.0)     # eval_ycb.py:37-41
# datasets/linemod/dataset.py:73-76,152-157: back-projection in millimetres (cam_scale 1), finished cloud / 1000
IMG_MEAN, IMG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # the kernel's normalisation (applied to 0-255-scale pixels, eval_ycb.py:33)
LINEMOD_CAM = dict(cx=325.26110, cy=242.04899, fx=572.41140, fy=573.57043, scale=1.0, cloud_div=1000.0)


def _snap(extent):
    for lo, hi in zip(BORDER_LIST[:-1], BORDER_LIST[1:]):
        if lo < extent < hi:
            return hi
    return extent


def get_bbox(roi, img_width=IMG_WIDTH, img_length=IMG_LENGTH):
    """PoseCNN roi row [batch, cls, x1, y1, x2, y2, ...] -> (rmin, rmax, cmin, cmax)  (eval_ycb.py:54-90)."""
    rmin, rmax = int(roi[3]) + 1, int(roi[5]) - 1
    cmin, cmax = int(roi[2]) + 1, int(roi[4]) - 1
    r_b, c_b = _snap(rmax - rmin), _snap(cmax - cmin)
    cr, cc = int((rmin + rmax) / 2), int((cmin + cmax) / 2)
    rmin, rmax = cr - int(r_b / 2), cr + int(r_b / 2)
    cmin, cmax = cc - int(c_b / 2), cc + int(c_b / 2)
    if rmin < 0:
        rmax, rmin = rmax - rmin, 0
    if cmin < 0:
        cmax, cmin = cmax - cmin, 0
    if rmax > img_width:
        rmin, rmax = rmin - (rmax - img_width), img_width
    if cmax > img_length:
        cmin, cmax = cmin - (cmax - img_length), img_length
    return rmin, rmax, cmin, cmax


def preprocess_objects(rgb, depth, label, objects, num_points, cam=YCB_CAM, choose_in=None):
    """rgb [F,IH,IW,3] uint8, depth [F,IH,IW] uint16 (as int16 bits is fine), label [F,IH,IW] int32 -- device tensors.
    objects: list of (frame, itemid, (rmin, rmax, cmin, cmax), seed), all boxes of one size.
    choose_in (optional, [B,N] / [B,1,N] int64): the chosen pixel indices as an INPUT (sampling skipped) -- the reference's own
    np.random.shuffle subset in the golden tests.
    Returns img [B,3,H,W], cloud [B,N,3], choose [B,1,N] int64, count [B] int32 (0 = lost detection)."""
    if not (rgb.is_cuda and depth.is_cuda and label.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    F, IH, IW, _ = rgb.shape
    B = len(objects)
    H = objects[0][2][1] - objects[0][2][0]
    W = objects[0][2][3] - objects[0][2][2]
    desc = np.zeros((B, 8), dtype=np.int32)
    for i, (frame, itemid, (rmin, rmax, cmin, cmax), seed) in enumerate(objects):
        if rmax - rmin != H or cmax - cmin != W:
            raise RuntimeError("preprocess_objects: all boxes of one call must have the same size")
        if not (0 <= frame < F and 0 <= rmin and rmax <= IH and 0 <= cmin and cmax <= IW):
            raise RuntimeError("preprocess_objects: box outside the frame")
        desc[i, :6] = (frame, itemid, rmin, rmax, cmin, cmax)
        desc[i, 6] = np.array([seed & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0]      # uint32 seed bits
        desc[i, 7] = 1 if choose_in is not None else 0
    dev = rgb.device
    d_desc = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)      # pinned: the upload does not wait for the stream
    rgb, label = rgb.contiguous(), label.to(torch.int32).contiguous()
    depth = depth.contiguous()
    if depth.dtype not in (torch.int16, torch.uint16):
        raise RuntimeError("preprocess_objects: depth must be 16-bit")
    scratch = torch.empty(B * H * W, dtype=torch.int32, device=dev)
    img = torch.empty(B, 3, H, W, device=dev)
    cloud = torch.empty(B, num_points, 3, device=dev)
    if choose_in is not None:
        choose = choose_in.to(device=dev, dtype=torch.int64).reshape(B, 1, num_points).contiguous().clone()
    else:
        choose = torch.empty(B, 1, num_points, dtype=torch.int64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        st = _lib.lib().df_preprocess_objects(rgb.data_ptr(), depth.data_ptr(), label.data_ptr(), F, IH, IW, d_desc.data_ptr(), B,
                                              H, W, num_points, cam["cx"], cam["cy"], cam["fx"], cam["fy"], cam["scale"], cam.get("cloud_div", 1.0),
                                              scratch.data_ptr(), img.data_ptr(), cloud.data_ptr(), choose.data_ptr(),
                                              count.data_ptr(), _lib.current_stream())
    _lib.check(st, "preprocess_objects")
    return img, cloud, choose, count


def _on_device(x, np_dtype, dev, ok, error):
    """A host array, a host tensor or a device tensor -> a contiguous device tensor.  ``ok(tensor)`` checks dtype and shape before
    anything is uploaded (``RuntimeError(error)`` otherwise); host data goes up from pinned memory: the upload does not wait for the stream."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype))
    if not ok(x):
        raise RuntimeError(error)
    if not x.is_cuda:
        x = (x if x.is_pinned() else x.pin_memory()).to(dev, non_blocking=True)
    return x.contiguous()


def _u16(t, what):
    if t.dtype not in (torch.int16, torch.uint16):
        raise RuntimeError(f"{what} must be 16-bit")
    return t.contiguous()


def cad_frame_stats(depth, label, label_value=65535):
    """customCAD frames (``df_cad_frame_stats``): depth, label [F,IH,IW] 16-bit device tensors -> stats [F,6] int32 on the device,
    ``{depth_max, n_label, rmin, rmax, cmin, cmax}`` per frame: np.max(depth), the number of label pixels and their INCLUSIVE box
    (get_bbox of datasets/customCAD/dataset.py:247-249); n_label = 0 and a zero box without the label.  No read-back here."""
    if not (depth.is_cuda and label.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    if depth.dim() != 3 or depth.shape != label.shape:
        raise RuntimeError("cad_frame_stats: depth and label must both be [F,IH,IW]")
    depth, label = _u16(depth, "cad_frame_stats: depth"), _u16(label, "cad_frame_stats: label")
    F, IH, IW = depth.shape
    stats = torch.empty(F, 6, dtype=torch.int32, device=depth.device)
    with _lib.device_guard(depth.device):
        st = _lib.lib().df_cad_frame_stats(depth.data_ptr(), label.data_ptr(), F, IH, IW, int(label_value), stats.data_ptr(), _lib.current_stream())
    _lib.check(st, "cad_frame_stats")
    return stats


def cad_item_table(depth, label, label_value=65535, min_side=8):
    """customCAD frames that stay on the device (``df_cad_item_table``): depth, label [F,IH,IW] 16-bit device tensors -> table [F,8]
    int32 on the device: the six entries of ``cad_frame_stats``, then ``count``, the mask pixels ``(label == label_value) & (depth !=
    depth_max)`` of the half-open crop ``[rmin:rmax, cmin:cmax]`` (``PoseDataset._count``), and ``live``: ``n_label > 0``, both crop
    sides at least ``min_side`` and ``count > 0`` (``PoseDataset._live_box`` plus the count test).  No read-back here."""
    if not (depth.is_cuda and label.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    if depth.dim() != 3 or depth.shape != label.shape:
        raise RuntimeError("cad_item_table: depth and label must both be [F,IH,IW]")
    depth, label = _u16(depth, "cad_item_table: depth"), _u16(label, "cad_item_table: label")
    F, IH, IW = depth.shape
    table = torch.empty(F, 8, dtype=torch.int32, device=depth.device)
    with _lib.device_guard(depth.device):
        st = _lib.lib().df_cad_item_table(depth.data_ptr(), label.data_ptr(), F, IH, IW, int(label_value), int(min_side), table.data_ptr(),
                                          _lib.current_stream())
    _lib.check(st, "cad_item_table")
    return table


def cad_targets(model, pose, seeds, num_points, model_scale=10.0, cloud_div=10000.0):
    """The pose half of a customCAD item on the device (``df_cad_targets``).  model [P,3] float64 device tensor (the loader's ``pt[obj]``);
    pose [B,3,4] / [B,12] float64, host or device, ``[R|T]`` with ``R = target_r @ Y_180`` and ``T = target_t`` (``+ add_t * 10000`` with
    noise); seeds: B integers (their low 32 bits) or a [B] int32 device tensor of those bits.  Per item the ``num_points`` model points
    with the smallest ``mix32(seed, index)`` keys, in index order, scaled by ``model_scale``.
    Returns (target, model_points), both [B,num_points,3] float32 on the device, already divided by ``cloud_div``."""
    if not model.is_cuda:
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    if model.dim() != 2 or model.shape[1] != 3 or model.dtype != torch.float64:
        raise RuntimeError("cad_targets: model must be [P,3] float64")
    dev, model = model.device, model.contiguous()
    pose = _cad_pose(pose, dev, "cad_targets")
    B, P, M = pose.shape[0], model.shape[0], int(num_points)
    if torch.is_tensor(seeds):
        if tuple(seeds.shape) != (B,) or seeds.dtype != torch.int32 or not seeds.is_cuda:
            raise RuntimeError("cad_targets: seeds as a tensor must be [B] int32 on the device")
        seeds = seeds.contiguous()
    else:
        bits = np.array([int(s) & 0xFFFFFFFF for s in seeds], dtype=np.uint32).view(np.int32)
        if bits.shape != (B,):
            raise RuntimeError("cad_targets: one seed per pose")
        seeds = torch.from_numpy(bits).pin_memory().to(dev, non_blocking=True)
    with _lib.device_guard(dev):
        L = _lib.lib()
        need = L.df_cad_targets_scratch_bytes(B, P, M)
        if need == 0:
            raise RuntimeError(f"cad_targets: bad sizes (B 1..65535, 1 <= num_points <= P <= 2^24); got B {B}, P {P}, num_points {M}")
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        model_points = torch.empty(B, M, 3, device=dev)
        target = torch.empty(B, M, 3, device=dev)
        st = L.df_cad_targets(model.data_ptr(), P, float(model_scale), pose.data_ptr(), seeds.data_ptr(), B, M, float(cloud_div),
                              scratch.data_ptr(), need, model_points.data_ptr(), target.data_ptr(), _lib.current_stream())
    _lib.check(st, "cad_targets")
    return target, model_points


def preprocess_objects_cad(rgb, depth, label, objects, num_points, frame_stats, ray_map, p22, p23, add_t=None, cloud_div=10000.0, choose_in=None):
    """The customCAD counterpart of ``preprocess_objects`` (``df_preprocess_objects_cad``).  rgb [F,IH,IW,3] uint8, depth and label
    [F,IH,IW] 16-bit, frame_stats [F,6] int32 (``cad_frame_stats``), ray_map [IH,IW,3] float64 -- device tensors; p22, p23: the
    projection matrix' [2,2] and [2,3]; objects: list of (frame, label_value, (rmin, rmax, cmin, cmax), seed), all boxes of one size;
    add_t (optional): [B,3] float64, host or device, added to the float32 points in fp64 before the division by ``cloud_div``.
    Returns img [B,3,H,W], cloud [B,N,3], choose [B,1,N] int64, count [B] int32 (0 = no mask pixel in the box)."""
    if not (rgb.is_cuda and depth.is_cuda and label.is_cuda and frame_stats.is_cuda and ray_map.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    F, IH, IW, _ = rgb.shape
    if tuple(depth.shape) != (F, IH, IW) or tuple(label.shape) != (F, IH, IW):
        raise RuntimeError("preprocess_objects_cad: depth and label must be [F,IH,IW] like rgb")
    if tuple(frame_stats.shape) != (F, 6) or frame_stats.dtype != torch.int32:
        raise RuntimeError("preprocess_objects_cad: frame_stats must be [F,6] int32")
    if tuple(ray_map.shape) != (IH, IW, 3) or ray_map.dtype != torch.float64:
        raise RuntimeError("preprocess_objects_cad: ray_map must be [IH,IW,3] float64")
    B = len(objects)
    H = objects[0][2][1] - objects[0][2][0]
    W = objects[0][2][3] - objects[0][2][2]
    desc = np.zeros((B, 8), dtype=np.int32)
    for i, (frame, label_value, (rmin, rmax, cmin, cmax), seed) in enumerate(objects):
        if rmax - rmin != H or cmax - cmin != W:
            raise RuntimeError("preprocess_objects_cad: all boxes of one call must have the same size")
        if not (0 <= frame < F and 0 <= rmin and rmax <= IH and 0 <= cmin and cmax <= IW):
            raise RuntimeError("preprocess_objects_cad: box outside the frame")
        desc[i, :6] = (frame, label_value, rmin, rmax, cmin, cmax)
        desc[i, 6] = np.array([seed & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0]      # uint32 seed bits
        desc[i, 7] = 1 if choose_in is not None else 0
    dev = rgb.device
    d_desc = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)      # pinned: the upload does not wait for the stream
    if add_t is not None:
        add_t = _on_device(add_t, np.float64, dev, lambda t: tuple(t.shape) == (B, 3) and t.dtype == torch.float64,
                           "preprocess_objects_cad: add_t must be [B,3] float64")
    rgb, depth, label = rgb.contiguous(), _u16(depth, "preprocess_objects_cad: depth"), _u16(label, "preprocess_objects_cad: label")
    scratch = torch.empty(B * H * W, dtype=torch.int32, device=dev)
    img = torch.empty(B, 3, H, W, device=dev)
    cloud = torch.empty(B, num_points, 3, device=dev)
    if choose_in is not None:
        choose = choose_in.to(device=dev, dtype=torch.int64).reshape(B, 1, num_points).contiguous().clone()
    else:
        choose = torch.empty(B, 1, num_points, dtype=torch.int64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        st = _lib.lib().df_preprocess_objects_cad(rgb.data_ptr(), depth.data_ptr(), label.data_ptr(), F, IH, IW, d_desc.data_ptr(),
                                                  frame_stats.contiguous().data_ptr(), _lib.dptr(ray_map), float(p22), float(p23),
                                                  None if add_t is None else add_t.data_ptr(), B, H, W, num_points, float(cloud_div),
                                                  scratch.data_ptr(), img.data_ptr(), cloud.data_ptr(), choose.data_ptr(), count.data_ptr(),
                                                  _lib.current_stream())
    _lib.check(st, "preprocess_objects_cad")
    return img, cloud, choose, count


def _cad_pose(pose, dev, name):
    """pose [F,3,4] / [F,12] float64, host or device -> the device tensor"""
    return _on_device(pose, np.float64, dev, lambda p: p.dtype == torch.float64 and p.dim() in (2, 3) and p.numel() == p.shape[0] * 12,
                      f"{name}: pose must be [F,3,4] float64")


def _cad_proj(proj, name):
    proj = np.ascontiguousarray(proj, dtype=np.float64)
    if proj.shape != (4, 4):
        raise RuntimeError(f"{name}: proj must be 4 x 4")
    return proj


def _cad_holes(holes, F, name):
    """None or (hole_idx [F,K], hole_r [F,K]) -> (K, hole_idx int32, hole_r float64), the arrays None without holes"""
    if holes is None:
        return 0, None, None
    hole_idx, hole_r = np.ascontiguousarray(holes[0], dtype=np.int32), np.ascontiguousarray(holes[1], dtype=np.float64)
    if hole_idx.ndim != 2 or hole_idx.shape[0] != F or hole_r.shape != hole_idx.shape:
        raise RuntimeError(f"{name}: holes must be (hole_idx [F,K], hole_r [F,K])")
    return hole_idx.shape[1], hole_idx, hole_r


def _cad_scratch(scratch, need, dev, name, sizes):
    """The caller's scratch, checked against the ``need`` bytes the library asks for (0: it refuses the sizes), or a new one"""
    if need == 0:
        raise RuntimeError(f"{name}: bad sizes {sizes}")
    if scratch is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if not scratch.is_cuda or scratch.dtype != torch.uint8 or scratch.numel() < need:
        raise RuntimeError(f"{name}: scratch must be a uint8 device tensor of at least {need} bytes")
    return scratch


def _cad_frames(F, IH, IW, dev):
    """rgb [F,IH,IW,3] uint8, depth [F,IH,IW] uint16 and a third uint16 image (mask or label), uninitialised"""
    u16 = lambda: torch.empty(F, IH, IW, dtype=torch.int16, device=dev).view(torch.uint16)
    return torch.empty(F, IH, IW, 3, dtype=torch.uint8, device=dev), u16(), u16()


def _cad_mesh(vertices, colors, triangles, name):
    """The checks of a mesh on the device: vertices [V,3] float32, colors [V,3] uint8, triangles [T,3] int32 -> (V, T)"""
    if not (vertices.is_cuda and colors.is_cuda and triangles.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise RuntimeError(f"{name}: vertices must be [V,3] float32")
    V = vertices.shape[0]
    if tuple(colors.shape) != (V, 3) or colors.dtype != torch.uint8:
        raise RuntimeError(f"{name}: colors must be [V,3] uint8")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype != torch.int32:
        raise RuntimeError(f"{name}: triangles must be [T,3] int32")
    return V, triangles.shape[0]


def _cad_light(normals, normal_mode, light, V, T, F, dev, name):
    """The lit calls' three arguments, checked: normals [T,3] (normal_mode 0) or [V,3] (1) float32 on the device, light [F,8] float64,
    host or device -> (normals, normal_mode, the light on the device)"""
    if normals is None:
        raise RuntimeError(f"{name}: a light needs normals")
    if normal_mode not in (0, 1):
        raise RuntimeError(f"{name}: normal_mode {normal_mode} is neither 0 (per triangle) nor 1 (per vertex)")
    rows = V if normal_mode else T
    if not torch.is_tensor(normals) or not normals.is_cuda or normals.dtype != torch.float32 or tuple(normals.shape) != (rows, 3):
        raise RuntimeError(f"{name}: normals must be a [{rows},3] float32 device tensor for normal_mode {normal_mode}")
    light = _on_device(light, np.float64, dev, lambda p: p.dtype == torch.float64 and tuple(p.shape) == (F, 8),
                       f"{name}: light must be [F,8] float64")
    return normals, int(normal_mode), light


def cad_render(points, normals, colors, pose, model_scale, proj, image_dims, holes=None, splat=0, mask_mode=0, scratch=None):
    """F views of a coloured cloud as customCAD frames (``df_cad_render``; the contract is its comment in include/dfusion.h).
    points [P,3] float32, normals [P,3] float32 or None, colors [P,3] uint8 -- device tensors; pose [F,3,4] / [F,12] float64 [R|t] into
    camera space, host or device; proj: the 4 x 4 projection matrix (host); image_dims = (rows, columns); holes: None or HOST
    (hole_idx [F,K] int32 with -1 = none, hole_r [F,K] float64); mask_mode 0 = box, 1 = pixels; scratch: an optional uint8 device
    tensor of at least ``df_cad_render_scratch_bytes`` to reuse between calls.
    Returns rgb [F,IH,IW,3] uint8, depth and mask [F,IH,IW] uint16, stats [F,6] int32 on the device; no read-back, no synchronisation."""
    if not (points.is_cuda and colors.is_cuda and (normals is None or normals.is_cuda)):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise RuntimeError("cad_render: points must be [P,3] float32")
    P = points.shape[0]
    if tuple(colors.shape) != (P, 3) or colors.dtype != torch.uint8:
        raise RuntimeError("cad_render: colors must be [P,3] uint8")
    if normals is not None and (tuple(normals.shape) != (P, 3) or normals.dtype != torch.float32):
        raise RuntimeError("cad_render: normals must be [P,3] float32")
    dev = points.device
    pose = _cad_pose(pose, dev, "cad_render")
    F, IH, IW = pose.shape[0], int(image_dims[0]), int(image_dims[1])
    proj = _cad_proj(proj, "cad_render")
    K, hole_idx, hole_r = _cad_holes(holes, F, "cad_render")
    L = _lib.lib()
    scratch = _cad_scratch(scratch, L.df_cad_render_scratch_bytes(F, IH, IW), dev, "cad_render", f"F={F}, IH={IH}, IW={IW}")
    rgb, depth, mask = _cad_frames(F, IH, IW, dev)
    stats = torch.empty(F, 6, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        st = L.df_cad_render(_lib.dptr(points), None if normals is None else _lib.dptr(normals), _lib.dptr(colors), P, pose.data_ptr(),
                             float(model_scale), hole_idx.ctypes.data if K else None, hole_r.ctypes.data if K else None, K,
                             proj.ctypes.data, F, IH, IW, int(splat), int(mask_mode), rgb.data_ptr(), depth.data_ptr(), mask.data_ptr(),
                             stats.data_ptr(), scratch.data_ptr(), scratch.numel(), _lib.current_stream())
    _lib.check(st, "cad_render")
    return rgb, depth, mask, stats


def cad_render_mesh(vertices, colors, triangles, pose, model_scale, proj, image_dims, holes=None, cull=1, mask_mode=0, scratch=None,
                    normals=None, normal_mode=0, light=None):
    """F views of a coloured triangle mesh as customCAD frames (``df_cad_render_mesh``; the contract is its comment in include/dfusion.h).
    vertices [V,3] float32, colors [V,3] uint8, triangles [T,3] int32 -- device tensors; pose, proj, image_dims, holes (indices name
    vertices), mask_mode and scratch as for ``cad_render`` (scratch: at least ``df_cad_render_mesh_scratch_bytes``); cull 1 drops the
    triangles that face away.  With ``light`` ([F,8] float64 {Lx, Ly, Lz, ambient, diffuse, cr, cg, cb}, host or device) the covered
    pixels are lit (``df_cad_render_mesh_lit``, steps L1..L6): normals is then a float32 device tensor, [T,3] for normal_mode 0 (flat)
    or [V,3] for normal_mode 1 (smooth).  Without a light normals and normal_mode are ignored.
    Returns rgb [F,IH,IW,3] uint8, depth and mask [F,IH,IW] uint16, stats [F,6] int32 on the device; no read-back, no synchronisation."""
    V, T = _cad_mesh(vertices, colors, triangles, "cad_render_mesh")
    dev = vertices.device
    pose = _cad_pose(pose, dev, "cad_render_mesh")
    F, IH, IW = pose.shape[0], int(image_dims[0]), int(image_dims[1])
    proj = _cad_proj(proj, "cad_render_mesh")
    K, hole_idx, hole_r = _cad_holes(holes, F, "cad_render_mesh")
    L = _lib.lib()
    scratch = _cad_scratch(scratch, L.df_cad_render_mesh_scratch_bytes(F, IH, IW, V, T), dev, "cad_render_mesh",
                           f"F={F}, IH={IH}, IW={IW}, V={V}, T={T}")
    if light is not None:
        normals, normal_mode, light = _cad_light(normals, normal_mode, light, V, T, F, dev, "cad_render_mesh")
    rgb, depth, mask = _cad_frames(F, IH, IW, dev)
    stats = torch.empty(F, 6, dtype=torch.int32, device=dev)
    head = (_lib.dptr(vertices), _lib.dptr(colors), V, _lib.dptr(triangles), T, pose.data_ptr(), float(model_scale),
            hole_idx.ctypes.data if K else None, hole_r.ctypes.data if K else None, K, proj.ctypes.data, F, IH, IW, int(cull), int(mask_mode))
    outs = (rgb.data_ptr(), depth.data_ptr(), mask.data_ptr(), stats.data_ptr(), scratch.data_ptr(), scratch.numel())
    with _lib.device_guard(dev):
        if light is None:
            st = L.df_cad_render_mesh(*head, *outs, _lib.current_stream())
        else:
            st = L.df_cad_render_mesh_lit(*head, _lib.dptr(normals), normal_mode, light.data_ptr(), *outs, _lib.current_stream())
    _lib.check(st, "cad_render_mesh")
    return rgb, depth, mask, stats


def cad_render_scene(vertices, colors, triangles, tri_begin, model_scales, pose, proj, image_dims, present=None, cull=1, scratch=None,
                     normals=None, normal_mode=0, light=None):
    """F frames of O objects with occlusion (``df_cad_render_scene``; the contract is its comment in include/dfusion.h).
    vertices [V,3] float32, colors [V,3] uint8, triangles [T,3] int32 -- device tensors, shared by all objects, the indices global;
    tri_begin [O+1] and model_scales [O] -- HOST; pose [F,O,3,4] / [F,O,12] float64, host or device; present: None (all) or [F,O]
    uint8, host or device; proj, image_dims and scratch (at least ``df_cad_render_scene_scratch_bytes``) as for ``cad_render_mesh``;
    normals, normal_mode and light ([F,8]: one light per frame for all objects) too, the per-triangle normals indexed globally
    (``df_cad_render_scene_lit``).
    Returns rgb [F,IH,IW,3] uint8, depth and label [F,IH,IW] uint16 (label = owner + 1, 0 = horizon), stats [F,O,6] int32 on the
    device; no read-back, no synchronisation."""
    V, T = _cad_mesh(vertices, colors, triangles, "cad_render_scene")
    dev = vertices.device
    tri_begin = np.ascontiguousarray(tri_begin, dtype=np.int32).reshape(-1)
    O = tri_begin.shape[0] - 1
    model_scales = np.ascontiguousarray(model_scales, dtype=np.float64).reshape(-1)
    if O < 1 or model_scales.shape[0] != O:
        raise RuntimeError("cad_render_scene: tri_begin must be [O+1] and model_scales [O], O >= 1")
    pose = _on_device(pose, np.float64, dev, lambda p: p.dtype == torch.float64 and p.dim() in (3, 4) and p.shape[1] == O and
                      p.numel() == p.shape[0] * O * 12, "cad_render_scene: pose must be [F,O,3,4] float64")
    F, IH, IW = pose.shape[0], int(image_dims[0]), int(image_dims[1])
    if present is not None:
        present = _on_device(present, np.uint8, dev, lambda p: p.dtype == torch.uint8 and tuple(p.shape) == (F, O),
                             "cad_render_scene: present must be [F,O] uint8")
    proj = _cad_proj(proj, "cad_render_scene")
    L = _lib.lib()
    scratch = _cad_scratch(scratch, L.df_cad_render_scene_scratch_bytes(F, IH, IW, V, T, O), dev, "cad_render_scene",
                           f"F={F}, IH={IH}, IW={IW}, V={V}, T={T}, O={O}")
    if light is not None:
        normals, normal_mode, light = _cad_light(normals, normal_mode, light, V, T, F, dev, "cad_render_scene")
    rgb, depth, label = _cad_frames(F, IH, IW, dev)
    stats = torch.empty(F, O, 6, dtype=torch.int32, device=dev)
    head = (_lib.dptr(vertices), _lib.dptr(colors), V, _lib.dptr(triangles), T, tri_begin.ctypes.data, model_scales.ctypes.data, O,
            pose.data_ptr(), None if present is None else present.data_ptr(), proj.ctypes.data, F, IH, IW, int(cull))
    outs = (rgb.data_ptr(), depth.data_ptr(), label.data_ptr(), stats.data_ptr(), scratch.data_ptr(), scratch.numel())
    with _lib.device_guard(dev):
        if light is None:
            st = L.df_cad_render_scene(*head, *outs, _lib.current_stream())
        else:
            st = L.df_cad_render_scene_lit(*head, _lib.dptr(normals), normal_mode, light.data_ptr(), *outs, _lib.current_stream())
    _lib.check(st, "cad_render_scene")
    return rgb, depth, label, stats


def cad_scene_mask(label, stats, pairs, mask_mode=0):
    """The loader's mask of each (frame, object) pair of a rendered scene (``df_cad_scene_mask``): label [F,IH,IW] uint16 and
    stats [F,O,6] int32 as ``cad_render_scene`` returns them, pairs [N,2] int32 (host or device).  mask_mode 0 = the half-open slice of
    the object's box, 1 = the pixels the object won.  Returns [N,IH,IW] uint16 on the device; a pair outside the scene gives zeros."""
    if not (label.is_cuda and stats.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    if label.dim() != 3 or label.dtype != torch.uint16 or stats.dim() != 3 or stats.shape[0] != label.shape[0] or stats.shape[2] != 6 or \
            stats.dtype != torch.int32:
        raise RuntimeError("cad_scene_mask: label must be [F,IH,IW] uint16 and stats [F,O,6] int32")
    dev = label.device
    F, IH, IW = label.shape
    O = stats.shape[1]
    if not torch.is_tensor(pairs):
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    pairs = _on_device(pairs, np.int32, dev, lambda p: p.dtype == torch.int32 and p.dim() == 2 and p.shape[1] == 2 and p.shape[0] != 0,
                       "cad_scene_mask: pairs must be a non-empty [N,2] int32")
    N = pairs.shape[0]
    mask = torch.empty(N, IH, IW, dtype=torch.int16, device=dev).view(torch.uint16)
    with _lib.device_guard(dev):
        st = _lib.lib().df_cad_scene_mask(label.contiguous().data_ptr(), stats.contiguous().data_ptr(), F, O, IH, IW, pairs.data_ptr(), N,
                                          int(mask_mode), mask.data_ptr(), _lib.current_stream())
    _lib.check(st, "cad_scene_mask")
    return mask


def cad_depth_sensor(depth, record, seed, first_frame=0, out=None):
    """The depth-sensor model over rendered frames (``df_cad_depth_sensor``; steps D0..D6 of its comment in include/dfusion.h):
    depth [F,IH,IW] uint16 device tensor, the clean render; record = (noise_mul, edge_radius, edge_step, edge_drop24, drop24, quant),
    six integers (``render.DepthSensor.record``); seed and first_frame are taken mod 2^32, frame f of the call draws from
    first_frame + f.  ``out``: an optional [F,IH,IW] uint16 device tensor that shares no memory with ``depth``.
    Returns (depth_out [F,IH,IW] uint16, stats [F,4] int32 = {edge pixels, dropped at random, dropped at an edge, kept and changed})
    on the device; no read-back, no synchronisation."""
    if not depth.is_cuda or depth.dtype != torch.uint16 or depth.dim() != 3:
        raise RuntimeError("cad_depth_sensor: depth must be a [F,IH,IW] uint16 device tensor (no CPU path)")
    record = tuple(int(v) for v in record)
    if len(record) != 6 or any(not -2 ** 31 <= v < 2 ** 31 for v in record):
        raise RuntimeError("cad_depth_sensor: record must hold six 32-bit integers (noise_mul, edge_radius, edge_step, edge_drop24, drop24, quant)")
    dev = depth.device
    F, IH, IW = depth.shape
    depth = depth.contiguous()
    if out is None:
        out = torch.empty(F, IH, IW, dtype=torch.int16, device=dev).view(torch.uint16)
    elif not out.is_cuda or out.device != dev or out.dtype != torch.uint16 or out.shape != depth.shape or not out.is_contiguous():
        raise RuntimeError("cad_depth_sensor: out must be a contiguous [F,IH,IW] uint16 tensor on the depth's device")
    stats = torch.empty(F, 4, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        st = _lib.lib().df_cad_depth_sensor(depth.data_ptr(), out.data_ptr(), F, IH, IW, int(seed) & 0xFFFFFFFF, int(first_frame) & 0xFFFFFFFF,
                                            *record, stats.data_ptr(), _lib.current_stream())
    _lib.check(st, "cad_depth_sensor")
    return out, stats


def color_jitter(frames_u8, plans, out=None):
    """The training colour jitter on the device (``df_color_jitter``): frames_u8 [F,H,W,3] uint8 device tensor, plans [F,8] float32
    (``datasets.augment.plan_row`` rows; host or device).  Returns the jittered uint8 frames, bit-identical to
    ``augment.ColorJitter.apply`` on each; ``out=frames_u8`` works in place."""
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise RuntimeError("color_jitter: frames must be a [F,H,W,3] uint8 device tensor (no CPU path)")
    F, H, W, _ = frames_u8.shape
    dev = frames_u8.device
    if not torch.is_tensor(plans):
        plans = torch.from_numpy(np.ascontiguousarray(plans, dtype=np.float32))
    if tuple(plans.shape) != (F, 8) or plans.dtype != torch.float32:
        raise RuntimeError("color_jitter: plans must be [F,8] float32")
    if not plans.is_cuda:
        plans = (plans if plans.is_pinned() else plans.pin_memory()).to(dev, non_blocking=True)
    out = torch.empty_like(frames_u8) if out is None else out
    if out.shape != frames_u8.shape or out.dtype != torch.uint8 or out.device != dev:
        raise RuntimeError("color_jitter: out must match the frames")
    sums = torch.empty(F, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        st = _lib.lib().df_color_jitter(_lib.dptr(frames_u8), _lib.dptr(plans), F, H, W, sums.data_ptr(), _lib.dptr(out), _lib.current_stream())
    _lib.check(st, "color_jitter")
    return out


def compose_frame(rgb, back=None, mask_back=None, front=None, mask_front=None):
    """The YCB training composition on the device, IN PLACE on rgb [H,W,3] uint8 (``df_compose_frame``; datasets/ycb/dataset.py):
    ``rgb += back`` where mask_back (uint8 wrap-around like the reference's), then ``rgb = front`` where not mask_front.  Masks [H,W]
    uint8 / bool device tensors; a layer and its mask are given together or not at all."""
    if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise RuntimeError("compose_frame: rgb must be a [H,W,3] uint8 device tensor (no CPU path)")
    H, W, _ = rgb.shape
    ptrs = []
    for layer, mask in ((back, mask_back), (front, mask_front)):
        if (layer is None) != (mask is None):
            raise RuntimeError("compose_frame: a layer and its mask come together")
        if layer is None:
            ptrs += [None, None]
            continue
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if layer.shape != rgb.shape or layer.dtype != torch.uint8 or tuple(mask.shape) != (H, W) or mask.dtype != torch.uint8:
            raise RuntimeError("compose_frame: a layer is [H,W,3] uint8, its mask [H,W] uint8 / bool")
        ptrs += [_lib.dptr(layer), _lib.dptr(mask)]
    with _lib.device_guard(rgb.device):
        st = _lib.lib().df_compose_frame(_lib.dptr(rgb), *ptrs, H, W, _lib.current_stream())
    _lib.check(st, "compose_frame")
    return rgb


def seg_batch_check(desc, F, IH, IW, H, W, NB, BH, BW):
    """``ValueError`` for the first bad row of desc [B,8] (the descriptor rule of ``df_seg_batch``); host integers only."""
    for n, (f, y0, x0, flip, b, by0, bx0, _) in enumerate(np.asarray(desc).reshape(-1, 8).tolist()):
        if not 0 <= f < F or not 0 <= y0 <= IH - H or not 0 <= x0 <= IW - W:
            raise ValueError(f"seg_batch: item {n}: frame {f} or window corner ({y0}, {x0}) outside {F} frames of {IH} x {IW} for a {H} x {W} window")
        if not 0 <= flip <= 3 or not -1 <= b < NB:
            raise ValueError(f"seg_batch: item {n}: flip {flip} outside 0..3 or background {b} outside -1..{NB - 1}")
        if b >= 0 and (not 0 <= by0 <= BH - H or not 0 <= bx0 <= BW - W):
            raise ValueError(f"seg_batch: item {n}: background corner ({by0}, {bx0}) outside the {BH} x {BW} pool for a {H} x {W} window")


def seg_batch(rgb, label, class_map, n_classes, desc, window, back=None, blur=1, noise_mul=0, check=True):
    """SegNet training items from rendered scenes (``df_seg_batch``; steps G1..G5 of its comment in include/dfusion.h): rgb
    [F,IH,IW,3] uint8 and label [F,IH,IW] uint16 as ``cad_render_scene`` returns them, class_map [O+1] HOST integers (label value ->
    class, class_map[0] = 0), desc [B,8] int32 rows {f, y0, x0, flip, b, by0, bx0, seed} (host or device), window = (H, W), back
    None or a [NB,BH,BW,3] uint8 device tensor.  A host ``desc`` is checked here and a bad row raises ``ValueError``
    (``check=False`` or a device ``desc``: the call writes zeros for such an item).
    Returns (x [B,H,W,4] float32, target [B,H,W] int64, counts [B,n_classes] int32) on the device; no read-back, no synchronisation."""
    if not (rgb.is_cuda and label.is_cuda) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or label.dtype != torch.uint16 or \
            tuple(label.shape) != tuple(rgb.shape[:3]):
        raise RuntimeError("seg_batch: rgb must be a [F,IH,IW,3] uint8 and label a [F,IH,IW] uint16 device tensor (no CPU path)")
    dev = rgb.device
    F, IH, IW, _ = rgb.shape
    H, W = int(window[0]), int(window[1])
    NB, BH, BW = 0, 0, 0
    if back is not None:
        if not back.is_cuda or back.device != dev or back.dtype != torch.uint8 or back.dim() != 4 or back.shape[3] != 3 or back.shape[0] == 0:
            raise RuntimeError("seg_batch: back must be a non-empty [NB,BH,BW,3] uint8 tensor on the frames' device")
        NB, BH, BW, _ = back.shape
    class_map = np.ascontiguousarray(class_map, dtype=np.int32).reshape(-1)
    if not torch.is_tensor(desc):
        desc = np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, 8)
        if check:
            seg_batch_check(desc, F, IH, IW, H, W, NB, BH, BW)
        desc = (desc & 0xFFFFFFFF).astype(np.uint32).view(np.int32)       # a seed may be given as unsigned
    desc = _on_device(desc, np.int32, dev, lambda d: d.dtype == torch.int32 and d.dim() == 2 and d.shape[1] == 8 and d.shape[0] != 0,
                      "seg_batch: desc must be a non-empty [B,8] int32")
    B = desc.shape[0]
    L = _lib.lib()
    need = L.df_seg_batch_scratch_bytes(B, H, W, int(n_classes))
    if need == 0:
        raise RuntimeError(f"seg_batch: sizes the call refuses (B={B}, H={H}, W={W}, C={n_classes})")
    x = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev)
    target = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    counts = torch.empty(B, int(n_classes), dtype=torch.int32, device=dev)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        st = L.df_seg_batch(_lib.dptr(rgb), _lib.dptr(label), F, IH, IW, None if back is None else _lib.dptr(back), NB, BH, BW,
                            class_map.ctypes.data, class_map.shape[0] - 1, int(n_classes), desc.data_ptr(), B, H, W, int(blur), int(noise_mul),
                            x.data_ptr(), target.data_ptr(), counts.data_ptr(), scratch.data_ptr(), scratch.numel(), _lib.current_stream())
    _lib.check(st, "seg_batch")
    return x, target, counts
