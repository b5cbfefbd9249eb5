"""``PoseDataset`` for the customCAD dataset (Unity renders of CAD models) -- host-side mirror of datasets/customCAD/dataset.py:18-265
of the reference over the device-side input preparation (``df_cad_frame_stats`` + ``df_preprocess_objects_cad``).

Kept from the reference: the constructor ``PoseDataset(mode, num, add_noise, root, noise_trans, refine)``; the layout it reads
(``data/XX/{train,test}.txt``, ``data/XX/rgb/FrameBuffer_NNNN.png``, ``depth/Depth_NNNN.png``, ``mask/NNNN.png``, ``meta/transforms.txt``,
``meta/proj_mat.txt``, ``models/obj_XX.ply``); the every-10th-line rule of 'test' mode (:40-44); the ``transforms.txt`` parser (:59-74) and
the ``index + 1`` lookup into it (:117); the RGBA -> RGB cut (:129); the mask ``label == 65535`` and ``depth != np.max(depth)`` (:120-124),
the crop ``[rmin:rmax, cmin:cmax]`` of the label's INCLUSIVE box (:137-138,247-249: the last row and column are left out) and the grey
(130, 130, 130) on the pixels at the depth maximum (:97,132); the order in which Python's ``random`` is consumed -- the colour jitter's
draws, three ``uniform`` for ``add_t`` (drawn even when unused, :144), ``random.sample`` for the mesh subset (:170); the left- to
right-handed quaternion flip, ``R @ y_180``, ``pos * 1000`` with z negated and ``model * 10``, all divided by 10000 at the end
(:140-143,168-210); the 6-tuple and the six-``LongTensor([0])`` sentinel (:147-149); ``get_sym_list() == []`` and 500 mesh points.

The reference's noise is INCONSISTENT and mirrored as it is, not repaired: with ``add_noise`` the cloud moves by ``add_t / 10000`` (:166
adds ``add_t`` before the final division by 10000, :205) while the target moves by ``add_t`` (:200 adds ``add_t * 10000`` before it).

Different by design:
  * frame sizes come from the files, not the hard-coded (520, 1109) of :99;
  * one ``UnityDepthProjector`` per object directory (the reference keeps the last one only: the same for its single object);
  * a crop with fewer than 8 rows or columns returns the sentinel -- the network's smallest crop, so an object needs 9 rows and 9
    columns of mask -- and so does a frame without any label pixel (the reference fails on it); a sentinel never draws the mesh subset;
  * ``ply_vtx`` is a small reader of its own for ASCII and binary little-endian PLY.  A vertex-only file is subsampled with the reference's
    ``np.random.choice(n, 3000)`` (:261); a mesh is sampled area-weighted with ``np.random`` -- there is no open3d here, so the mesh
    sampling is UNPINNED against open3d's ``sample_points_uniformly`` (:256);
  * the random pixel subset follows the key rule of include/dfusion.h instead of ``np.random.shuffle`` (:151-155).  The mesh subset
    keeps ``random.sample`` here; ``online.RenderedPoseDataset`` draws it by the same key rule on the device (``df_cad_targets``: the
    model points with the smallest ``mix32(seed, index)`` keys, in index order -- the same distribution, without Python's stream);
  * the host only decodes the PNGs: ``batch()`` finds depth maximum and box of every frame with ``df_cad_frame_stats`` (one small read-back
    of [F][6] per call, the only one), then mask, ``choose``, cloud and crop of all frames of one crop size run as one launch and stay on the
    device.  ``host_item`` (the loader's worker processes) finds the box in numpy instead;
  * ``jitter="device"`` keeps the jitter's draws on the host and applies them to the uploaded frames with ``df_color_jitter``.
"""
from __future__ import annotations

import random

import numpy as np
import torch
from PIL import Image
from scipy.spatial.transform import Rotation

from ...lib import preprocess as pp
from .. import augment
from .project_unity_depth import UnityDepthProjector

LABEL_VALUE = 65535
MIN_CROP = 8                     # the engine's smallest crop side
Y_180 = np.diag([-1.0, 1.0, -1.0])

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """(vertices float64 [n,3], triangles int64 [m,3]) of an ASCII or binary little-endian PLY; polygons are cut into fans."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a ply file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elements[-1][2].append((tok[-1], tok[2:4]) if tok[1] == "list" else (tok[-1], tok[1]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"{path}: unsupported ply format {fmt!r}")
        verts, faces = np.zeros((0, 3)), []
        for name, count, props in elements:
            has_list = any(isinstance(t, list) for _, t in props)
            if fmt == "ascii":
                rows = [f.readline().split() for _ in range(count)]
                if name == "vertex":
                    col = [[p for p, _ in props].index(a) for a in "xyz"]
                    verts = np.array([[float(r[c]) for c in col] for r in rows], dtype=np.float64).reshape(count, 3)
                elif name == "face":
                    faces = [[int(v) for v in r[1:1 + int(r[0])]] for r in rows]
            elif not has_list:
                rec = np.frombuffer(f.read(count * np.dtype([(p, "<" + _PLY_TYPES[t]) for p, t in props]).itemsize),
                                    dtype=np.dtype([(p, "<" + _PLY_TYPES[t]) for p, t in props]), count=count)
                if name == "vertex":
                    verts = np.stack([rec[a].astype(np.float64) for a in "xyz"], axis=1)
            else:
                for _ in range(count):
                    for p, t in props:
                        if isinstance(t, list):
                            ct, it = np.dtype("<" + _PLY_TYPES[t[0]]), np.dtype("<" + _PLY_TYPES[t[1]])
                            k = int(np.frombuffer(f.read(ct.itemsize), dtype=ct)[0])
                            vals = np.frombuffer(f.read(k * it.itemsize), dtype=it)
                            if name == "face" and p in ("vertex_indices", "vertex_index"):
                                faces.append(vals.astype(np.int64).tolist())
                        else:
                            f.read(np.dtype(_PLY_TYPES[t]).itemsize)
    tris = [[poly[0], poly[j], poly[j + 1]] for poly in faces for j in range(1, len(poly) - 1)]
    return verts, np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def ply_vtx(path, number_of_points=3000):
    """`number_of_points` model points, float64 [n,3] (dataset.py:251-265).  Vertex-only file: ``pts[np.random.choice(n, number_of_points)]``
    like the reference; mesh: points drawn uniformly over the surface with ``np.random`` (triangle by area, then uniform barycentric
    coordinates) -- the job of open3d's ``sample_points_uniformly``, not its stream."""
    return sample_model_points(*read_ply(path), number_of_points)


def sample_model_points(verts, tris, number_of_points=3000):
    """The draw of ``ply_vtx`` for a model that is already in memory: verts float64 [n,3], tris integer [m,3] (m = 0: a cloud)."""
    if len(tris) == 0:
        return verts[np.random.choice(verts.shape[0], number_of_points)]
    a, b, c = verts[tris[:, 0]], verts[tris[:, 1]], verts[tris[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    t = np.random.choice(len(tris), number_of_points, p=area / area.sum())
    r1, r2 = np.sqrt(np.random.random(number_of_points))[:, None], np.random.random(number_of_points)[:, None]
    return (1.0 - r1) * a[t] + r1 * (1.0 - r2) * b[t] + r1 * r2 * c[t]


def parse_transforms(path):
    """``transforms.txt`` -> {index: [pos (3,), quat (4,)]} (dataset.py:59-74): an index line, ``(x, y, z)``, ``(x, y, z, w)``; reading stops
    at the first record that does not parse."""
    meta = {}
    with open(path, "r") as f:
        while True:
            try:
                idx = int(f.readline().strip())
                pos, quat = (np.array([float(x.rstrip()) for x in f.readline().replace("(", "").replace(")", "").replace(",", "").split(" ")])
                             for _ in range(2))
                meta[idx] = [pos, quat]
            except Exception:
                break
    return meta


def convert_quat(Q):
    """Left- to right-handed quaternion (dataset.py:225-227)."""
    return np.array([-Q[0], -Q[1], Q[2], Q[3]])


def get_bbox(mask):
    """Inclusive (rmin, rmax, cmin, cmax) of a boolean mask (dataset.py:247-249)."""
    a = np.where(mask)
    return int(np.min(a[0])), int(np.max(a[0])), int(np.min(a[1])), int(np.max(a[1]))


def _sentinel():
    cc = torch.LongTensor([0])
    return (cc, cc, cc, cc, cc, cc)


class PoseDataset:
    def __init__(self, mode, num, add_noise, root, noise_trans, refine, device="cuda", seed=0, jitter="host", objlist=(1,)):
        if mode not in ("train", "test"):
            raise ValueError(f"mode must be train / test, got {mode!r}")
        if jitter not in ("host", "device"):
            raise ValueError(f"jitter must be host / device, got {jitter!r}")
        self.objlist = list(objlist)
        self.mode, self.num, self.root, self.refine = mode, int(num), root, refine
        self.noise_trans, self.add_noise = noise_trans, bool(add_noise)
        self.trancolor = augment.ColorJitter(0.2, 0.2, 0.2, 0.05)                  # :90
        self.jitter = jitter
        self._device_jitter = jitter == "device" and self.add_noise
        self.device = torch.device(device)
        self.seed = int(seed)
        self.list_rgb, self.list_depth, self.list_label, self.list_obj, self.list_meta = [], [], [], [], []
        self.meta, self.pt, self.udp = {}, {}, {}
        for item in self.objlist:
            sub = "%02d" % item
            with open(f"{root}/data/{sub}/{'train' if mode == 'train' else 'test'}.txt") as f:
                names = [ln.rstrip("\n") for ln in f if ln.strip()]
            if mode == "test":
                names = names[9::10]            # the running counter of :40-46 ends every list on a multiple of 10
            first = len(self.list_rgb)
            for name in names:
                self.list_rgb.append(f"{root}/data/{sub}/rgb/FrameBuffer_{int(name):04d}.png")
                self.list_depth.append(f"{root}/data/{sub}/depth/Depth_{int(name):04d}.png")
                self.list_label.append(f"{root}/data/{sub}/mask/{int(name):04d}.png")
                self.list_meta.append(int(name))
                self.list_obj.append(item)
            self.meta[item] = parse_transforms(f"{root}/data/{sub}/meta/transforms.txt")
            self.pt[item] = ply_vtx(f"{root}/models/obj_{sub}.ply")
            if names:                            # the frame size of this object directory, from its first depth image's header
                with Image.open(self.list_depth[first]) as im:
                    self.udp[item] = UnityDepthProjector(f"{root}/data/{sub}/meta/proj_mat.txt", (im.height, im.width))
        self.length = len(self.list_rgb)
        self.num_pt_mesh_large = self.num_pt_mesh_small = 500

    def __len__(self):
        return self.length

    def get_sym_list(self):
        return []

    def get_num_points_mesh(self):
        return self.num_pt_mesh_large if self.refine else self.num_pt_mesh_small

    # -- host part: decode; pose and model points ----------------------------------------------------------------
    def _host_frame(self, index):
        img = Image.open(self.list_rgb[index])
        row = None
        if self._device_jitter:                               # the draws of :126-127 here, their application after the upload
            img, row = augment.defer_jitter(self.trancolor, img)
        elif self.add_noise:
            img = self.trancolor(img)                         # :126-127
        rgb = np.ascontiguousarray(np.array(img)[:, :, :3])                  # :129
        depth = np.ascontiguousarray(np.asarray(Image.open(self.list_depth[index])).astype(np.uint16))
        label = np.ascontiguousarray(np.asarray(Image.open(self.list_label[index])).astype(np.uint16))
        obj = self.list_obj[index]
        if depth.shape != self.udp[obj].image_dims or label.shape != depth.shape or rgb.shape[:2] != depth.shape:
            raise ValueError(f"{self.list_depth[index]}: frame size differs from its object directory's {self.udp[obj].image_dims}")
        return rgb, depth, label, obj, self.meta[obj][self.list_meta[index] + 1], row          # :117: transform indices are one off

    def _draw_add_t(self):
        return np.array([random.uniform(-self.noise_trans, self.noise_trans) for _ in range(3)])      # :144, drawn even when unused

    def _targets(self, obj, gt_trans, add_t):
        """(target, model_points) float32 [500,3] of :140-143,168-210; consumes ``random.sample`` like :170."""
        target_r = Rotation.from_quat(convert_quat(gt_trans[1])).as_matrix()
        target_t = gt_trans[0] * 1000
        target_t[2] = -target_t[2]
        model_points = self.pt[obj] * 10
        n = len(model_points)
        keep = np.ones(n, dtype=bool)
        keep[random.sample(range(n), n - self.num_pt_mesh_small)] = False        # np.delete keeps the survivors in index order: so does this
        model_points = model_points[keep]
        target = np.dot(model_points, (target_r @ Y_180).T)
        target = np.add(target, target_t + add_t * 10000) if self.add_noise else np.add(target, target_t)       # :199-202
        return (torch.from_numpy(target.astype(np.float32) / 10000.), torch.from_numpy(model_points.astype(np.float32) / 10000.))

    @staticmethod
    def _live_box(n_label, rmin, rmax, cmin, cmax):
        return n_label > 0 and rmax - rmin >= MIN_CROP and cmax - cmin >= MIN_CROP

    @staticmethod
    def _count(depth, label, dmax, box):
        rmin, rmax, cmin, cmax = box
        return int(np.count_nonzero((label[rmin:rmax, cmin:cmax] == LABEL_VALUE) & (depth[rmin:rmax, cmin:cmax] != dmax)))

    def _seed(self, index):
        return (self.seed * 1000003 + int(index)) & 0xFFFFFFFF

    def _idx(self, obj, dev):
        oi = self.objlist.index(obj)
        idx = torch.tensor([oi], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        idx._host = [oi]                         # the trainer's losses branch on the index: spare it a device read-back
        return idx

    # -- device part: one statistics launch per frame size, one preparation launch per crop size ---------------------
    def batch(self, indices):
        """The 6-tuples of ``indices`` (same order)."""
        host = [self._host_frame(i) for i in indices]
        dev = self.device
        out = [None] * len(indices)
        by_frame = {}
        for k, h in enumerate(host):
            by_frame.setdefault((h[3], h[1].shape), []).append(k)
        prepared, plan = {}, {}
        for (obj, _), ks in by_frame.items():
            rgb = torch.from_numpy(np.stack([host[k][0] for k in ks])).to(dev)
            if self._device_jitter:
                rgb = pp.color_jitter(rgb, np.stack([host[k][5] for k in ks]), out=rgb)
            depth = torch.from_numpy(np.stack([host[k][1] for k in ks]).view(np.int16)).to(dev)
            label = torch.from_numpy(np.stack([host[k][2] for k in ks]).view(np.int16)).to(dev)
            stats = pp.cad_frame_stats(depth, label, LABEL_VALUE)
            plan[(obj, _)] = (ks, rgb, depth, label, stats, stats.tolist())          # the call's one read-back per frame size: [F][6]
        live = {}
        for key, (ks, rgb, depth, label, stats, rows) in plan.items():
            for f, k in enumerate(ks):
                dmax, n_label, rmin, rmax, cmin, cmax = rows[f]
                box = (rmin, rmax, cmin, cmax)
                live[k] = (f, box) if self._live_box(n_label, *box) and self._count(host[k][1], host[k][2], dmax, box) else None
        add_ts, targets = {}, {}
        for k, h in enumerate(host):                     # index order: Python's global random stream is consumed like :144,170
            add_ts[k] = self._draw_add_t()
            if live[k] is None:
                out[k] = _sentinel()
            else:
                targets[k] = self._targets(h[3], h[4], add_ts[k])
        for key, (ks, rgb, depth, label, stats, rows) in plan.items():
            udp = self.udp[key[0]]
            groups = {}
            for k in ks:
                if live[k] is not None:
                    (rmin, rmax, cmin, cmax) = live[k][1]
                    groups.setdefault((rmax - rmin, cmax - cmin), []).append(k)
            for members in groups.values():
                objs = [(live[k][0], LABEL_VALUE, live[k][1], self._seed(indices[k])) for k in members]
                add_t = np.stack([add_ts[k] for k in members]) if self.add_noise else None
                img, cloud, choose, _ = pp.preprocess_objects_cad(rgb, depth, label, objs, self.num, stats, udp.ray_map_on(dev),
                                                                  udp.proj_mat[2, 2], udp.proj_mat[2, 3], add_t=add_t)
                for j, k in enumerate(members):
                    prepared[k] = (cloud[j], choose[j], img[j])
        for k, h in enumerate(host):
            if out[k] is None:
                cloud, choose, img = prepared[k]
                target, model_points = targets[k]
                out[k] = (cloud, choose, img, target.to(dev), model_points.to(dev), self._idx(h[3], dev))
        return out

    def __getitem__(self, index):
        return self.batch([index])[0]

    # -- the same fetch cut in two for train_utils.Prefetcher(processes=...): worker processes decode, the trainer's process uploads --
    def host_item(self, index):
        """CPU half of ``__getitem__`` (never touches the device: runs in the loader's worker processes): the decoded frame, the frame's
        statistics and box found in numpy (:120,137), the number of mask pixels in the crop and the sampled model / target points, as
        host tensors.  info = [depth_max, n_label, rmin, rmax, cmin, cmax, count, object index]; count 0 marks the sentinel."""
        rgb, depth, label, obj, gt_trans, row = self._host_frame(index)
        lab = label == LABEL_VALUE
        n_label, dmax = int(np.count_nonzero(lab)), int(np.max(depth))
        box = get_bbox(lab) if n_label else (0, 0, 0, 0)
        count = self._count(depth, label, dmax, box) if self._live_box(n_label, *box) else 0
        add_t = self._draw_add_t()
        if count:
            target, model_points = self._targets(obj, gt_trans, add_t)
        else:
            target = model_points = torch.zeros(0, 3)
        item = (torch.from_numpy(rgb), torch.from_numpy(depth.view(np.int16)), torch.from_numpy(label.view(np.int16)),
                torch.tensor([dmax, n_label, *box, count, self.objlist.index(obj)], dtype=torch.int64), target, model_points,
                torch.from_numpy(add_t if self.add_noise else np.zeros(3)))
        return item + (torch.from_numpy(row[None]),) if self._device_jitter else item      # jitter="device": the raw frame and its plan row

    def device_item(self, index, host, choose=None):
        """Device half: uploads + one preparation launch on the current stream, no read-back.  Same 6-tuple as ``__getitem__``.
        ``choose``: the pixel subset as an input instead of the device-side sampling."""
        rgb, depth, label, info, target, model_points, add_t = host[:7]
        dmax, n_label, rmin, rmax, cmin, cmax, count, oi = (int(v) for v in info.tolist())
        if count == 0:
            return _sentinel()
        dev = self.device
        up = lambda t: t.to(dev, non_blocking=True)            # asynchronous when the loader pinned `t`, staged otherwise
        rgb = up(rgb)[None]
        if self._device_jitter:
            rgb = pp.color_jitter(rgb, up(host[7]), out=rgb)
        stats = torch.tensor([[dmax, n_label, rmin, rmax, cmin, cmax]], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        obj = self.objlist[oi]
        udp = self.udp[obj]
        img, cloud, choose, _ = pp.preprocess_objects_cad(rgb, up(depth)[None], up(label)[None],
                                                          [(0, LABEL_VALUE, (rmin, rmax, cmin, cmax), self._seed(index))], self.num, stats,
                                                          udp.ray_map_on(dev), udp.proj_mat[2, 2], udp.proj_mat[2, 3],
                                                          add_t=add_t.reshape(1, 3) if self.add_noise else None, choose_in=choose)
        return (cloud[0], choose[0], img[0], up(target), up(model_points), self._idx(obj, dev))
