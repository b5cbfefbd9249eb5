"""``UnityDepthProjector`` -- mirror of datasets/customCAD/project_unity_depth.py:5-51 of the reference: Unity's 16-bit depth buffer
back to camera-space points through the inverse of the render's projection matrix.

Kept from the reference: the constructor ``UnityDepthProjector(proj_file, image_dims)`` with ``image_dims = (rows, columns)``, the parser
of the tab-separated 4 x 4 matrix (:10-18: the first four lines), the pixel grid ``np.arange(-1, 1, 2 / W)`` (its first W values; the
rows' grid negated, :22-26), the ray map normalised by w and then by z (:35-40), and ``project_depth`` (:42-51):
``z = -P[2,3] / (P[2,2] + (1 - d / 65534))``, point = ray * z, all in float64.

Different by design: no OpenCV / open3d (``project_depth_file`` and the viewer of :53-80 are not built), and ``ray_map_on(device)``
keeps a device copy of the ray map for ``df_preprocess_objects_cad``, which does the work of ``project_depth`` for the chosen pixels only.
"""
from __future__ import annotations

import numpy as np
import torch


def read_proj_mat(proj_file):
    """The 4 x 4 projection matrix of a ``proj_mat.txt``: four lines of tab-separated numbers (:8-18); later lines are not read."""
    proj_mat = np.zeros((4, 4))
    with open(proj_file, "r") as f:
        for i, line in enumerate(f):
            if i == 4:
                break
            for k, elem in enumerate(line.split("\t")):
                proj_mat[i, k] = float(elem.strip())
    return proj_mat


class UnityDepthProjector:
    def __init__(self, proj_file, image_dims):
        self._setup(read_proj_mat(proj_file), image_dims)

    @classmethod
    def from_matrix(cls, proj_mat, image_dims):
        """The projector of a matrix that is already in memory (a renderer's own): what the constructor builds from a
        ``proj_mat.txt`` that holds these sixteen values."""
        self = cls.__new__(cls)
        self._setup(np.array(proj_mat, dtype=np.float64).reshape(4, 4), image_dims)
        return self

    def _setup(self, proj_mat, image_dims):
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        H, W = self.image_dims
        self.proj_mat = proj_mat
        self.inverse_proj_mat = np.linalg.inv(self.proj_mat)                     # :20
        x_range = np.arange(-1, 1, 2.0 / W)[:W]                                 # :22-26 reads the first W (H) values
        y_range = np.arange(-1, 1, 2.0 / H)[:H]
        pixel_map = np.empty((H, W, 4))
        pixel_map[:, :, 0] = x_range[None, :]
        pixel_map[:, :, 1] = -y_range[:, None]                                  # the image's rows run downwards
        pixel_map[:, :, 2] = -1.0                                               # the near plane (:29)
        pixel_map[:, :, 3] = 1.0
        ray_map = np.matmul(self.inverse_proj_mat, pixel_map[..., np.newaxis]).squeeze(-1)      # :35
        ray_map /= ray_map[:, :, 3, np.newaxis]                                 # :37-38
        ray_map /= ray_map[:, :, 2, np.newaxis]
        self.ray_map = np.ascontiguousarray(ray_map[:, :, :3])
        self._device_maps = {}

    def project_depth(self, image):
        """uint16 depth image [rows, columns] -> float64 points [rows, columns, 3] on the host (:42-51)."""
        assert image.shape == self.image_dims
        depth = image.astype(np.float64) / 65534
        depth = 1 - depth
        depth = -self.proj_mat[2, 3] / (self.proj_mat[2, 2] + depth)
        world_ray_map = np.copy(self.ray_map)
        world_ray_map *= depth[..., np.newaxis]
        return world_ray_map

    def ray_map_on(self, device):
        """The ray map as a float64 [rows, columns, 3] tensor on `device`, uploaded once per device."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device_maps.get(device)
        if t is None:
            t = self._device_maps[device] = torch.from_numpy(self.ray_map).to(device)
        return t

    def __getstate__(self):                     # the loader's worker processes get the host part only
        state = dict(self.__dict__)
        state["_device_maps"] = {}
        return state
