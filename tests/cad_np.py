"""The customCAD loader restated in numpy: datasets/customCAD/dataset.py:109-210 and project_unity_depth.py:20-51 of the reference, on
decoded arrays.  TEST INFRASTRUCTURE: the specification densefusion_amd/csrc/cad.hip and densefusion_amd/datasets/customCAD are held to.

The reference itself cannot be imported here (open3d, cv2 and torchvision are absent), so no reference-generated golden exists for this
loader: it is pinned by this restatement only.  Every line keeps the reference's operand types and order of operations; the one deliberate
difference is the random pixel subset (np.random.shuffle at :151-155), replaced by the key rule build and checker share
(oracle.preprocess_ref.mix32: the N mask pixels with the smallest keys, ties to the lower index, in index order).
"""
import random

import numpy as np
import numpy.ma as ma
from scipy.spatial.transform import Rotation as R

from oracle.preprocess_ref import mix32

GRAY = np.array([130, 130, 130])                         # dataset.py:97
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)[:, None, None]
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)[:, None, None]


def ray_map(proj_mat, image_dims):
    """project_unity_depth.py:20-40, loops and all."""
    inverse_proj_mat = np.linalg.inv(proj_mat)
    x_range = np.arange(-1, 1, 2. / image_dims[1])
    y_range = np.arange(-1, 1, 2. / image_dims[0])
    pixel_map = np.array([[[x_range[i], -y_range[k]] for i in range(image_dims[1])] for k in range(image_dims[0])])
    z_map = np.ones((pixel_map.shape[0], pixel_map.shape[1], 1)) * -1
    w_map = np.ones((pixel_map.shape[0], pixel_map.shape[1], 1))
    pixel_map = np.concatenate((pixel_map, z_map, w_map), axis=2)
    pixel_map = pixel_map[..., np.newaxis]
    rays = np.matmul(inverse_proj_mat, pixel_map).squeeze()
    rays /= rays[:, :, 3, np.newaxis]
    rays /= rays[:, :, 2, np.newaxis]
    return rays[:, :, :3]


def project_depth(proj_mat, rays, image):
    """project_unity_depth.py:42-51."""
    depth = image.astype(np.float64) / 65534
    depth = 1 - depth
    depth = -proj_mat[2, 3] / (proj_mat[2, 2] + depth)
    world_ray_map = np.copy(rays)
    world_ray_map *= depth[..., np.newaxis]
    return world_ray_map


def frame_stats(depth, label, label_value=65535):
    """{depth_max, n_label, rmin, rmax, cmin, cmax}: np.max(depth) (:120) and get_bbox (:247-249, inclusive); zero box without the label."""
    a = np.where(label == label_value)
    if len(a[0]) == 0:
        return [int(np.max(depth)), 0, 0, 0, 0, 0]
    return [int(np.max(depth)), len(a[0]), int(np.min(a[0])), int(np.max(a[0])), int(np.min(a[1])), int(np.max(a[1]))]


def convert_quat(Q):
    return np.array([-Q[0], -Q[1], Q[2], Q[3]])              # :225-227


def choose_rule(choose, num, seed):
    """:151-157 with the shared key rule in place of np.random.shuffle."""
    if len(choose) > num:
        keys = mix32(seed, choose)
        order = np.lexsort((choose, keys))[:num]             # smallest keys, ties -> lower index
        return np.sort(choose[order])
    return np.pad(choose, (0, num - len(choose)), 'wrap')


def prepare(rgb, depth, label, bbox, num, seed, proj_mat, rays, add_t=None, given=None):
    """The pixel half of __getitem__ (:120-138,146-166,205-207) for one crop [rmin:rmax, cmin:cmax]: img [3,H,W] f32, cloud [num,3] f32,
    choose [1,num] i64, count.  rgb: the (already jittered) [IH,IW,>=3] uint8 frame; add_t: the noise of :165-166 or None; given: the
    chosen indices as an input.  count == 0 -> (None, None, None, 0), the sentinel of :147-149."""
    rmin, rmax, cmin, cmax = bbox
    mask_depth = ma.getmaskarray(ma.masked_not_equal(depth, np.max(depth)))          # :120
    mask_label = ma.getmaskarray(ma.masked_equal(label, 65535))                      # :123
    mask = mask_label * mask_depth
    img = np.array(rgb)[:, :, :3]                                                    # :129
    img[depth == np.max(depth)] = GRAY                                               # :132
    img = np.transpose(img, (2, 0, 1))
    img_masked = img[:, rmin:rmax, cmin:cmax]                                        # :138
    choose = mask[rmin:rmax, cmin:cmax].flatten().nonzero()[0]                       # :146
    count = len(choose)
    if count == 0:
        return None, None, None, 0
    choose = choose_rule(choose, num, seed) if given is None else np.asarray(given).reshape(-1)
    depth_projected = project_depth(proj_mat, rays, depth)[rmin:rmax, cmin:cmax].reshape((-1, 3))      # :159
    cloud = depth_projected[choose].astype(np.float32)                               # :161
    choose = np.array([choose])
    if add_t is not None:
        cloud = np.add(cloud, add_t)                                                 # :165-166 (float32 + float64 -> float64)
    img_norm = (img_masked.astype(np.float32) - MEAN) / STD                          # :207, transforms.Normalize on a float32 tensor
    return img_norm, cloud.astype(np.float32) / 10000., choose.astype(np.int64), count           # :205-206


def targets(pt, gt_trans, num_pt_mesh, add_noise, add_t):
    """The pose half (:140-143,168-210): (target, model_points) float32; consumes random.sample like :170."""
    target_r_quat = convert_quat(gt_trans[1])
    target_r = R.from_quat(target_r_quat).as_matrix()                                # :229-244
    target_t = gt_trans[0] * 1000
    target_t[2] = -target_t[2]
    model_points = pt * 10
    dellist = [j for j in range(0, len(model_points))]
    dellist = random.sample(dellist, len(model_points) - num_pt_mesh)
    model_points = np.delete(model_points, dellist, axis=0)
    y_180 = np.zeros((3, 3))
    y_180[0, 0] = -1
    y_180[1, 1] = 1
    y_180[2, 2] = -1
    target = np.copy(model_points)
    target = np.dot(target, (target_r @ y_180).T)
    if add_noise:
        target = np.add(target, target_t + add_t * 10000)
    else:
        target = np.add(target, target_t)
    return target.astype(np.float32) / 10000., model_points.astype(np.float32) / 10000.


def get_item(rgb, depth, label, gt_trans, pt, num, seed, proj_mat, rays, add_noise=False, noise_trans=0.0, num_pt_mesh=500, min_crop=8):
    """One item in the reference's order (the jitter's draws come before this call): box (:137), add_t (:144), the pixel half, then the pose
    half.  Returns None for the sentinel, else (cloud, choose, img, target, model_points, box).  A box under `min_crop` rows or columns is a
    sentinel too (the build's documented limit, not the reference's)."""
    st = frame_stats(depth, label)
    box = tuple(st[2:6])
    add_t = np.array([random.uniform(-noise_trans, noise_trans) for i in range(3)])        # :144
    if st[1] == 0 or box[1] - box[0] < min_crop or box[3] - box[2] < min_crop:
        return None
    img, cloud, choose, count = prepare(rgb, depth, label, box, num, seed, proj_mat, rays, add_t if add_noise else None)
    if count == 0:
        return None
    target, model_points = targets(pt, gt_trans, num_pt_mesh, add_noise, add_t)
    return cloud, choose, img, target, model_points, box
