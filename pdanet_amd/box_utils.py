"""Box geometry the IA-SSD head needs (pcdet/utils/box_utils.py:28-53,145-158 and
pcdet/utils/common_utils.py rotate_points_along_z), torch only, and the host conversion of KITTI annotations to lidar boxes
(box_utils.py:92-108), numpy."""
import numpy as np
import torch


def rotate_points_along_z(points, angle):
    """common_utils.rotate_points_along_z: points (B, N, 3+C), angle (B) -> rotated about z (x towards y), in the
    points' type (float32 in the reference)."""
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).to(points.dtype)
    out = torch.matmul(points[:, :, 0:3], rot)
    return torch.cat((out, points[:, :, 3:]), dim=-1)


_CONST = {}


def const_tensor(like, key, values):
    """Small constant on `like`'s device/dtype, uploaded once (a per-call new_tensor(list) on the GPU is
    a pageable host-to-device copy, i.e. a host synchronisation in the middle of the step)."""
    k = (key, like.device, like.dtype)
    if k not in _CONST:
        _CONST[k] = torch.tensor(values, device=like.device, dtype=like.dtype)
    return _CONST[k]


_CORNER_TEMPLATE = ((1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1))


def boxes_to_corners_3d(boxes3d):
    """box_utils.py:28-53: (N, 7) [x, y, z, dx, dy, dz, heading] -> (N, 8, 3) corners."""
    template = const_tensor(boxes3d, 'corners', _CORNER_TEMPLATE) / 2
    corners = boxes3d[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    corners = rotate_points_along_z(corners.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    return corners + boxes3d[:, None, 0:3]


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """box_utils.py:145-158."""
    large = boxes3d.clone()
    for k, w in enumerate(extra_width):      # python scalars travel as kernel arguments
        large[:, 3 + k] += float(w)
    return large


def rect_to_lidar(pts_rect, calib):
    """Calibration.rect_to_lidar (calibration_kitti.py:50-63), numpy on the host: (N, 3) rect camera -> lidar.  calib: an
    object with R0 (3, 3) and V2C (3, 4), or a dict with 'R0' and 'Tr_velo2cam'."""
    r0 = calib['R0'] if isinstance(calib, dict) else calib.R0
    v2c = calib['Tr_velo2cam'] if isinstance(calib, dict) else calib.V2C
    hom = np.hstack((pts_rect, np.ones((pts_rect.shape[0], 1), dtype=np.float32)))
    r0_ext = np.hstack((r0, np.zeros((3, 1), dtype=np.float32)))
    r0_ext = np.vstack((r0_ext, np.zeros((1, 4), dtype=np.float32)))
    r0_ext[3, 3] = 1
    v2c_ext = np.vstack((v2c, np.zeros((1, 4), dtype=np.float32)))
    v2c_ext[3, 3] = 1
    return np.dot(hom, np.linalg.inv(np.dot(r0_ext, v2c_ext).T))[:, 0:3]


def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """box_utils.py:92-108, numpy on the host (a frame holds a few dozen boxes and the transform needs a 4x4 inverse):
    (N, 7) [x, y, z, l, h, w, r] in rect camera coordinates -> [x, y, z, dx, dy, dz, heading], (x, y, z) the box centre."""
    cam = np.array(boxes3d_camera, copy=True)
    xyz_camera, r = cam[:, 0:3], cam[:, 6:7]
    l, h, w = cam[:, 3:4], cam[:, 4:5], cam[:, 5:6]
    xyz_lidar = rect_to_lidar(xyz_camera, calib)
    xyz_lidar[:, 2] += h[:, 0] / 2
    return np.concatenate([xyz_lidar, l, w, h, -(r + np.pi / 2)], axis=-1)
