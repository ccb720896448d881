"""Dataset configs as the hot path consumes them (mirror of reference
datasets/sunrgbd.py:54-165 and datasets/scannet.py:36-169): class / angle-bin
counts, the 640-d CLIP embedding length, angle <-> (class, residual) coding and
box-parameter -> corner conversion.  Loaders, augmentation and file paths are
out of scope."""
import numpy as np
import torch

from .box_util import (flip_axis_to_camera_np, flip_axis_to_camera_tensor, get_3d_box_batch_np,
                       get_3d_box_batch_tensor)


class _Base:
    clip_embed_length = 640
    max_num_obj = 64

    def box_parametrization_to_corners(self, box_center_unnorm, box_size, box_angle):
        return get_3d_box_batch_tensor(box_size, box_angle,
                                       flip_axis_to_camera_tensor(box_center_unnorm))

    def box_parametrization_to_corners_np(self, box_center_unnorm, box_size, box_angle):
        return get_3d_box_batch_np(box_size, box_angle, flip_axis_to_camera_np(box_center_unnorm))


class SunrgbdDatasetConfig(_Base):
    def __init__(self):
        self.num_semcls = 20
        self.num_angle_bin = 12
        self.type2class = {n: i for i, n in enumerate(
            ["bathtub", "bed", "bookshelf", "box", "chair", "counter", "desk", "door", "dresser",
             "lamp", "night_stand", "pillow", "sink", "sofa", "table", "tv", "toilet"])}
        self.class2type = {v: k for k, v in self.type2class.items()}
        self.support_class = np.arange(10, 20)

    def angle2class(self, angle):
        """continuous angle -> (bin, residual); bin centres at k*2pi/N (sunrgbd.py:102-120)"""
        n = self.num_angle_bin
        angle = angle % (2 * np.pi)
        per = 2 * np.pi / float(n)
        shifted = (angle + per / 2) % (2 * np.pi)
        cls = int(shifted / per)
        return cls, shifted - (cls * per + per / 2)

    def class2angle_batch(self, pred_cls, residual, to_label_format=True):
        per = 2 * np.pi / float(self.num_angle_bin)
        angle = pred_cls * per + residual
        if to_label_format:
            mask = angle > np.pi
            angle[mask] = angle[mask] - 2 * np.pi
        return angle


class ScannetDatasetConfig(_Base):
    def __init__(self):
        self.num_semcls = 18
        self.num_angle_bin = 1
        names = ["cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf",
                 "picture", "counter", "desk", "curtain", "refrigerator", "shower curtain",
                 "toilet", "sink", "bathtub", "garbagebin"]
        self.type2class = {n: i for i, n in enumerate(names)}
        self.class2type = {v: k for k, v in self.type2class.items()}
        self.max_num_obj = 64
        # the 18 detection classes' NYU40 ids, in class order (scannet.py:64-69)
        self.nyu40ids = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
        self.nyu40id2class = {i: c for c, i in enumerate(list(self.nyu40ids))}

    def angle2class(self, angle):
        raise ValueError("ScanNet does not have rotated bounding boxes.")

    @staticmethod
    def rotate_aligned_boxes(input_boxes, rot_mat):
        """(K, 6) axis-aligned boxes (centre, lengths) rotated about z and re-aligned: the
        rotated centres, and per box twice the largest x / y of its four rotated half-extent
        corners (scannet.py:148-169, with the reference's numpy dtype rules); z length kept"""
        ctr, length = input_boxes[:, 0:3], input_boxes[:, 3:6]
        rt = np.transpose(rot_mat)
        new_ctr = np.dot(ctr, rt)
        hx, hy = length[:, 0] / 2.0, length[:, 1] / 2.0
        ext_x = np.zeros((hx.shape[0], 4))
        ext_y = np.zeros((hx.shape[0], 4))
        for q, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            corner = np.zeros((hx.shape[0], 3))
            corner[:, 0] = sx * hx
            corner[:, 1] = sy * hy
            corner = np.dot(corner, rt)
            ext_x[:, q] = corner[:, 0]
            ext_y[:, q] = corner[:, 1]
        new_len = np.stack((2.0 * np.max(ext_x, 1), 2.0 * np.max(ext_y, 1), length[:, 2]), axis=1)
        return np.concatenate([new_ctr, new_len], axis=1)

    def class2anglebatch_tensor(self, pred_cls, residual, to_label_format=True):
        return torch.zeros(pred_cls.shape[:2], dtype=torch.float32, device=pred_cls.device)


CONFIGS = {"sunrgbd": SunrgbdDatasetConfig, "scannet": ScannetDatasetConfig}
