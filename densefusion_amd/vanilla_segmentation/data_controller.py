"""``SegDataset`` -- the training / test set of the SegNet mask network, mirroring the reference's
vanilla_segmentation/data_controller.py:17-104 over a YCB-Video tree.

Each item is a RANDOM frame of the list (the index passed in is ignored, as in the reference): its colour image, ColorJitter(0.2,
0.2, 0.2, 0.05) when ``use_noise`` (datasets/augment.py, the restatement of torchvision's); a ``data_syn/`` frame is brightened
(1.5) and blurred (GaussianBlur 0.8) with PIL, jittered, given N(0, 5) noise and composited onto a random real frame and its label
where its own label is 0; with ``use_noise`` one of the four joint flips (left-right, up-down, both, none) moves image and label
together.  ImageNet normalisation is applied to the 0..255 values: the reference does not divide by 255, and neither does this.
Returns ``(rgb float32 [3,480,640], target int64 [480,640])``; ``len()`` is ``length``.  Host-only (loader worker processes).
"""
from __future__ import annotations

import random

import numpy as np
import torch
import torch.utils.data as data
from PIL import Image, ImageEnhance, ImageFilter

from ..datasets.augment import ColorJitter

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


class SegDataset(data.Dataset):
    def __init__(self, root_dir, txtlist, use_noise, length):
        self.path, self.real_path = [], []
        self.use_noise = use_noise
        self.root = root_dir
        with open(txtlist) as f:
            for line in f:
                line = line.rstrip("\n")
                if not line:
                    continue
                self.path.append(line)
                if line[:5] == "data/":
                    self.real_path.append(line)
        self.length = length
        self.data_len = len(self.path)
        self.back_len = len(self.real_path)
        self.trancolor = ColorJitter(0.2, 0.2, 0.2, 0.05)

    def _open(self, name, kind):
        return Image.open(f"{self.root}/{name}-{kind}.png")

    def __getitem__(self, idx):
        # the reference draws from [0, len - 10] (data_controller.py:45); a list shorter than 10 frames draws from its first frame
        index = random.randint(0, max(0, self.data_len - 10))
        name = self.path[index]
        label = np.array(self._open(name, "label"))
        rgb_img = self._open(name, "color").convert("RGB")
        rgb = np.array(self.trancolor(rgb_img) if self.use_noise else rgb_img)

        if name[:8] == "data_syn":
            rgb = ImageEnhance.Brightness(rgb_img).enhance(1.5).filter(ImageFilter.GaussianBlur(radius=0.8))
            rgb = np.array(self.trancolor(rgb))
            seed = random.randint(0, max(0, self.back_len - 10))
            back = np.array(self.trancolor(self._open(self.real_path[seed], "color").convert("RGB")))
            back_label = np.array(self._open(self.real_path[seed], "label"))
            mask = label == 0
            back = np.transpose(back, (2, 0, 1))
            rgb = np.transpose(rgb, (2, 0, 1))
            rgb = rgb + np.random.normal(loc=0.0, scale=5.0, size=rgb.shape)
            rgb = back * mask + rgb
            label = back_label * mask + label
            rgb = np.transpose(rgb, (1, 2, 0))

        if self.use_noise:
            choice = random.randint(0, 3)
            if choice == 0:
                rgb, label = np.fliplr(rgb), np.fliplr(label)
            elif choice == 1:
                rgb, label = np.flipud(rgb), np.flipud(label)
            elif choice == 2:
                rgb, label = np.flipud(np.fliplr(rgb)), np.flipud(np.fliplr(label))

        rgb = np.transpose(rgb, (2, 0, 1)).astype(np.float32)
        rgb = (rgb - MEAN[:, None, None]) / STD[:, None, None]
        return torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(label).astype(np.int64))

    def __len__(self):
        return self.length
