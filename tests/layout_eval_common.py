"""Shared by tools/gen_layout_eval_golden.py (which drives the reference) and tests/test_layout_eval_*.py: the seeded inputs of
tests/golden/layout_eval.npz, the stub generator of its end-to-end case and the detector file written from seeded weights.  Everything is a
pure function of names and seeds (oracle/seeded.py), so both sides rebuild the same bits without storing them."""
import os
import shutil

import torch

from oracle import seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_ZIP = os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip')
DATASET_NAME = 'ads_banner_collection'      # 13 labels + label_idx_replace in the reference (metric_layoutnet.py:28, metric_utils_layout.py:239)
WEIGHT_SEED = 11
N_LAYOUTS, N_SLOTS, NUM_LABEL = 1024, 9, 13


def seeded_layouts(tag, n=N_LAYOUTS, N=N_SLOTS, num_label=NUM_LABEL, seed=3):
    """-> bbox [n, N, 4] float32 (xywh), label [n, N] int64 in [0, num_label), padding_mask [n, N] bool: item i has 1 + i % N valid elements."""
    xy = seeded.uniform(f'layout_eval.{tag}.xy', (n, N, 2), seed, 0.2, 0.8)
    wh = seeded.uniform(f'layout_eval.{tag}.wh', (n, N, 2), seed, 0.05, 0.4)
    label = seeded.randint(f'layout_eval.{tag}.cls', (n, N), num_label, seed)
    valid = torch.arange(N)[None, :] < (1 + torch.arange(n) % N)[:, None]
    return torch.cat([xy, wh], -1), label, ~valid


def seeded_layoutnet_state(module, seed=WEIGHT_SEED):
    return seeded.seeded_state_dict(module, seed)


class StubGenerator(torch.nn.Module):
    """A generator that is a fixed smooth function of (bbox_real, bbox_class) and ignores z: the end-to-end case does not depend on a device RNG.
    Takes the keyword arguments both the reference's and this package's metric passes call G with."""

    def __init__(self):
        super().__init__()
        self.z_dim, self.c_dim = 4, 0
        self.register_buffer('phase', torch.tensor([0.7, 0.4]))

    def forward(self, z, bbox_class, bbox_real, bbox_text=None, bbox_patch=None, padding_mask=None, background=None, c=None, **_kwargs):
        t = bbox_class.to(torch.float32).unsqueeze(-1)
        xy = 0.5 + 0.35 * torch.sin(3.0 * bbox_real[..., :2] + self.phase[0] * t)
        wh = 0.05 + 0.15 * (1.0 + torch.cos(10.0 * bbox_real[..., 2:] + self.phase[1] * t))
        return torch.cat([xy, wh], dim=-1)


def stage_dataset(tmp):
    """Copy the tiny archive to <tmp>/ads_banner_collection/zip/train.zip: the reference derives the detector file AND its label count from the third
    path component from the end (layout_frechet_inception_distance.py:21); under tests/golden/ that would be 'tests', 5 labels."""
    d = os.path.join(str(tmp), DATASET_NAME, 'zip')
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, 'train.zip')
    shutil.copyfile(TINY_ZIP, path)
    return path


def write_detector(tmp, layoutnet_cls, dataset_name=DATASET_NAME, num_label=NUM_LABEL):
    """<tmp>/pretrained/layoutnet_<dataset>.pth.tar from the seeded weights; the metric opens it relative to the working directory."""
    os.makedirs(os.path.join(str(tmp), 'pretrained'), exist_ok=True)
    path = os.path.join(str(tmp), 'pretrained', f'layoutnet_{dataset_name}.pth.tar')
    torch.save(seeded_layoutnet_state(layoutnet_cls(num_label)), path)
    return path
