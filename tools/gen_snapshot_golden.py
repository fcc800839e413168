"""Generates tests/golden/snapshot.npz by driving the REFERENCE's own convert_layout_to_image (util.py:85-112) on the CPU: data only.

Run where the reference tree is available:  python tools/gen_snapshot_golden.py [path to the reference]
The reference's util.py imports torchvision and skimage at the top; neither is needed by convert_layout_to_image (pure PIL), so empty stand-in
modules are put in sys.modules before the import.  Stored, per page-size case: fp32 boxes (handed to the reference as fp32 torch tensors, so
its `b[2] * b[3]` and corner arithmetic run in fp32 as they do in save_image), validity, labels, the palette, the reference's cell for every
layout, the same boxes drawn over a random uint8 page by the same Pillow calls (the reference's function with `Image.new` replaced by the page:
the over-background kind), and make_grid(padding=2) RESTATED (tests/snapshot_common.py; torchvision is not installed) for B = 5, nrow = 3 and for
B = 1.  Every box is at least 3 page pixels wide and high; thinner boxes are this package's own definition and are not pinned by Pillow."""
import os
import sys
import types

import numpy as np
import PIL.Image
import PIL.ImageDraw
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (the one place that names where the reference tree lies)
import snapshot_common as SC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else _DEFAULT_REF
OUT = os.path.join(ROOT, 'tests', 'golden', 'snapshot.npz')
PALETTE = [(228, 26, 28), (55, 126, 184), (77, 175, 74), (152, 78, 163), (255, 127, 0)]
CASES = [('land', 50, 30, 16), ('port', 30, 50, 16), ('up', 24, 24, 32), ('same', 16, 16, 16), ('round', 37, 23, 16)]


def _reference_util():
    sys.path.insert(0, REF)
    for name in ('torchvision', 'torchvision.utils', 'torchvision.transforms', 'skimage', 'skimage.transform'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].utils = sys.modules['torchvision.utils']
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.modules['skimage'].transform = sys.modules['skimage.transform']
    import util
    return util


def ref_cell(util, bbox, valid, labels, colors, W, H, S, page=None):
    """The reference's call chain of save_image for one sample: boxes[mask], labels[mask], convert_layout_to_image."""
    m = torch.from_numpy(valid.astype(bool))
    boxes = torch.from_numpy(bbox)[m]
    labs = torch.from_numpy(labels.astype(np.int64))[m]
    if page is None:
        img = util.convert_layout_to_image(boxes, labs, colors, W, H, S)
    else:                                        # the same Pillow calls on a canvas that starts as the page instead of white
        real = util.Image            # util's name `Image` only: PIL.Image itself stays as it is

        def new(mode, size, color=None):
            return PIL.Image.fromarray(page.copy(), 'RGB') if tuple(size) == (W, H) else real.new(mode, size, color=color)
        util.Image = types.SimpleNamespace(new=new, BILINEAR=real.BILINEAR)
        try:
            img = util.convert_layout_to_image(boxes, labs, colors, W, H, S)
        finally:
            util.Image = real
    out = np.array(img)
    assert out.shape == (S, S, 3) and out.dtype == np.uint8
    return out


def snap(v, size, lo):
    """Round a normalised extent so that the box is at least `lo` pixels at `size`."""
    return max(v, (lo + 0.6) / size)


def layouts_for(W, H, rng):
    """Five layouts of nine slots: 0, 1 and 9 valid elements, equal areas (tie order), boxes partly and wholly off the page."""
    bbox = np.zeros((5, 9, 4), np.float32)
    valid = np.zeros((5, 9), np.uint8)
    labels = rng.randint(0, len(PALETTE), size=(5, 9)).astype(np.int64)

    def box(xc, yc, w, h):
        return [xc, yc, snap(w, W, 3), snap(h, H, 3)]
    # 0: nothing valid (the slots still hold boxes: they must not be drawn)
    bbox[0] = [box(*rng.uniform(0.2, 0.8, 2), *rng.uniform(0.1, 0.5, 2)) for _ in range(9)]
    # 1: one element
    bbox[1, 0] = box(0.45, 0.55, 0.5, 0.4); valid[1, 0] = 1
    # 2: nine elements, overlapping
    bbox[2] = [box(*rng.uniform(0.15, 0.85, 2), *rng.uniform(0.1, 0.6, 2)) for _ in range(9)]; valid[2] = 1
    # 3: equal areas in different slots (w * h identical bit for bit: the same pair of factors), overlapping so that the order shows
    w, h = np.float32(snap(0.4, W, 3)), np.float32(snap(0.5, H, 3))
    bbox[3, :4] = [[0.4, 0.4, w, h], [0.5, 0.5, w, h], [0.6, 0.45, w, h], [0.45, 0.6, w, h]]; valid[3, :4] = 1
    bbox[3, 4] = box(0.5, 0.5, 0.2, 0.2); valid[3, 4] = 1
    # 4: partly and wholly off the page, with a gap in the valid slots
    bbox[4, :6] = [box(0.02, 0.5, 0.3, 0.5), box(0.98, 0.1, 0.4, 0.4), box(0.5, 1.05, 0.6, 0.3), box(1.6, 0.5, 0.3, 0.3), box(-0.7, -0.7, 0.3, 0.3),
                   box(0.5, 0.5, 1.4, 1.3)]
    valid[4, :6] = [1, 1, 1, 1, 1, 1]; valid[4, 1] = 0; valid[4, 7] = 1; bbox[4, 7] = box(0.6, 0.3, 0.25, 0.3)
    return bbox, valid, labels


def main():
    util = _reference_util()
    rng = np.random.RandomState(20240)
    out = {'palette': np.asarray(PALETTE, np.uint8), 'cases': np.asarray([c[0] for c in CASES]), 'case_whs': np.asarray([c[1:] for c in CASES], np.int32)}
    for name, W, H, S in CASES:
        bbox, valid, labels = layouts_for(W, H, rng)
        pages = rng.randint(0, 256, size=(5, H, W, 3)).astype(np.uint8)
        white = np.stack([ref_cell(util, bbox[k], valid[k], labels[k], PALETTE, W, H, S) for k in range(5)])
        over = np.stack([ref_cell(util, bbox[k], valid[k], labels[k], PALETTE, W, H, S, pages[k]) for k in range(5)])
        shared = np.stack([ref_cell(util, bbox[k], valid[k], labels[k], PALETTE, W, H, S, pages[0]) for k in (2, 3, 4)])   # three cells, ONE page
        out.update({f'{name}_bbox': bbox, f'{name}_valid': valid, f'{name}_labels': labels.astype(np.uint8), f'{name}_pages': pages,
                    f'{name}_white': white, f'{name}_over': over, f'{name}_shared': shared})
        if name == 'land':
            out['grid_b5_nrow3'] = SC.make_grid(white, nrow=3)
            out['grid_b5_default'] = SC.make_grid(white)
            out['grid_b1'] = SC.make_grid(white[2:3])
    # the three layouts of tests/golden/dataset_tiny.zip at their page size, canvas 128, with the dataset's own palette
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset
    ds = LayoutDataset(os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip'), mode='device')
    colors = [tuple(int(v) for v in c) for c in ds.colors]
    items = [ds[i][0] for i in range(len(ds))]
    tb = np.stack([it['bboxes'] for it in items]).astype(np.float32)
    tv = np.stack([it['mask'] for it in items]).astype(np.uint8)
    tl = np.stack([it['labels'] for it in items]).astype(np.int64)
    twh = np.asarray([[it['W_page'], it['H_page']] for it in items], np.int32)
    for k, it in enumerate(items):
        ph, pw = it['background'].shape[:2]      # the archive's decoded pages are smaller than attr.width x attr.height: drawn over at their own size
        px = tb[k][tv[k] != 0]
        assert (px[:, 2] * min(pw, twh[k, 0]) >= 3.5).all() and (px[:, 3] * min(ph, twh[k, 1]) >= 3.5).all(), 'a dataset box is thinner than 3 pixels'
    out.update(tiny_palette=np.asarray(colors, np.uint8), tiny_bbox=tb, tiny_valid=tv, tiny_labels=tl.astype(np.uint8), tiny_wh=twh,
               tiny_white=np.stack([ref_cell(util, tb[k], tv[k], tl[k], colors, int(twh[k, 0]), int(twh[k, 1]), 128) for k in range(len(items))]),
               tiny_pages=np.stack([it['background'] for it in items]),
               tiny_over=np.stack([ref_cell(util, tb[k], tv[k], tl[k], colors, it['background'].shape[1], it['background'].shape[0], 128, np.ascontiguousarray(it['background']))
                                   for k, it in enumerate(items)]))
    ds.close()
    # every fixture box is at least 3 page pixels wide and high
    for name, W, H, S in CASES:
        b = out[f'{name}_bbox'][out[f'{name}_valid'] != 0]
        assert (b[:, 2] * W >= 3.5).all() and (b[:, 3] * H >= 3.5).all(), name
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
