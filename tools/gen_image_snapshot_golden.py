"""Generates tests/golden/image_snapshot.npz by driving the REFERENCE's own convert_layout_to_real_image and
convert_layout_to_real_image_with_background (util.py:144-204, 234-295) on the CPU: data only.

Run where the reference tree is available:  python tools/gen_image_snapshot_golden.py [path to the reference]

What the fixture pins, and what it does not.  The reference's util.py imports torchvision and skimage at the top.  torchvision is stubbed (not used by the
two functions).  skimage is NOT installed where this tool runs, so `skimage.transform.resize` is a STAND-IN written here on scipy.ndimage, in float64:
gaussian_filter(sigma = max(0, (in / out - 1) / 2), mode='mirror'), zoom(order=1, mode='mirror', grid_mode=True), clipped to the input's range -- the calls
skimage's resize makes for anti_aliasing=True on a float image.  The fixture therefore pins the reference's CODE PATH (crop, de-normalise, corner rounding,
draw order, clipping, paste, `(img * 255).astype('ubyte')`, PIL resize, expand2square) over a restated library call; it is not a captured skimage output.
The stand-in is checked against the closed form of tests/image_snapshot_common.py (resize_f64) on every call, to 1e-12.

Inputs go in as the dataset hands them to the reference: normalised fp32 CHW patch canvases and backgrounds, fp32 box tensors.  The same run is stored a
second time with float64 inputs ((u8 / 255 - mean) / std in double: the de-normalised value is u8 / 255 to double rounding); the share of cell pixels
on which the two runs differ is the fixture's own noise floor and is stored per cell.  Elements on which the reference's lines cannot run are left out of
its call, as the package's rule leaves them undrawn: a crop window that leaves the patch canvas (the reference's slice would wrap or come out short).

Asserted here: every fake corner * W|H is at least 1e-3 from a half-integer and every real extent * W|H at least 1e-3 from an integer (the reference's
result then does not depend on numpy's scalar promotion); on the cells where no resize keeps a size on an axis the noise floor is <= 0.25 % of pixels."""
import math
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndi
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (the one place that names where the reference tree lies)
import image_snapshot_common as ISC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else _DEFAULT_REF
OUT = os.path.join(ROOT, 'tests', 'golden', 'image_snapshot.npz')
CASES = [('land', 50, 30, 40), ('port', 30, 50, 32), ('round', 37, 23, 24)]
TINY_CANVAS = 64
N = 9


def resize_stand_in(image, output_shape, anti_aliasing=False, **kwargs):
    """skimage.transform.resize for a float image with its defaults (order 1, mode 'reflect' = ndimage 'mirror', clip) on scipy.ndimage, float64."""
    assert anti_aliasing and not kwargs
    im = np.asarray(image, np.float64)
    shape = tuple(int(v) for v in output_shape) + im.shape[len(output_shape):]
    factors = np.divide(im.shape, shape)
    sigma = np.maximum(0, (factors - 1) / 2)
    filtered = ndi.gaussian_filter(im, sigma, mode='mirror') if np.any(sigma > 0) else im
    out = ndi.zoom(filtered, [1.0 / f for f in factors], order=1, mode='mirror', grid_mode=True)
    assert out.shape == shape, (out.shape, shape)
    out = np.clip(out, im.min(), im.max())
    assert np.abs(out - ISC.resize_f64(im, shape[0], shape[1])).max() < 1e-12
    return out


def _reference_util():
    sys.path.insert(0, REF)
    for name in ('torchvision', 'torchvision.utils', 'torchvision.transforms', 'skimage', 'skimage.transform'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].utils = sys.modules['torchvision.utils']
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.modules['skimage'].transform = sys.modules['skimage.transform']
    sys.modules['skimage.transform'].resize = resize_stand_in
    import util
    return util


def normalised_chw(u8, dtype):
    """What the dataset hands out for a uint8 [h, w, 3] image (training/dataset_layoutganpp.py:305-315, 329-340)."""
    a = np.asarray(u8)
    return torch.from_numpy(np.ascontiguousarray(((a.astype(dtype) / dtype(255.0) - ISC.RGB_MEAN.astype(dtype)) / ISC.RGB_STD.astype(dtype)).transpose(2, 0, 1)))


def ref_cell(util, bbox_fake, bbox_real, valid, canvases, W, H, S, background, dtype):
    """The reference's call chain of save_real_image[_with_background] for one sample."""
    m = torch.from_numpy(np.asarray(valid).astype(bool))
    fake, real = torch.from_numpy(bbox_fake)[m], torch.from_numpy(bbox_real)[m]
    images = [normalised_chw(canvases[i], dtype) for i in range(len(valid)) if valid[i]]
    if background is None:
        img = util.convert_layout_to_real_image(fake, real, images, W, H, S)
    else:
        img = util.convert_layout_to_real_image_with_background(fake, real, images, normalised_chw(background, dtype), W, H, S)
    out = np.array(img)
    assert out.shape == (S, S, 3) and out.dtype == np.uint8
    return out


def texture(rng, h, w):
    """A smooth random texture, uint8 [h, w, 3]: a few random sinusoids per channel, not a flat field."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx = rng.uniform(-0.9, 0.9, 2)
            out[:, :, c] += rng.uniform(0.3, 1.0) * np.sin(fy * y + fx * x + rng.uniform(0, 6.28))
    out = (out - out.min()) / (out.max() - out.min())
    return np.clip(np.rint(out * 255.0), 0, 255).astype(np.uint8)


def fake_box(W, H, x1, y1, x2, y2):
    """A box whose corners land 0.2 past the integer rectangle: rounding is far from a tie."""
    return [((x1 + x2) / 2.0 + 0.2) / W, ((y1 + y2) / 2.0 + 0.2) / H, (x2 - x1) / float(W), (y2 - y1) / float(H)]


def real_box(W, H, cw, ch):
    """A real box whose crop is cw x ch: the extent lands 0.5 past the integer."""
    return [0.5, 0.5, (cw + 0.5) / W, (ch + 0.5) / H]


def layouts_for(W, H, rng):
    """Five layouts of nine slots -> fake / real boxes, validity.  See the case list in DESIGN.md §13."""
    fake = np.zeros((5, N, 4), np.float32)
    real = np.zeros((5, N, 4), np.float32)
    valid = np.zeros((5, N), np.uint8)

    def hits(n_in, n_out):
        """Whether some output sample of n_in -> n_out falls exactly on an input sample: (2 o + 1) n_in == (2 m + 1) n_out has a solution."""
        g = math.gcd(n_in, n_out)
        return (n_in // g) % 2 == 1 and (n_out // g) % 2 == 1

    def put(b, i, rect, crop_wh, on=1):
        # An output pixel that falls on an input sample on BOTH axes is an exact level in exact arithmetic: there the reference's own float noise
        # decides between k and k - 1 (the identity-size effect in small).  Off the identity cell, keep one axis free of such samples.  For the same
        # reason the jobs below shrink by 1.5 or more on at least one axis wherever the case list allows: an axis that grows, or shrinks by less than
        # 1.42 (sigma < 0.21: Gaussian side weights under 1e-5), interpolates integers with small rational weights, and at patches of a few pixels
        # such sums land on exact levels at about one pixel in a few hundred.
        cw, ch = crop_wh
        rw, rh = rect[2] - rect[0], rect[3] - rect[1]
        while b != 1 and cw > 1 and (hits(cw, rw) and hits(ch, rh) or cw == rw):
            cw -= 1
        fake[b, i], real[b, i], valid[b, i] = fake_box(W, H, *rect), real_box(W, H, cw, ch), on
    # 0: nothing valid (the slots still hold boxes and crops: they must not be drawn)
    for i in range(N):
        put(0, i, (3 + i, 2 + i, 12 + i, 9 + i), (7, 5), on=0)
    # 1: one element that keeps its size (identity on both axes)
    put(1, 0, (W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2), (W // 2, H // 2))
    # 2: nine overlapping elements: shrink both, grow both, shrink one axis and grow the other
    for i in range(N):
        rw, rh = int(rng.randint(4, W // 2)), int(rng.randint(4, H // 2))
        kind = i % 4
        cw = rw * 2 + 1 if kind in (0, 2) or i > 5 else max(2, rw // 2)       # (slots 1 and 5 grow on both axes)
        ch = rh * 2 + 1 if kind in (0, 3) else max(2, rh // 2)
        if cw == rw:
            cw -= 1
        if ch == rh:
            ch -= 1
        x1, y1 = int(rng.randint(0, W - rw)), int(rng.randint(0, H - rh))
        put(2, i, (x1, y1, x1 + rw, y1 + rh), (cw, ch))
    # 3: equal fake areas (the same w and h bit for bit) overlapping, so that the tie order shows; a 1-pixel-high target; a 3 px -> 1 px axis (the
    #    Gaussian's radius 4 exceeds the axis: repeated reflection); a 1-pixel crop axis
    rw, rh = W // 3, H // 3
    for i, (x1, y1) in enumerate([(W // 4, H // 4), (W // 4 + 3, H // 4 + 2), (W // 4 + 6, H // 4 - 1), (W // 4 + 1, H // 4 + 4)]):
        put(3, i, (x1, y1, x1 + rw, y1 + rh), (2 * rw + 1, rh - 2))
    put(3, 4, (2, 3, 14, 4), (8, 5))
    put(3, 5, (W - 6, 2, W - 5, 11), (3, 6))
    put(3, 6, (W - 12, H - 6, W - 8, H - 3), (1, 7))
    # 4: partly and wholly off the page on each side, with a gap in the valid slots; slot 0 covers the whole page and more
    put(4, 0, (-3, -2, W + 4, H + 3), (2 * W - 1, 2 * H - 1))
    put(4, 1, (5, 5, 15, 12), (6, 6), on=0)
    put(4, 2, (-4, 6, 7, 15), (5, 15))
    put(4, 3, (W - 6, -3, W + 5, 8), (20, 5))
    put(4, 4, (10, H - 4, 19, H + 6), (5, 21))
    put(4, 5, (W + 3, 4, W + 12, 11), (5, 5))
    put(4, 6, (-7, 8, 0, 14), (4, 4))
    put(4, 7, (12, -6, 20, 0), (5, 4))
    put(4, 8, (6, H + 2, 16, H + 9), (6, 5))
    return fake, real, valid


def check_margins(fake, real, valid, wh):
    for b in range(fake.shape[0]):
        W, H = int(wh[b][0]), int(wh[b][1])
        for i in range(fake.shape[1]):
            if not valid[b, i]:
                continue
            xc, yc, w, h = fake[b, i]
            two = np.float32(2)
            for v in ((xc - w / two) * np.float32(W), (xc + w / two) * np.float32(W), (yc - h / two) * np.float32(H), (yc + h / two) * np.float32(H)):
                assert abs((float(v) - 0.5) - round(float(v) - 0.5)) >= 1e-3, ('corner near a half-integer', b, i, float(v))
            for v in (real[b, i, 2] * np.float32(W), real[b, i, 3] * np.float32(H)):
                assert abs(float(v) - round(float(v))) >= 1e-3, ('real extent near an integer', b, i, float(v))


def run_case(util, fake, real, valid, canvases, wh, S, backgrounds):
    """-> crops, then per variant (white / bg) the fp32-input cells, the float64-input cells and the per-cell noise floor."""
    B = fake.shape[0]
    crops, drawable = [], valid.copy()
    for b in range(B):
        W, H = int(wh[b][0]), int(wh[b][1])
        row = []
        for i in range(fake.shape[1]):
            win = ISC.crop_window(canvases[b][i].shape[:2], real[b, i], W, H) if canvases[b][i] is not None else None
            row.append(None if win is None else np.ascontiguousarray(canvases[b][i][win[0]:win[1], win[2]:win[3]]))
            if win is None:
                drawable[b, i] = 0
        crops.append(row)
    out = {}
    for tag, bgs in (('white', None), ('bg', backgrounds))[:1 if backgrounds is None else 2]:
        cells = {}
        for name, dtype in (('', np.float32), ('_exact', np.float64)):
            cells[name] = np.stack([ref_cell(util, fake[b], real[b], drawable[b], canvases[b], int(wh[b][0]), int(wh[b][1]), S,
                                             None if bgs is None else bgs[b], dtype) for b in range(B)])
        out[tag], out[tag + '_exact_xor'] = cells[''], cells[''] ^ cells['_exact']       # (the second run as its XOR with the first: it compresses to nothing)
        noise = np.asarray([(cells[''][b] != cells['_exact'][b]).any(-1).mean() for b in range(B)])
        out[tag + '_noise'] = noise
        for b in range(B):
            W, H = int(wh[b][0]), int(wh[b][1])
            if not ISC.keeps_a_size(fake[b], valid[b], crops[b], W, H, None if bgs is None else bgs[b]):
                assert noise[b] <= 0.0025, ('noise floor', tag, b, noise[b])
            # the float64 restatement of the tests is the same procedure: it must reproduce the float64-input run
            mine = ISC.cell_f64(fake[b], valid[b], crops[b], W, H, S, None if bgs is None else bgs[b])
            assert np.abs(mine.astype(int) - cells['_exact'][b].astype(int)).max() <= 1, (tag, b)
    return crops, out


def main():
    util = _reference_util()
    rng = np.random.RandomState(20240)
    out = {'cases': np.asarray([c[0] for c in CASES]), 'case_whs': np.asarray([c[1:] for c in CASES], np.int32)}
    for name, W, H, S in CASES:
        fake, real, valid = layouts_for(W, H, rng)
        wh = [(W, H)] * 5
        check_margins(fake, real, valid, wh)
        canvases = [[texture(rng, 2 * H, 2 * W) for _ in range(N)] for _ in range(5)]
        two = np.stack([texture(rng, H + H // 2 + 2, W - 9) for _ in range(2)])             # a different size from the page on both axes
        backgrounds = two[[0, 1, 0, 1, 0]]                                                  # cell b lies over background b % 2
        crops, res = run_case(util, fake, real, valid, canvases, wh, S, backgrounds)
        buf, table = ISC.pack_crops(crops)
        out.update({f'{name}_bbox_fake': fake, f'{name}_bbox_real': real, f'{name}_valid': valid, f'{name}_crops': buf, f'{name}_crop_table': table,
                    f'{name}_backgrounds': two})
        out.update({f'{name}_{k}': v for k, v in res.items()})
        print(name, 'noise floor white', res['white_noise'].round(4), 'bg', res['bg_noise'].round(4))
    # the three items of tests/golden/dataset_tiny.zip: crops through LayoutDataset.patch_crops, the real boxes shifted and rescaled as the fake ones
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset
    path = os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip')
    dev, ref = LayoutDataset(path, mode='device'), LayoutDataset(path, mode='reference')
    items = [dev[i][0] for i in range(len(dev))]
    real = np.stack([it['bboxes'] for it in items]).astype(np.float32)
    valid = np.stack([it['mask'] for it in items]).astype(np.uint8)
    wh = [(int(it['W_page']), int(it['H_page'])) for it in items]
    fake = np.zeros_like(real)
    for b in range(len(items)):
        W, H = wh[b]
        for i in range(N):
            xc, yc, w, h = (float(v) for v in real[b, i])
            x1, y1, x2, y2 = int((xc - w / 2) * W), int((yc - h / 2) * H), int((xc + w / 2) * W), int((yc + h / 2) * H)
            fake[b, i] = fake_box(W, H, x1 + 5 - 3 * i, y1 - 4 + 2 * i, x2 + 11 + i, y2 - 9 + 2 * i) if valid[b, i] else 0
    check_margins(fake, real, valid, wh)
    canvases = []
    for b in range(len(items)):
        po = ref[b][0]['patches_orig']                                    # normalised fp32 [9, 3, Hc, Wc]: back to the uint8 the PNG holds
        u8 = np.clip(np.rint((np.asarray(po, np.float64).transpose(0, 2, 3, 1) * ISC.RGB_STD + ISC.RGB_MEAN) * 255.0), 0, 255).astype(np.uint8)
        canvases.append([u8[i] if valid[b, i] else None for i in range(N)])
    # white page only: the archive's decoded pages are 80 x 56 for 800 x 560 page sizes, a tenfold enlargement whose weights are multiples of 1 / 20 --
    # a large share of such pixels are exact levels, where the reference's float noise decides (measured: 0.7 % of a cell); backgrounds are the cases above
    crops, res = run_case(util, fake, real, valid, canvases, wh, TINY_CANVAS, None)
    for b in range(len(items)):
        mine = dev.patch_crops(b)
        assert all((c is None and m is None) or np.array_equal(c, m) for c, m in zip(crops[b], mine)), 'patch_crops differs from rule 8 on the decoded canvas'
    print('tiny: drawable crops per item', [sum(c is not None for c in row) for row in crops], 'noise floor', res['white_noise'].round(4))
    out.update({'tiny_bbox_fake': fake, 'tiny_wh': np.asarray(wh, np.int32), 'tiny_canvas': np.asarray(TINY_CANVAS)})
    out.update({f'tiny_{k}': v for k, v in res.items()})
    dev.close(); ref.close()
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
