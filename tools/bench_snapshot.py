"""Measurements behind the image snapshots (layoutdetr_amd/render.py, csrc/layout_raster.hip) -> profiles/snapshot_bench.json, one JSON line on stdout.

    python tools/bench_snapshot.py [--out profiles/snapshot_bench.json]

Configurations: B = 64 layouts of 9 boxes on white 1200 x 628 pages, canvas 128 (a `*_layouts_*` grid); B = 16 over 1200 x 628 uint8 pages, canvas 256 (a
`*_layouts_over_background_*` grid); B = 16 at canvas 1024 over 1200 x 628 pages with 9 text patches each, on white (`*_images_*`) and over a 1024 x 1024
background (`*_images_with_background_*`).
  (a) reference_procedure   the reference's save_image (util.py:85-141) RESTATED here: per sample `boxes[i][mask]` on device tensors, fp32 0-d tensor arithmetic,
                            one ImageDraw.rectangle per element on a page-sized canvas, a PIL BILINEAR resize, expand2square, the grid assembled with numpy in
                            place of ToTensor / make_grid (torchvision is not installed), PIL's PNG encoder
  (b) grid_and_png          render.layout_grid + render.save_png: one launch, one device-to-host copy, PIL's PNG encoder
  (c) launch                render.layout_grid alone
For the two `images` cases: (a) the reference's save_real_image[_with_background] (util.py:144-325) RESTATED: per element the 0-d tensor arithmetic, the
[3, H, W] fp32 canvas fetched from the device, crop, de-normalise, a stand-in of skimage.transform.resize on scipy.ndimage (gaussian_filter + zoom, float64;
skimage is not installed), paste; the page to uint8, PIL resize, grid, PNG.  (b) render.image_grid + save_png.  (c) render.image_grid alone: the two launches
and the host work in front of them (one device-to-host copy of the boxes, the job and axis tables).
Method (as tools/bench_generate.py): warm-up, then blocks of calls that last at least 0.2 s (at least 3 calls), each block timed by a pair of device events
(`*_us`) and by a host clock between two synchronisations (`host_*_us`); the versions alternate, 5 blocks each; median, minimum and maximum per call.  Kernel
launches per call are counted by torch.profiler.  (a) is bound by the host; what a training tick waits for is the host figure."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_generate import alternate, launches  # noqa: E402


def reference_cell(boxes, labels, colors, W_page, H_page, size_canvas, page=None):
    """util.py:85-112 restated (the canvas starts as `page` for the over-background kind)."""
    from PIL import Image, ImageDraw
    img = Image.new('RGB', (W_page, H_page), color=(255, 255, 255)) if page is None else Image.fromarray(page, 'RGB')
    draw = ImageDraw.Draw(img, 'RGBA')
    area = [b[2] * b[3] for b in boxes]
    for i in sorted(range(len(area)), key=lambda i: area[i], reverse=True):
        bbox, color = boxes[i], colors[labels[i]]
        xc, yc, w, h = bbox
        x1, y1, x2, y2 = xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2
        draw.rectangle([float(x1 * W_page), float(y1 * H_page), float(x2 * W_page), float(y2 * H_page)], outline=color, fill=color + (100,))
    if W_page > H_page:
        wn, hn = size_canvas, int(float(H_page) / float(W_page) * float(size_canvas)) // 2 * 2
    else:
        wn, hn = int(float(W_page) / float(H_page) * float(size_canvas)) // 2 * 2, size_canvas
    img = img.resize((wn, hn), resample=Image.BILINEAR)
    out = Image.new('RGB', (size_canvas, size_canvas), color=(0, 0, 0))
    out.paste(img, (0, (size_canvas - hn) // 2) if W_page > H_page else ((size_canvas - wn) // 2, 0))
    return out


def reference_save_image(bbox, labels, mask, colors, path, W, H, S, pages=None):
    """util.py:115-141 restated: the per-sample loop over DEVICE tensors, then the grid (numpy in place of make_grid) and the PNG."""
    from PIL import Image
    B = bbox.size(0)
    cells = []
    for i in range(B):
        m = mask[i]
        cells.append(np.array(reference_cell(bbox[i][m], labels[i][m], colors, W, H, S, None if pages is None else pages[i])))
    nrow = int(np.ceil(np.sqrt(B)))
    ymaps = int(np.ceil(B / nrow))
    grid = np.zeros((ymaps * (S + 2) + 2, nrow * (S + 2) + 2, 3), np.uint8)
    for k, c in enumerate(cells):
        grid[2 + (k // nrow) * (S + 2):2 + (k // nrow) * (S + 2) + S, 2 + (k % nrow) * (S + 2):2 + (k % nrow) * (S + 2) + S] = c
    Image.fromarray(grid, 'RGB').save(path)
    return grid


def resize_stand_in(im, shape):
    """skimage.transform.resize(im, shape, anti_aliasing=True) for a float [h, w, 3] image on scipy.ndimage, float64 (DESIGN.md §13 rule 10)."""
    import scipy.ndimage as ndi
    im = np.asarray(im, np.float64)
    shape = tuple(shape) + (3,)
    factors = np.divide(im.shape, shape)
    sigma = np.maximum(0, (factors - 1) / 2)
    out = ndi.zoom(ndi.gaussian_filter(im, sigma, mode='mirror') if np.any(sigma > 0) else im, [1.0 / f for f in factors], order=1, mode='mirror', grid_mode=True)
    return np.clip(out, im.min(), im.max())


def reference_real_cell(boxes_fake, boxes_real, images, W_page, H_page, size_canvas, bg=None):
    """util.py:144-204 / :234-295 restated, on the device tensors the reference is handed."""
    from PIL import Image
    mean = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 1, 3)
    std = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 1, 3)
    if bg is None:
        img = np.ones((H_page, W_page, 3))
    else:
        img = resize_stand_in(np.clip(np.transpose(bg.cpu().numpy(), [1, 2, 0]) * std + mean, 0.0, 1.0), (H_page, W_page))
    area = [b[2] * b[3] for b in boxes_fake]
    for i in sorted(range(len(area)), key=lambda i: area[i], reverse=True):
        fake, real = boxes_fake[i], boxes_real[i]
        width, height = int(real[2] * W_page), int(real[3] * H_page)
        image = np.transpose(images[i].cpu().numpy(), [1, 2, 0])
        cy, cx = image.shape[0] // 2, image.shape[1] // 2
        im = np.clip(image[cy - height // 2:cy + height - height // 2, cx - width // 2:cx + width - width // 2] * std + mean, 0.0, 1.0)
        xc, yc, w, h = fake
        x1, x2 = int(round((xc - w / 2).cpu().numpy() * float(W_page))), int(round((xc + w / 2).cpu().numpy() * float(W_page)))
        y1, y2 = int(round((yc - h / 2).cpu().numpy() * float(H_page))), int(round((yc + h / 2).cpu().numpy() * float(H_page)))
        im = resize_stand_in(im, (max(y2 - y1, 1), max(x2 - x1, 1)))
        xa, xb, ya, yb = max(x1, 0), min(x2, W_page), max(y1, 0), min(y2, H_page)
        if xa < xb and ya < yb:
            img[ya:yb, xa:xb] = im[ya - y1:yb - y1, xa - x1:xb - x1]
    img = Image.fromarray((img * 255.0).astype('ubyte'), 'RGB')
    wn, hn = (size_canvas, int(float(H_page) / float(W_page) * float(size_canvas)) // 2 * 2) if W_page > H_page else \
        (int(float(W_page) / float(H_page) * float(size_canvas)) // 2 * 2, size_canvas)
    out = Image.new('RGB', (size_canvas, size_canvas), color=(0, 0, 0))
    out.paste(img.resize((wn, hn), resample=Image.BILINEAR), (0, (size_canvas - hn) // 2) if W_page > H_page else ((size_canvas - wn) // 2, 0))
    return out


def reference_save_real_image(fake, real, images, mask, path, W, H, S, backgrounds=None):
    """util.py:207-231 / :298-325 restated: the per-sample loop over DEVICE tensors, the grid (numpy in place of make_grid) and the PNG."""
    from PIL import Image
    B = fake.size(0)
    cells = []
    for i in range(B):
        m = mask[i]
        cells.append(np.array(reference_real_cell(fake[i][m], real[i][m], images[i][m], W, H, S, None if backgrounds is None else backgrounds[i])))
    nrow = int(np.ceil(np.sqrt(B)))
    grid = np.zeros((int(np.ceil(B / nrow)) * (S + 2) + 2, nrow * (S + 2) + 2, 3), np.uint8)
    for k, c in enumerate(cells):
        grid[2 + (k // nrow) * (S + 2):2 + (k // nrow) * (S + 2) + S, 2 + (k % nrow) * (S + 2):2 + (k % nrow) * (S + 2) + S] = c
    Image.fromarray(grid, 'RGB').save(path)
    return grid


def image_cases(res, render, dev, g, tmp, W, H):
    """The two `images` kinds: B = 16, canvas 1024, 9 text patches per page."""
    B, N, S = 16, 9, 1024
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 1, 3, 1, 1)
    # smooth page-sized canvases: a coarse random field enlarged (text patches are not noise)
    coarse = torch.rand(B * N, 3, H // 8 + 1, W // 8 + 1, generator=g).to(dev)
    canv_u8 = (torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False) * 255.0).round().clamp(0, 255).to(torch.uint8).view(B, N, 3, H, W)
    images = (canv_u8.float() / 255.0 - mean) / std                                        # what the dataset hands the reference: [B, N, 3, H, W] fp32
    real = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.4 + 0.05], -1)
    fake = torch.cat([torch.rand(B, N, 2, generator=g) * 0.6 + 0.2, torch.rand(B, N, 2, generator=g) * 0.4 + 0.05], -1).to(dev)
    mask = torch.ones(B, N, dtype=torch.bool)
    crops = []
    for b in range(B):
        row = []
        for i in range(N):
            width, height = int(real[b, i, 2] * W), int(real[b, i, 3] * H)
            row.append(canv_u8[b, i, :, H // 2 - height // 2:H // 2 + height - height // 2, W // 2 - width // 2:W // 2 + width - width // 2].permute(1, 2, 0).contiguous())
        crops.append(row)
    patches = render.PatchSet(crops, dev)
    real_d, mask_d = real.to(dev), mask.to(dev)
    bg_coarse = torch.rand(B, 3, 129, 129, generator=g).to(dev)
    bg_u8 = (torch.nn.functional.interpolate(bg_coarse, size=(1024, 1024), mode='bilinear', align_corners=False) * 255.0).round().clamp(0, 255).to(torch.uint8)
    bg_norm = (bg_u8.float() / 255.0 - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    bg_pages = render.PageSet(list(bg_u8.permute(0, 2, 3, 1).contiguous()))
    for name, with_bg in (('images_B16_canvas1024', False), ('images_with_background_B16_canvas1024', True)):
        def reference_procedure():
            return reference_save_real_image(fake, real_d, images, mask_d, os.path.join(tmp, 'a.png'), W, H, S, bg_norm if with_bg else None)

        def launch():
            return render.image_grid(fake, real_d, mask, patches, (W, H), backgrounds=bg_pages if with_bg else None, canvas=S)

        def grid_and_png():
            render.save_png(launch(), os.path.join(tmp, 'b.png'))
        a, b = reference_procedure().astype(np.int32), launch().cpu().numpy().astype(np.int32)
        r = alternate(dict(reference_procedure=reference_procedure, grid_and_png=grid_and_png, launch=launch), warmup=1, blocks=3, min_calls=2)     # (a) takes seconds per call
        r['blocks'] = 3
        for k, fn in (('grid_and_png', grid_and_png), ('launch', launch)):
            r[k]['launches'] = launches(fn)
        r['max_level_difference_to_reference_procedure'] = int(np.abs(a - b).max())
        r['share_of_pixels_differing_from_reference_procedure'] = float((a != b).any(-1).mean())
        r['one_snapshot_adds_ms_host'] = r['grid_and_png']['host_median_us'] * 1e-3
        res['cases'][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'snapshot_bench.json'))
    args = ap.parse_args()
    from layoutdetr_amd import render
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    colors = [(246, 85, 85), (246, 205, 85), (165, 246, 85), (85, 246, 125), (85, 246, 246), (85, 125, 246), (165, 85, 246), (246, 85, 205)]
    W, H = 1200, 628
    res = dict(device=torch.cuda.get_device_name(0), page=[W, H], boxes_per_layout=9,
               method='device events (and, host_*, a synchronised host clock) around >= 0.2 s blocks of calls (>= 3); versions alternated; 5 blocks; median [min, max] in us per call',
               cases={})
    tmp = tempfile.mkdtemp()
    for name, B, S, over in (('layouts_B64_canvas128', 64, 128, False), ('over_background_B16_canvas256', 16, 256, True)):
        bbox = torch.cat([torch.rand(B, 9, 2, generator=g) * 0.6 + 0.2, torch.rand(B, 9, 2, generator=g) * 0.4 + 0.05], -1).to(dev)
        mask = (torch.arange(9)[None, :] < torch.randint(3, 10, (B, 1), generator=g))
        labels = torch.randint(0, 8, (B, 9), generator=g)
        pages_h = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g) if over else None
        pages = render.PageSet(list(pages_h.to(dev))) if over else None
        pages_np = pages_h.numpy() if over else None
        mask_d, labels_d = mask.to(dev), labels.to(dev)

        def reference_procedure():
            return reference_save_image(bbox, labels_d, mask_d, colors, os.path.join(tmp, 'a.png'), W, H, S, pages_np)

        def launch():
            return render.layout_grid(bbox, mask, labels, colors, (W, H), pages=pages, canvas=S)

        def grid_and_png():
            render.save_png(launch(), os.path.join(tmp, 'b.png'))
        same = bool(np.array_equal(reference_procedure(), launch().cpu().numpy()))
        r = alternate(dict(reference_procedure=reference_procedure, grid_and_png=grid_and_png, launch=launch), warmup=1)
        for k, fn in (('reference_procedure', reference_procedure), ('grid_and_png', grid_and_png), ('launch', launch)):
            r[k]['launches'] = launches(fn)
        r['pixels_equal_reference_procedure'] = same
        r['one_snapshot_adds_ms_host'] = r['grid_and_png']['host_median_us'] * 1e-3
        res['cases'][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    image_cases(res, render, dev, g, tmp, W, H)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
