"""Image snapshots of a training run: the reference's fixed sample grids (training_loop.py:36-59 setup_snapshot, :209-223 the `real` grids,
:371-392 the `fake` grids per snapshot tick), rendered on the device by render.layout_grid instead of util.save_image's per-element PIL loop.

Written per set (`train`, and `val` when a validation set is configured):
    <set>_layouts_real.png, <set>_layouts_fake_<kimg>.png                      the reference's save_image grids (canvas 128), bit-identical pixels
    <set>_layouts_over_background_real.png, ..._fake_<kimg>.png                this package's own kind: the same boxes over the sample's decoded page, canvas 256
and, when asked for (`kinds`; training_loop reads LDETR_IMAGE_SNAPSHOT_KINDS, `python -m layoutdetr_amd.dropin --image-snapshot-kinds=...` sets it):
    <set>_images_real.png, <set>_images_fake_<kimg>.png                        util.save_real_image (:144-231): every element's text patch resized to its box
    <set>_images_with_background_real.png, ..._fake_<kimg>.png                 util.save_real_image_with_background (:234-325): the same over the page
both at canvas 1024 by render.image_grid (two launches per grid; the rule is DESIGN.md §13, rules 8-12).  The patches are LayoutDataset.patch_crops of the
grid items, read once at setup; the page under `images_with_background` is the decoded page (the reference resizes its 256 x 256 training background up).
A dataset without patch files skips these two kinds with one printed note.

The grid items are read from a dataset instance of their own, opened here and closed afterwards: the training set's archive handle is shared
with the DataLoader's forked workers, and a read through it in the main process would move a file offset they use.  `z` comes from a private
generator; the torch (CPU, device) and numpy generator states are left as found."""
import contextlib
import os

import numpy as np
import torch

from .. import render

LAYOUT_CANVAS = 128          # util.save_image's default size_canvas
BACKGROUND_CANVAS = 256
IMAGE_CANVAS = render.IMAGE_CANVAS   # util.save_real_image's default size_canvas
KINDS = ('layouts', 'layouts_over_background', 'images', 'images_with_background')
DEFAULT_KINDS = KINDS[:2]
KINDS_ENV = 'LDETR_IMAGE_SNAPSHOT_KINDS'


def parse_kinds(kinds):
    """A tuple of kinds from a tuple / list or a comma-separated string; None or '' -> DEFAULT_KINDS.  An unknown kind is an error."""
    if kinds is None or kinds == '':
        return DEFAULT_KINDS
    if isinstance(kinds, str):
        kinds = [k.strip() for k in kinds.split(',') if k.strip()]
    kinds = tuple(kinds)
    bad = [k for k in kinds if k not in KINDS]
    if bad:
        raise ValueError(f'unknown image snapshot kind(s) {bad}: choose from {list(KINDS)}')
    return tuple(k for k in KINDS if k in kinds)


def grid_indices(n_items, batch_size, random_seed=0):
    """training_loop.py:37-40: a seeded shuffle of all item indices, repeated cyclically up to batch_size."""
    rnd = np.random.RandomState(random_seed)
    all_indices = list(range(n_items))
    rnd.shuffle(all_indices)
    return [all_indices[i % len(all_indices)] for i in range(batch_size)]


@contextlib.contextmanager
def preserved_rng(device):
    """Leave the torch CPU / device and numpy generator states as found (the contract metric_main.calc_metric keeps)."""
    device = torch.device(device)
    on_gpu = device.type == 'cuda'
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(device) if on_gpu else None, np.random.get_state())
    try:
        yield
    finally:
        torch.set_rng_state(state[0])
        if on_gpu:
            torch.cuda.set_rng_state(state[1], device)
        np.random.set_state(state[2])


class SnapshotGrid(object):
    """The fixed grid inputs of one dataset, kept on the device: per batch_gpu split the assembled generator inputs (boxes, labels, tokens,
    masks, resized backgrounds, conditioning labels) and the fixed z; for the whole grid the real boxes, the uint8 pages with their sizes, and
    host copies of the masks and labels (the raster entry reads those on the host)."""

    def __init__(self, name, dataset, G, batch_size, batch_gpu, device, colors, random_seed=0, kinds=DEFAULT_KINDS, image_canvas=IMAGE_CANVAS):
        from .dataset_layoutganpp import RawPage, decode_pages
        from .training_loop import assemble_batch
        self.name, self.device, self.colors = name, device, [tuple(int(v) for v in c) for c in colors]
        self.kinds, self.image_canvas = parse_kinds(kinds), int(image_canvas)
        self.indices = grid_indices(len(dataset), batch_size, random_seed)
        items = [dataset[i] for i in self.indices]
        collate = dataset.collate if (getattr(dataset, 'mode', None) in ('device', 'raw', 'packed') and hasattr(dataset, 'collate')) else torch.utils.data.default_collate
        self.page_wh = [(int(s['W_page']), int(s['H_page'])) for s, _ in items]
        pages = [s['background'] for s, _ in items]
        self.pages = self.pages_wh = None
        raw = [i for i, p in enumerate(pages) if isinstance(p, RawPage)]
        if raw:                                                            # mode='raw' / 'packed': the same uint8 pages, decoded on the device
            dec = decode_pages([pages[i] for i in raw], device)
            pages = list(pages)
            for j, i in enumerate(raw):
                pages[i] = dec[j]
            self.pages = render.PageSet([p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in pages])
            self.pages_wh = [(int(p.shape[1]), int(p.shape[0])) for p in pages]
        elif all(isinstance(p, np.ndarray) and p.dtype == np.uint8 and p.ndim == 3 for p in pages):
            self.pages = render.PageSet([torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in pages])
            self.pages_wh = [(int(p.shape[1]), int(p.shape[0])) for p in pages]      # the decoded page's own size
        self.patches = None
        if 'images' in self.kinds or 'images_with_background' in self.kinds:
            try:
                if not hasattr(dataset, 'patch_crops'):
                    raise KeyError('the dataset has no patch_crops')
                self.patches = render.PatchSet([dataset.patch_crops(i) for i in self.indices], device)
            except (KeyError, FileNotFoundError) as e:
                print(f'Image snapshots: the `images` kinds are skipped for the {name} set: no text patches ({e})')
        self.splits = []
        for lo in range(0, len(items), batch_gpu):
            samples, real_c = collate(items[lo:lo + batch_gpu])
            self.splits.append(assemble_batch(samples, real_c, G, dataset.background_size_for_training, device))
        self.bbox_real = torch.cat([s['bbox_real'] for s in self.splits])
        self.bbox_real_host = self.bbox_real.cpu()      # (the `images` kinds check the crop sizes against it on the host)
        self.valid = (~torch.cat([s['padding_mask'] for s in self.splits])).cpu()
        self.labels = torch.cat([s['bbox_class'] for s in self.splits]).cpu()
        gen = torch.Generator(device=device)
        gen.manual_seed(random_seed)
        self.z = torch.randn([len(items), self.bbox_real.shape[1], G.z_dim], dtype=torch.float32, device=device, generator=gen)

    def fake_boxes(self, G_ema):
        """G_ema on the fixed inputs, in batch_gpu splits (training_loop.py:373-376)."""
        out, lo = [], 0
        with torch.no_grad():
            for s in self.splits:
                n = s['bbox_real'].shape[0]
                out.append(G_ema(z=self.z[lo:lo + n], bbox_class=s['bbox_class'], bbox_real=s['bbox_real'], bbox_text=s['bbox_text'], bbox_patch=s['bbox_patch'],
                                 padding_mask=s['padding_mask'], background=s['background'], c=s['real_c']).detach().clone())
                lo += n
        return torch.cat(out)

    def grids(self, bbox):
        """{kind: uint8 grid} for one set of boxes: one raster launch per grid."""
        out = {}
        if 'layouts' in self.kinds:
            out['layouts'] = render.layout_grid(bbox, self.valid, self.labels, self.colors, self.page_wh, canvas=LAYOUT_CANVAS)
        if 'layouts_over_background' in self.kinds and self.pages is not None:
            out['layouts_over_background'] = render.layout_grid(bbox, self.valid, self.labels, self.colors, self.pages_wh, pages=self.pages, canvas=BACKGROUND_CANVAS)
        if self.patches is not None:
            for kind, pages in (('images', None), ('images_with_background', self.pages)):
                if kind not in self.kinds or (kind == 'images_with_background' and pages is None):
                    continue
                try:
                    out[kind] = render.image_grid(bbox, self.bbox_real_host, self.valid, self.patches, self.page_wh, backgrounds=pages, canvas=self.image_canvas)
                except RuntimeError as e:
                    # a generated box so small that one output pixel's source window exceeds the resize kernel's LDS (zoom 14 on both
                    # axes): a preview must not end a training run, so this grid is left out of this tick, with a note
                    if 'floats of LDS' not in str(e):
                        raise
                    print(f'Image snapshots: {self.name}_{kind} is not written at this tick: {e}')
        return out

    def write(self, run_dir, bbox, tag):
        paths = []
        for kind, grid in self.grids(bbox).items():
            paths.append(os.path.join(run_dir, f'{self.name}_{kind}_{tag}.png'))
            render.save_png(grid, paths[-1])
        return paths


def _open(name, dataset_kwargs, G, batch_size, batch_gpu, device, colors, random_seed, kinds, image_canvas):
    from .training_loop import construct_class_by_name
    dataset = construct_class_by_name(**dataset_kwargs)
    try:
        colors = getattr(dataset, 'colors', None) if colors is None else colors
        item = dataset[0][0] if len(dataset) else {}
        if colors is None or 'W_page' not in item or 'H_page' not in item:
            return None, colors
        return SnapshotGrid(name, dataset, G, batch_size, batch_gpu, device, colors, random_seed, kinds, image_canvas), colors
    finally:
        if hasattr(dataset, 'close'):
            dataset.close()


class ImageSnapshots(object):
    """What training_loop() holds: the train (and val) grids.  `setup` writes the `real` files, `write_fake` the files of one snapshot tick."""

    def __init__(self, run_dir, grids):
        self.run_dir, self.grids = run_dir, grids

    @classmethod
    def setup(cls, run_dir, training_set_kwargs, validation_set_kwargs, G, batch_size, batch_gpu, device, random_seed=0, kinds=None, image_canvas=IMAGE_CANVAS):
        """None (after one printed note) when the dataset's items carry no page sizes or the dataset has no palette.  kinds: a subset of KINDS
        (tuple or comma-separated string); None = DEFAULT_KINDS, the two `layouts` kinds."""
        kinds = parse_kinds(kinds)
        with preserved_rng(device):
            train, colors = _open('train', training_set_kwargs, G, batch_size, batch_gpu, device, None, random_seed, kinds, image_canvas)
            if train is None:
                print('Image snapshots skipped: the dataset has no page sizes (W_page / H_page) or no colors')
                return None
            grids = [train]
            if validation_set_kwargs:
                val, _ = _open('val', validation_set_kwargs, G, batch_size, batch_gpu, device, colors, random_seed, kinds, image_canvas)      # training_set.colors for both (:218)
                if val is not None:
                    grids.append(val)
            self = cls(run_dir, grids)
            print('Exporting sample images...')
            for g in grids:
                g.write(run_dir, g.bbox_real, 'real')
        return self

    def write_fake(self, G_ema, cur_nimg):
        with preserved_rng(self.grids[0].device):
            for g in self.grids:
                g.write(self.run_dir, g.fake_boxes(G_ema), f'fake_{cur_nimg // 1000:06d}')
