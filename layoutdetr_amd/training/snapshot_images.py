"""Image snapshots of a training run: the reference's fixed sample grids (training_loop.py:36-59 setup_snapshot, :209-223 the `real` grids,
:371-392 the `fake` grids per snapshot tick), rendered on the device by render.layout_grid instead of util.save_image's per-element PIL loop.

Written per set (`train`, and `val` when a validation set is configured):
    <set>_layouts_real.png, <set>_layouts_fake_<kimg>.png                      the reference's save_image grids (canvas 128), bit-identical pixels
    <set>_layouts_over_background_real.png, ..._fake_<kimg>.png                this package's own kind: the same boxes over the sample's decoded page, canvas 256
The reference's `*_images_*` kinds paste the decoded text patches (skimage.transform.resize); this path never decodes patches, so they are not built.

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

    def __init__(self, name, dataset, G, batch_size, batch_gpu, device, colors, random_seed=0):
        from .training_loop import assemble_batch
        self.name, self.device, self.colors = name, device, [tuple(int(v) for v in c) for c in colors]
        self.indices = grid_indices(len(dataset), batch_size, random_seed)
        items = [dataset[i] for i in self.indices]
        collate = dataset.collate if (getattr(dataset, 'mode', None) == 'device' and hasattr(dataset, 'collate')) else torch.utils.data.default_collate
        self.page_wh = [(int(s['W_page']), int(s['H_page'])) for s, _ in items]
        pages = [s['background'] for s, _ in items]
        self.pages = self.pages_wh = None
        if all(isinstance(p, np.ndarray) and p.dtype == np.uint8 and p.ndim == 3 for p in pages):
            self.pages = render.PageSet([torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in pages])
            self.pages_wh = [(int(p.shape[1]), int(p.shape[0])) for p in pages]      # the decoded page's own size
        self.splits = []
        for lo in range(0, len(items), batch_gpu):
            samples, real_c = collate(items[lo:lo + batch_gpu])
            self.splits.append(assemble_batch(samples, real_c, G, dataset.background_size_for_training, device))
        self.bbox_real = torch.cat([s['bbox_real'] for s in self.splits])
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
        out = {'layouts': render.layout_grid(bbox, self.valid, self.labels, self.colors, self.page_wh, canvas=LAYOUT_CANVAS)}
        if self.pages is not None:
            out['layouts_over_background'] = render.layout_grid(bbox, self.valid, self.labels, self.colors, self.pages_wh, pages=self.pages, canvas=BACKGROUND_CANVAS)
        return out

    def write(self, run_dir, bbox, tag):
        paths = []
        for kind, grid in self.grids(bbox).items():
            paths.append(os.path.join(run_dir, f'{self.name}_{kind}_{tag}.png'))
            render.save_png(grid, paths[-1])
        return paths


def _open(name, dataset_kwargs, G, batch_size, batch_gpu, device, colors, random_seed):
    from .training_loop import construct_class_by_name
    dataset = construct_class_by_name(**dataset_kwargs)
    try:
        colors = getattr(dataset, 'colors', None) if colors is None else colors
        item = dataset[0][0] if len(dataset) else {}
        if colors is None or 'W_page' not in item or 'H_page' not in item:
            return None, colors
        return SnapshotGrid(name, dataset, G, batch_size, batch_gpu, device, colors, random_seed), colors
    finally:
        if hasattr(dataset, 'close'):
            dataset.close()


class ImageSnapshots(object):
    """What training_loop() holds: the train (and val) grids.  `setup` writes the `real` files, `write_fake` the files of one snapshot tick."""

    def __init__(self, run_dir, grids):
        self.run_dir, self.grids = run_dir, grids

    @classmethod
    def setup(cls, run_dir, training_set_kwargs, validation_set_kwargs, G, batch_size, batch_gpu, device, random_seed=0):
        """None (after one printed note) when the dataset's items carry no page sizes or the dataset has no palette."""
        with preserved_rng(device):
            train, colors = _open('train', training_set_kwargs, G, batch_size, batch_gpu, device, None, random_seed)
            if train is None:
                print('Image snapshots skipped: the dataset has no page sizes (W_page / H_page) or no colors')
                return None
            grids = [train]
            if validation_set_kwargs:
                val, _ = _open('val', validation_set_kwargs, G, batch_size, batch_gpu, device, colors, random_seed)      # training_set.colors for both (:218)
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
