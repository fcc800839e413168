"""The `images` snapshot kinds on the GPU (DESIGN.md §13 rules 8-12): csrc/patch_resize.hip and the image raster of csrc/layout_raster.hip through
render.resize_u8 / render.image_grid, bit for bit against the fp32 restatement of the rule (tests/image_snapshot_common.py) and, under the two bars
of test_image_snapshot_cpu.judge, against the fixture made by the reference's own functions (tests/golden/image_snapshot.npz); ImageSnapshots and
training_loop with the kinds switched on."""
import os

import numpy as np
import pytest
import torch

import image_snapshot_common as ISC
import snapshot_common as SC
from test_image_snapshot_cpu import TINY, cases, judge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'image_snapshot.npz'), allow_pickle=False)
    return {k: d[k] for k in d.files}


@pytest.fixture(scope='module')
def want(gold):
    """The restated cells of every fixture case, computed once: {(name, tag): uint8 [5, S, S, 3]}."""
    out = {}
    for name, W, H, S, fake, valid, crops, bgs in cases(gold):
        for tag, backs in (('white', [None] * 5), ('bg', bgs)):
            out[name, tag] = np.stack([ISC.cell_f32(fake[b], valid[b], crops[b], W, H, S, backs[b]) for b in range(5)])
    return out


def _same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = int((got != ref).any(-1).sum())
    assert bad == 0, f'{what}: {bad} of {got.shape[0] * got.shape[1]} pixels differ'


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _grid(dev, fake, real, valid, patches, wh, S, backgrounds=None, **kw):
    from layoutdetr_amd import render
    g = render.image_grid(_t(fake, dev), _t(real, dev), torch.from_numpy(np.asarray(valid)), patches, wh, backgrounds=backgrounds, canvas=S, **kw)
    assert g.dtype == torch.uint8 and g.device.type == 'cuda'
    return g.cpu().numpy()


def test_patch_resize_is_the_rule_bit_for_bit(dev, gold):
    """Every resize job of the fixture (element crops and backgrounds) and the shapes at which the kernel takes another path, in ONE launch."""
    from layoutdetr_amd import render
    rng = np.random.RandomState(11)
    jobs = []
    for name, W, H, S, fake, valid, crops, bgs in cases(gold):
        for b in range(5):
            jobs += [(c, (y2 - y1, x2 - x1)) for _, c, (x1, y1, x2, y2) in ISC.jobs_of_cell(fake[b], valid[b], crops[b], W, H)]
        jobs += [(bg, (H, W)) for bg in gold[f'{name}_backgrounds']]

    def noise(h, w):
        return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    jobs += [(noise(40, 150), (70, 100)),        # several 16 x 64 tiles on both axes, the last ones partial
             (noise(90, 120), (7, 9)),           # zoom 13: radius 24 / 25, the tile shrinks until the window fits
             (noise(33, 700), (33, 70)),         # one axis kept, zoom 10 on the other: column tiles of a wide source
             (noise(1, 1), (5, 3)), (noise(2, 300), (9, 1)), (noise(65, 17), (17, 65))]
    assert len(jobs) > 60
    got = render.resize_u8([_t(c, dev) for c, _ in jobs], [s for _, s in jobs])
    torch.cuda.synchronize()
    for k, ((c, (ho, wo)), g) in enumerate(zip(jobs, got)):
        ref = ISC.resize_f32(c, ho, wo)
        g = g.cpu().numpy()
        assert g.shape == ref.shape and np.array_equal(g, ref), f'job {k}: {c.shape[1]} x {c.shape[0]} -> {wo} x {ho}: {int((g != ref).sum())} values differ'
        if c.shape[:2] == (ho, wo):
            assert np.array_equal(g, c)                    # an identity-size job returns its input


def test_patch_resize_refuses_what_does_not_fit(dev):
    from layoutdetr_amd import render
    with pytest.raises(RuntimeError, match='floats of LDS'):
        render.resize_u8([torch.zeros(600, 600, 3, dtype=torch.uint8, device=dev)], [(20, 20)])
    with pytest.raises(ValueError, match=r'every axis must be in \[1, 16384\]'):
        render.resize_u8([torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev)], [(0, 4)])


@pytest.mark.parametrize('name', ['land', 'port', 'round'])
def test_image_grid_is_the_rule_and_within_the_bars_of_the_reference(dev, gold, want, name):
    from layoutdetr_amd import render
    (_, W, H, S, fake, valid, crops, bgs), = [c for c in cases(gold) if c[0] == name]
    real = gold[f'{name}_bbox_real']
    patches = render.PatchSet(crops, dev)                            # ONE buffer for the five cells
    backs = render.PageSet([_t(b, dev) for b in gold[f'{name}_backgrounds']])
    for tag, kw in (('white', {}), ('bg', dict(backgrounds=backs, background_index=[0, 1, 0, 1, 0]))):
        g = _grid(dev, fake, real, valid, patches, (W, H), S, nrow=3, **kw)
        _same(g, SC.make_grid(want[name, tag], nrow=3), f'{name} {tag}: B = 5 at nrow = 3')
        for b in range(5):                                           # B = 1: the cell itself
            one = {k: ([v[b]] if k == 'background_index' else v) for k, v in kw.items()}
            cell = _grid(dev, fake[b:b + 1], real[b:b + 1], valid[b:b + 1], patches, (W, H), S, patch_index=[b], **one)
            _same(cell, want[name, tag][b], f'{name} {tag}: cell {b}')
            keeps = ISC.keeps_a_size(fake[b], valid[b], crops[b], W, H, None if tag == 'white' else bgs[b])
            judge(cell, gold[f'{name}_{tag}'][b], keeps, f'{name} {tag} cell {b} against the reference')
            r, c = 2 + (b // 3) * (S + 2), 2 + (b % 3) * (S + 2)
            judge(g[r:r + S, c:c + S], gold[f'{name}_{tag}'][b] ^ gold[f'{name}_{tag}_exact_xor'][b], keeps, f'{name} {tag} cell {b} against the float64-input run')
    # several cells share one cell of the patch buffer and one background; page sizes per cell
    idx = [2, 2, 4, 3, 2]
    g = _grid(dev, fake[idx], real[idx], valid[idx], patches, [(W, H)] * 5, S, backgrounds=backs, patch_index=idx, background_index=[1] * 5)
    _same(g, SC.make_grid(np.stack([ISC.cell_f32(fake[i], valid[i], crops[i], W, H, S, bgs[1]) for i in idx])), f'{name}: shared patches')


def test_image_grid_checks_its_inputs(dev, gold):
    from layoutdetr_amd import render
    (_, W, H, S, fake, valid, crops, bgs), = [c for c in cases(gold) if c[0] == 'land']
    real = gold['land_bbox_real']
    patches = render.PatchSet(crops, dev)
    with pytest.raises(ValueError, match='the crop is'):              # crops that were not made from these real boxes
        _grid(dev, fake, real[::-1].copy(), valid, patches, (W, H), S)
    with pytest.raises(ValueError, match='patches must be a render.PatchSet'):
        _grid(dev, fake, real, valid, crops, (W, H), S)
    with pytest.raises(ValueError, match='canvas size must be even'):
        _grid(dev, fake, real, valid, patches, (W, H), 33)
    nan = fake.copy()
    nan[2, 0, 2] = np.nan                                              # a NaN box draws nothing, here and in the restatement
    _same(_grid(dev, nan[2:3], real[2:3], valid[2:3], patches, (W, H), S, patch_index=[2]), ISC.cell_f32(nan[2], valid[2], crops[2], W, H, S), 'NaN box')


# ---------------------------------------------------------------------------------------------------------------------------------
# ImageSnapshots / training_loop


@pytest.fixture(scope='module')
def run(dev, tmp_path_factory):
    """One short training_loop run on dataset_tiny.zip with all four kinds switched on (train and val both point at the archive)."""
    import json
    import zipfile
    from test_snapshot_gpu import _loop_kwargs, _vocab
    from layoutdetr_amd.training import snapshot_images as SI
    from layoutdetr_amd.training import training_loop as tl
    words = set()
    with zipfile.ZipFile(TINY) as z:
        for s in json.loads(z.read('non_image.json'))['samples']:
            for t in s[1]['texts']:
                words.update(t.replace('%', ' % ').replace('!', ' !').split())
    tmp = tmp_path_factory.mktemp('image_snapshots')
    vf = _vocab(tmp, words)
    ds_kw = dict(class_name='layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset', path=TINY, use_labels=False, max_size=3, xflip=False, background_size=64)
    d = tmp / 'on'
    d.mkdir()
    saved = os.environ.get(SI.KINDS_ENV)
    os.environ[SI.KINDS_ENV] = ','.join(SI.KINDS)
    try:
        res = tl.training_loop(run_dir=str(d), image_snapshot_ticks=1, **_loop_kwargs(vf, ds_kw, total_kimg=0.002))
    finally:
        if saved is None:
            del os.environ[SI.KINDS_ENV]
        else:
            os.environ[SI.KINDS_ENV] = saved
    return dict(dir=d, tmp=tmp, G=res['G'], G_ema=res['G_ema'], ds_kw=ds_kw)


def _png(path):
    import PIL.Image
    return np.array(PIL.Image.open(path).convert('RGB'))


def test_training_loop_writes_the_image_kinds(dev, run):
    from layoutdetr_amd import render
    from layoutdetr_amd.training.snapshot_images import KINDS, SnapshotGrid
    from layoutdetr_amd.training.training_loop import construct_class_by_name
    d = run['dir']
    old = {f'{s}_{kind}_{tag}.png' for s in ('train', 'val') for kind in ('layouts', 'layouts_over_background') for tag in ('real', 'fake_000000')}
    new = {f'{s}_{kind}_{tag}.png' for s in ('train', 'val') for kind in ('images', 'images_with_background') for tag in ('real', 'fake_000000')}
    assert {f for f in os.listdir(d) if f.endswith('.png')} == old | new          # exactly four extra files per set
    ds = construct_class_by_name(**run['ds_kw'])
    try:
        holder = SnapshotGrid('train', ds, run['G_ema'], 2, 2, dev, ds.colors, kinds=KINDS)
        crops = [ds.patch_crops(i) for i in holder.indices]
    finally:
        ds.close()
    assert holder.patches is not None          # (the two grid items of this run have no drawable crop: the next test draws item 0's)
    real = _png(d / 'train_images_real.png')
    assert real.shape == (1024 + 4, 2 * 1026 + 2, 3)
    g = render.image_grid(holder.bbox_real, holder.bbox_real, holder.valid, holder.patches, holder.page_wh)
    _same(real, g.cpu().numpy(), 'train_images_real.png')
    _same(_png(d / 'val_images_real.png'), real, 'val_images_real.png')
    g = render.image_grid(holder.bbox_real, holder.bbox_real, holder.valid, holder.patches, holder.page_wh, backgrounds=holder.pages)
    _same(_png(d / 'train_images_with_background_real.png'), g.cpu().numpy(), 'train_images_with_background_real.png')
    fake = holder.fake_boxes(run['G_ema'])
    g = render.image_grid(fake, holder.bbox_real, holder.valid, holder.patches, holder.page_wh)
    _same(_png(d / 'train_images_fake_000000.png'), g.cpu().numpy(), 'train_images_fake')


def test_image_snapshots_kinds_and_generator_states(dev, run, capsys):
    from layoutdetr_amd.training.snapshot_images import KINDS, ImageSnapshots
    from test_snapshot_gpu import _rng_states
    torch.manual_seed(3); torch.cuda.manual_seed(4); np.random.seed(5)
    before = _rng_states(dev)
    for name, kinds, kinds_written in (('default', None, KINDS[:2]), ('images', 'images,images_with_background', KINDS[2:]), ('all', KINDS, KINDS)):
        d = run['tmp'] / name
        d.mkdir()
        snaps = ImageSnapshots.setup(str(d), run['ds_kw'], {}, run['G'], 4, 4, dev, kinds=kinds, image_canvas=64)
        snaps.write_fake(run['G_ema'], 2000)
        assert {f for f in os.listdir(d)} == {f'train_{kind}_{tag}.png' for kind in kinds_written for tag in ('real', 'fake_000002')}, name
    # four grid cells cycle through the three items, item 0 with its one drawable crop among them: the files against the restatement
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset
    holder = snaps.grids[0]
    ds = LayoutDataset(TINY, mode='device')
    try:
        crops = [ds.patch_crops(i) for i in holder.indices]
        pages = [ds[i][0]['background'] for i in holder.indices]
    finally:
        ds.close()
    assert sorted(set(holder.indices)) == [0, 1, 2] and sum(c is not None for row in crops for c in row) >= 1
    br, va = holder.bbox_real.cpu().numpy(), holder.valid.numpy()
    _same(_png(d / 'train_images_real.png'), ISC.grid_f32(br, va, crops, holder.page_wh, 64), 'train_images_real.png against the restatement')
    _same(_png(d / 'train_images_with_background_real.png'), ISC.grid_f32(br, va, crops, holder.page_wh, 64, backgrounds=pages), 'with background')
    after = _rng_states(dev)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), 'torch generators'
    assert before[2][0] == after[2][0] and np.array_equal(before[2][1], after[2][1]) and before[2][2:] == after[2][2:], 'numpy generator'
    assert 'are skipped' not in capsys.readouterr().out


def test_datasets_without_patches_skip_the_image_kinds_with_a_note(dev, run, capsys):
    from layoutdetr_amd.training import dataset_layoutganpp as DL
    from layoutdetr_amd.training.snapshot_images import KINDS, ImageSnapshots

    class NoPatches(DL.LayoutDataset):
        def patch_crops(self, idx):
            raise KeyError("There is no item named 'x_0_patch_orig.png' in the archive")
    DL.NoPatchesForTest = NoPatches
    try:
        d = run['tmp'] / 'nopatches'
        d.mkdir()
        kw = dict(run['ds_kw'], class_name='layoutdetr_amd.training.dataset_layoutganpp.NoPatchesForTest')
        snaps = ImageSnapshots.setup(str(d), kw, {}, run['G'], 2, 2, dev, kinds=KINDS, image_canvas=64)
        snaps.write_fake(run['G_ema'], 0)
    finally:
        del DL.NoPatchesForTest
    assert capsys.readouterr().out.count('the `images` kinds are skipped') == 1
    assert {f for f in os.listdir(d)} == {f'train_{kind}_{tag}.png' for kind in KINDS[:2] for tag in ('real', 'fake_000000')}
