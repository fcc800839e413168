"""Snapshot grids on the GPU: csrc/layout_raster.hip through render.layout_grid against the fixture made by the reference's own
convert_layout_to_image (tests/golden/snapshot.npz) and, for the inputs Pillow does not pin, against the restated rule (tests/snapshot_common.py);
training_loop's image snapshots; the contact sheet of generate.py.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import snapshot_common as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZIP = os.path.join(ROOT, 'tests', 'golden', 'dataset_tiny.zip')
CASES = ['land', 'port', 'up', 'same', 'round']


@pytest.fixture(scope='module')
def fx():
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'snapshot.npz'), allow_pickle=False)
    out = {k: d[k] for k in d.files}
    out['whs'] = {str(n): tuple(int(v) for v in w) for n, w in zip(d['cases'], d['case_whs'])}
    out['pal'] = [tuple(int(v) for v in c) for c in d['palette']]
    return out


def _grid(dev, bbox, valid, labels, pal, wh, S, pages=None, **kw):
    from layoutdetr_amd import render
    if pages is not None:
        pages = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in pages]
    g = render.layout_grid(torch.from_numpy(np.ascontiguousarray(bbox)).to(dev), torch.from_numpy(np.asarray(valid)), torch.from_numpy(np.asarray(labels).astype(np.int64)),
                           pal, wh, pages=pages, canvas=S, **kw)
    assert g.dtype == torch.uint8 and g.device.type == 'cuda'
    return g.cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got != want).any(-1).sum())
    assert bad == 0, f'{what}: {bad} of {got.shape[0] * got.shape[1]} pixels differ'


@pytest.mark.parametrize('name', CASES)
def test_kernel_reproduces_the_reference_fixture(dev, fx, name):
    """Every fixture case per cell (B = 1) and as a grid (B = 5), on white pages, over one page per cell, and with three cells naming ONE page."""
    W, H, S = fx['whs'][name]
    bb, va, la, pages = fx[f'{name}_bbox'], fx[f'{name}_valid'], fx[f'{name}_labels'], fx[f'{name}_pages']
    for k in range(5):
        _same(_grid(dev, bb[k:k + 1], va[k:k + 1], la[k:k + 1], fx['pal'], (W, H), S), fx[f'{name}_white'][k], f'{name} cell {k}')
        _same(_grid(dev, bb[k:k + 1], va[k:k + 1], la[k:k + 1], fx['pal'], (W, H), S, pages=[pages[k]]), fx[f'{name}_over'][k], f'{name} cell {k} over its page')
    _same(_grid(dev, bb, va, la, fx['pal'], (W, H), S), SC.make_grid(fx[f'{name}_white']), f'{name} grid')
    _same(_grid(dev, bb, va, la, fx['pal'], (W, H), S, pages=list(pages), nrow=2), SC.make_grid(fx[f'{name}_over'], nrow=2), f'{name} grid over pages')
    idx = [2, 3, 4]
    _same(_grid(dev, bb[idx], va[idx], la[idx], fx['pal'], (W, H), S, pages=[pages[0]], page_index=[0, 0, 0]), SC.make_grid(fx[f'{name}_shared']), f'{name} shared page')
    if name == 'land':
        _same(_grid(dev, bb, va, la, fx['pal'], (W, H), S, nrow=3), fx['grid_b5_nrow3'], 'B = 5, nrow = 3')
        _same(_grid(dev, bb, va, la, fx['pal'], (W, H), S), fx['grid_b5_default'], 'B = 5')
        _same(_grid(dev, bb[2:3], va[2:3], la[2:3], fx['pal'], (W, H), S), fx['grid_b1'], 'B = 1')


def test_kernel_mixed_page_sizes_in_one_grid_and_the_dataset_layouts(dev, fx):
    """Ragged pages: cells of four page sizes in one launch, some over pages and some white (page_index -1); the three layouts of dataset_tiny.zip
    at 800 x 560 -> 128 and over their decoded 80 x 56 pages."""
    names = ['land', 'port', 'same', 'round', 'port', 'land', 'round']
    ks = [2, 4, 3, 2, 1, 0, 4]
    over = [True, False, True, True, False, True, False]
    bb = np.stack([fx[f'{n}_bbox'][k] for n, k in zip(names, ks)])
    va = np.stack([fx[f'{n}_valid'][k] for n, k in zip(names, ks)])
    la = np.stack([fx[f'{n}_labels'][k] for n, k in zip(names, ks)])
    wh = [fx['whs'][n][:2] for n in names]
    pages, pidx = [], []
    for n, k, o in zip(names, ks, over):
        pidx.append(len(pages) if o else -1)
        if o:
            pages.append(fx[f'{n}_pages'][k])
    want = SC.make_grid(np.stack([fx[f'{n}_over' if o else f'{n}_white'][k] for n, k, o in zip(names, ks, over)]), nrow=3)      # 3 + 3 + 1: two empty slots
    _same(_grid(dev, bb, va, la, fx['pal'], wh, 16, pages=pages, page_index=pidx, nrow=3), want, 'mixed grid')
    tp = [tuple(int(v) for v in c) for c in fx['tiny_palette']]
    _same(_grid(dev, fx['tiny_bbox'], fx['tiny_valid'], fx['tiny_labels'], tp, fx['tiny_wh'], 128), SC.make_grid(fx['tiny_white']), 'dataset layouts')
    _same(_grid(dev, fx['tiny_bbox'], fx['tiny_valid'], fx['tiny_labels'], tp, (80, 56), 128, pages=list(fx['tiny_pages'])), SC.make_grid(fx['tiny_over']), 'dataset layouts over pages')


def _degenerate(rng, B, N):
    bb = np.concatenate([rng.uniform(-0.2, 1.2, (B, N, 2)), rng.uniform(0.0, 0.7, (B, N, 2))], -1).astype(np.float32)
    nan, inf = np.float32('nan'), np.float32('inf')
    bb[0, 0] = [0.5, 0.5, 0.0, 0.0]; bb[0, 1] = [0.3, 0.3, 0.01, 0.5]; bb[0, 2] = [0.6, 0.6, 0.5, 0.001]; bb[0, 3] = [0.5, 0.5, 0.04, 0.04]      # zero size, under 3 pixels
    bb[1, 0] = [nan, 0.5, 0.2, 0.2]; bb[1, 1] = [0.5, 0.5, nan, 0.2]; bb[1, 2] = [0.5, nan, 0.3, 0.3]; bb[1, 3] = [0.4, 0.4, 0.3, nan]
    bb[1, 4] = [inf, 0.5, inf, 0.2]; bb[1, 5] = [0.5, 0.5, inf, 0.0]                                                                               # inf - inf, inf * 0
    bb[2, 0] = [1e30, 0.5, 0.2, 0.2]; bb[2, 1] = [0.5, 0.5, 1e30, 0.3]; bb[2, 2] = [0.5, -1e30, 0.3, 0.3]; bb[2, 3] = [0.5, 0.5, 3e9, 3e9]
    bb[2, 4] = [0.5, 0.5, inf, 0.4]; bb[2, 5] = [0.5, 0.5, 0.5, inf]; bb[2, 6] = [4e7, 0.5, 8e7, 0.5]
    bb[3, 0] = [0.5, 0.5, -0.4, 0.3]; bb[3, 1] = [0.4, 0.6, 0.3, -0.5]; bb[3, 2] = [0.5, 0.5, -0.2, -0.2]                                          # negative extents: swapped
    va = rng.rand(B, N) < 0.8
    va[:4, :8] = True
    return bb, va.astype(np.uint8), rng.randint(0, 5, (B, N))


@pytest.mark.parametrize('W,H,S,over', [(50, 30, 16, False), (300, 200, 64, True), (40, 600, 64, False), (1200, 628, 128, False), (640, 640, 64, True),
                                         (64, 41, 64, True), (41, 64, 64, True)])
def test_own_rules_for_degenerate_boxes_equal_the_restatement(dev, fx, W, H, S, over):
    """Boxes under 3 pixels, zero size, NaN, infinities, coordinates beyond the int32 range, negative extents, 16 slots -- where Pillow's outline
    path differs between versions or rejects the input, the rule of DESIGN.md section 13 is the definition.  The page sizes take the kernel
    through one and several bands per cell, several source-row chunks per band, both letterbox directions, and one pass skipped while the
    other runs: 64 x 41 -> a 64 x 40 cell (no horizontal pass), 41 x 64 -> 40 x 64 (no vertical pass); the fixture's 16 x 16 case skips both."""
    rng = np.random.RandomState(W + S)
    B, N = 5, 16
    bb, va, la = _degenerate(rng, B, N)
    pages = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)] if over else None
    pidx = [0, 1, -1, 0, 1] if over else None
    want = SC.grid(bb, va, la, fx['pal'], (W, H), S, pages=pages, page_index=pidx)
    _same(_grid(dev, bb, va, la, fx['pal'], (W, H), S, pages=pages, page_index=pidx), want, f'{W} x {H} -> {S}')


def test_layout_grid_rejects_bad_arguments_on_the_host(dev):
    from layoutdetr_amd import render
    bb = torch.zeros(2, 9, 4, device=dev)
    ok = (torch.ones(2, 9), torch.zeros(2, 9), [(1, 2, 3)])
    with pytest.raises(ValueError, match='even'):
        render.layout_grid(bb, *ok, (50, 30), canvas=15)
    with pytest.raises(ValueError, match='no pixel'):
        render.layout_grid(bb, *ok, (1000, 1), canvas=16)
    with pytest.raises(ValueError, match='boxes per layout'):
        render.layout_grid(torch.zeros(2, 17, 4, device=dev), torch.ones(2, 17), torch.zeros(2, 17), [(1, 2, 3)], (50, 30))
    with pytest.raises(ValueError, match='palette'):
        render.layout_grid(bb, torch.ones(2, 9), torch.full((2, 9), 1), [(1, 2, 3)], (50, 30))
    with pytest.raises(RuntimeError, match='wider than'):
        render.layout_grid(bb, *ok, (6000, 4000))
    assert tuple(render.layout_grid(bb[:0], torch.ones(0, 9), torch.zeros(0, 9), [(1, 2, 3)], (50, 30)).shape) == (0, 0, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# training_loop


def _vocab(tmp, words):
    vf = tmp / 'vocab.txt'
    vf.write_text('\n'.join(['[PAD]', '[unused0]', '[UNK]', '[CLS]', '[SEP]', '[MASK]'] + sorted(words)) + '\n')
    return vf


def _loop_kwargs(vf, dataset_kwargs, validation=True, **over):
    P = 'layoutdetr_amd.training.'
    net = dict(bert_f_dim=768, bert_num_heads=4, bert_num_encoder_layers=2, bert_num_decoder_layers=2, im_f_dim=512, text_mode='encoder', tokenizer_vocab=str(vf))
    kw = dict(training_set_kwargs=dataset_kwargs, validation_set_kwargs=dataset_kwargs if validation else {}, data_loader_kwargs=dict(num_workers=0), random_seed=0,
              num_gpus=1, rank=0, batch_size=2, batch_gpu=2,
              G_kwargs=dict(class_name=P + 'networks_detr.Generator', z_dim=4, **net), D_kwargs=dict(class_name=P + 'networks_detr.Discriminator', **net),
              G_opt_kwargs=dict(class_name='torch.optim.Adam', betas=[0, 0.99], eps=1e-8, lr=1e-5), D_opt_kwargs=dict(class_name='torch.optim.Adam', betas=[0, 0.99], eps=1e-8, lr=1e-5),
              loss_kwargs=dict(class_name=P + 'loss.StyleGAN2Loss', r1_gamma=0.0, pl_weight=0.0), G_reg_interval=4, D_reg_interval=16,
              ema_kimg=2 * 10 / 32, total_kimg=0.004, kimg_per_tick=0.002, network_snapshot_ticks=None)
    kw.update(over)
    return kw


def _rng_states(dev):
    return torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone(), np.random.get_state()


@pytest.fixture(scope='module')
def runs(dev, tmp_path_factory):
    """The same short run on dataset_tiny.zip twice: with image_snapshot_ticks = 1 (train and val both point at the archive) and with None."""
    import json
    import zipfile
    from layoutdetr_amd.training import training_loop as tl
    words = set()
    with zipfile.ZipFile(ZIP) as z:
        for s in json.loads(z.read('non_image.json'))['samples']:
            for t in s[1]['texts']:
                words.update(t.replace('%', ' % ').replace('!', ' !').split())
    tmp = tmp_path_factory.mktemp('snapshots')
    vf = _vocab(tmp, words)
    ds_kw = dict(class_name='layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset', path=ZIP, use_labels=False, max_size=3, xflip=False, background_size=64)
    out = {}
    for name, ticks in (('on', 1), ('off', None)):
        d = tmp / name
        d.mkdir()
        res = tl.training_loop(run_dir=str(d), image_snapshot_ticks=ticks, **_loop_kwargs(vf, ds_kw))
        out[name] = dict(dir=d, states=_rng_states(dev), G_ema=res['G_ema'], G=res['G'], cur_nimg=res['stats']['cur_nimg'])
    out['ds_kw'], out['vf'] = ds_kw, vf
    return out


def _png(path):
    import PIL.Image
    return np.array(PIL.Image.open(path).convert('RGB'))


def test_training_loop_writes_the_snapshot_files(dev, fx, runs):
    from layoutdetr_amd import render
    from layoutdetr_amd.training.snapshot_images import SnapshotGrid, grid_indices
    from layoutdetr_amd.training.training_loop import construct_class_by_name
    d = runs['on']['dir']
    assert runs['on']['cur_nimg'] == 4
    want = {f'{s}_{kind}_{tag}.png' for s in ('train', 'val') for kind in ('layouts', 'layouts_over_background') for tag in ('real', 'fake_000000')}
    assert {f for f in os.listdir(d) if f.endswith('.png')} == want
    assert not [f for f in os.listdir(runs['off']['dir']) if f.endswith('.png')]
    # train_layouts_real.png is the fixture's grid: the reference's cells of the grid items, make_grid restated
    idx = grid_indices(3, 2)
    real = _png(d / 'train_layouts_real.png')
    _same(real, SC.make_grid(fx['tiny_white'][idx]), 'train_layouts_real.png')
    _same(_png(d / 'val_layouts_real.png'), real, 'val_layouts_real.png')
    over = _png(d / 'train_layouts_over_background_real.png')
    assert over.shape == (258 + 2, 2 * 258 + 2, 3)
    tp = [tuple(int(v) for v in c) for c in fx['tiny_palette']]
    _same(over, SC.grid(fx['tiny_bbox'][idx], fx['tiny_valid'][idx], fx['tiny_labels'][idx], tp, (80, 56), 256, pages=list(fx['tiny_pages'][idx])), 'over background')
    # train_layouts_fake_*.png is layout_grid of G_ema's boxes for the holder's z
    G_ema = runs['on']['G_ema']
    ds = construct_class_by_name(**runs['ds_kw'])
    try:
        holder = SnapshotGrid('train', ds, G_ema, 2, 2, dev, ds.colors)
    finally:
        ds.close()
    assert holder.indices == idx and tuple(holder.z.shape) == (2, 9, 4)
    fake = holder.fake_boxes(G_ema)
    assert not torch.equal(fake, holder.bbox_real)
    g = render.layout_grid(fake, holder.valid, holder.labels, holder.colors, holder.page_wh, canvas=128)
    _same(_png(d / 'train_layouts_fake_000000.png'), g.cpu().numpy(), 'train_layouts_fake')
    _same(g.cpu().numpy(), SC.grid(fake.cpu().numpy(), holder.valid.numpy(), holder.labels.numpy(), holder.colors, (800, 560), 128), 'fake grid against the restatement')


def test_image_snapshots_leave_the_generator_states_as_found(runs):
    a, b = runs['on']['states'], runs['off']['states']
    assert torch.equal(a[0], b[0]), 'torch CPU generator'
    assert torch.equal(a[1], b[1]), 'torch device generator'
    assert a[2][0] == b[2][0] and np.array_equal(a[2][1], b[2][1]) and a[2][2:] == b[2][2:], 'numpy generator'


def test_datasets_without_page_sizes_are_skipped_with_a_note(dev, tmp_path, capsys):
    from layoutdetr_amd.training import training_loop as tl
    import test_boundary_gpu as TB
    vf = _vocab(tmp_path, {w for s in TB.SyntheticLayouts().words for w in s.replace('%', ' % ').replace('!', ' !').split()})
    kw = _loop_kwargs(vf, dict(class_name='test_boundary_gpu.SyntheticLayouts', n=8), validation=False, batch_size=4, batch_gpu=4, total_kimg=0.004, kimg_per_tick=0.004,
                      ema_kimg=4 * 10 / 32)
    out = tl.training_loop(run_dir=str(tmp_path), image_snapshot_ticks=1, **kw)
    assert out['stats']['cur_nimg'] == 4
    printed = capsys.readouterr().out
    assert printed.count('Image snapshots skipped') == 1
    assert not [f for f in os.listdir(tmp_path) if f.endswith('.png')]


# ---------------------------------------------------------------------------------------------------------------------------------
# contact sheet


def test_contact_sheet_is_the_grid_of_the_ranked_candidates(dev):
    from layoutdetr_amd import generate, render
    g = torch.Generator().manual_seed(5)
    C, K, n = 2, 5, 4
    bbox = torch.cat([torch.rand(C, K, 9, 2, generator=g) * 0.6 + 0.2, torch.rand(C, K, 9, 2, generator=g) * 0.4 + 0.1], -1).to(dev)
    order = torch.tensor([[4, 0, 3, 1, 2], [2, 4, 1, 0, 3]], dtype=torch.int32, device=dev)
    res = generate.Layouts(bbox, bbox, None, None, order, torch.tensor([n, n], device=dev), [False] * K, [0] * K)
    page = torch.randint(0, 256, (40, 56, 3), dtype=torch.uint8, generator=g)
    labels = [0, 3, 5, 7]
    sheet = res.sheet(page.to(dev), labels, canvas=32, condition=1)
    assert tuple(sheet.shape) == (2 * 34 + 2, 3 * 34 + 2, 3)
    valid = (torch.arange(9) < n).expand(K, 9)
    lab = torch.tensor(labels + [0] * 5).expand(K, 9)
    want = render.layout_grid(bbox[1][order[1].long()], valid, lab, generate.PALETTE, (56, 40), pages=[page.to(dev)], page_index=[0] * K, canvas=32)
    assert torch.equal(sheet, want)
    _same(sheet.cpu().numpy(), SC.grid(bbox[1][order[1].long()].cpu().numpy(), valid.numpy(), lab.numpy(), generate.PALETTE, (56, 40), 32, pages=[page.numpy()], page_index=[0] * K), 'sheet')
    assert tuple(res.sheet(page.to(dev), labels).shape) == (2 * 258 + 2, 3 * 258 + 2, 3)


def test_generate_command_line_writes_the_sheet(dev, tmp_path):
    import copy
    import pickle
    import PIL.Image
    from layoutdetr_amd import generate
    from test_generate_gpu import _make_G
    vf = _vocab(tmp_path, {'sale', 'shop', 'now'})
    G = _make_G(dev, 64, seed=3, text_mode='encoder', tokenizer_vocab=str(vf), bert_num_encoder_layers=2, bert_num_heads=4)
    with open(tmp_path / 'snap.pkl', 'wb') as f:
        pickle.dump(dict(G=None, D=None, G_ema=copy.deepcopy(G).cpu(), augment_pipe=None, training_set_kwargs={}), f)
    page = np.random.RandomState(0).randint(0, 256, (40, 56, 3)).astype(np.uint8)
    PIL.Image.fromarray(page).save(tmp_path / 'bg.png')
    generate.main(['--ckpt', str(tmp_path / 'snap.pkl'), '--bg', str(tmp_path / 'bg.png'), '--bg-preprocessing', '128', '--strings', 'Sale|Shop now',
                   '--string-labels', 'header|button', '--seeds', '1-5', '--sheet', '--outfile', str(tmp_path / 'out' / 'x')])
    assert PIL.Image.open(tmp_path / 'out' / 'x_sheet.png').size == (3 * 258 + 2, 2 * 258 + 2)
    assert PIL.Image.open(tmp_path / 'out' / 'x_bboxes.png').size == (56, 40)
