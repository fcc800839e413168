"""Page filters on the device (csrc/page_filter.hip) against live Pillow, zero tolerance: the kernel entry, `filter_pages`,
`background_to_tensor(page_filter=...)`, `batch_backgrounds_to_device`, the generate command line and the metric passes."""
import copy
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

import layout_eval_common as C
import page_filter_common as PF

pytestmark = pytest.mark.gpu

from layoutdetr_amd.training.dataset_layoutganpp import PAGE_FILTER_TILE as T   # noqa: E402

# every size of the CPU test, plus the tile seams on each axis paired with a small other axis
SEAMS = [(t, 5) for t in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1)] + [(5, t) for t in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1)]
KINDS = [('blur', 1.0), ('blur', 3.0), ('blur', 5.0), ('edge', 3.0)]


def _check(dev, hw, n, pattern):
    from layoutdetr_amd.training.dataset_layoutganpp import filter_pages
    pages = PF.pages(np.random.RandomState(hw[0] * 1000 + hw[1] + n), (n,) + hw + (3,), pattern)
    d = torch.from_numpy(pages).to(dev)
    for kind, radius in KINDS:
        want = np.stack([PF.pillow_filter(p, kind, radius) for p in pages])
        got = filter_pages(d, kind, radius)
        assert got.dtype == torch.uint8 and got.shape == d.shape and got.data_ptr() != d.data_ptr()
        bad = int((got.cpu() != torch.from_numpy(want)).sum())
        print(f'{kind} radius {radius} {hw} x{n} {pattern}: {bad} bytes differ')
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (kind, radius)
        assert torch.equal(d.cpu(), torch.from_numpy(pages)), 'the input was written to'
        if n > 1:                                                # one call over n images = n single calls
            for i in range(n):
                assert torch.equal(filter_pages(d[i], kind, radius), got[i]), (kind, i)


@pytest.mark.parametrize('pattern', ['random', 'checker'])
@pytest.mark.parametrize('hw', PF.SIZES + SEAMS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_filter_pages_equals_pillow(dev, hw, pattern):
    _check(dev, hw, 1, pattern)


@pytest.mark.parametrize('hw', [(33, 17), (T + 1, 5), (5, 2 * T + 1), (T + 3, T + 2)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_three_images_in_one_call(dev, hw):
    _check(dev, hw, 3, 'random')
    _check(dev, hw, 3, 'checker')


def test_unaligned_view_and_single_page(dev):
    """A page that starts in the middle of a buffer (odd byte offset) and the [H, W, 3] form."""
    from layoutdetr_amd.training.dataset_layoutganpp import filter_pages
    pages = PF.pages(np.random.RandomState(4), (3, 7, 5, 3), 'random')           # 105 bytes per page: page 1 starts at an odd address
    d = torch.from_numpy(pages).to(dev)
    for kind in ('blur', 'edge'):
        got = filter_pages(d[1], kind)
        assert got.shape == (7, 5, 3) and torch.equal(got.cpu(), torch.from_numpy(PF.pillow_filter(pages[1], kind)))


def test_python_surface_rejections(dev):
    from layoutdetr_amd.training.dataset_layoutganpp import filter_pages
    page = torch.zeros((4, 5, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        filter_pages(page, 'sharpen')
    with pytest.raises(ValueError):
        filter_pages(page.float(), 'blur')
    with pytest.raises(ValueError):
        filter_pages(page[..., :2], 'blur')
    for radius in (0.0, 5.5, -1.0):
        with pytest.raises(ValueError):
            filter_pages(page, 'blur', radius)
    filter_pages(page, 'edge', 0.0)                              # the radius is ignored for the edge filter


def test_host_rejections(dev):
    """The C entry: overlapping src / dst, bad kind, radius 0 and 5.5, null pointers, bad shapes; images == 0 is a no-op."""
    from layoutdetr_amd.hip import core
    lib = core.lib()
    H, W = 6, 8
    buf = torch.zeros(3 * H * W * 3, dtype=torch.uint8, device=dev)
    n1 = H * W * 3
    src, dst = buf.data_ptr(), buf.data_ptr() + 2 * n1
    st = core.stream()

    def call(s, d, images, h, w, kind, radius):
        return lib.ldetr_page_filter_u8(ctypes.c_void_p(s), ctypes.c_void_p(d), images, h, w, kind, radius, st)
    assert call(src, dst, 1, H, W, 1, 3.0) == 0 and call(src, dst, 1, H, W, 2, 0.0) == 0
    assert call(src, dst, 0, H, W, 1, 3.0) == 0
    for args in ((src, src, 1, H, W, 1, 3.0), (src, src + n1, 2, H, W, 2, 3.0), (src + n1, src, 2, H, W, 1, 3.0),      # overlap
                 (src, dst, 1, H, W, 0, 3.0), (src, dst, 1, H, W, 3, 3.0),                                              # kind
                 (src, dst, 1, H, W, 1, 0.0), (src, dst, 1, H, W, 1, 5.5),                                              # radius
                 (None, dst, 1, H, W, 1, 3.0), (src, None, 1, H, W, 1, 3.0), (src, dst, -1, H, W, 1, 3.0), (src, dst, 1, 0, W, 1, 3.0),
                 (src, dst, 1, H, 0, 2, 3.0)):
        assert call(*args) != 0, args
        assert b'page_filter' in lib.ldetr_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# filter + resize + normalise


def _reference_background(page, S, kind):
    """Pillow filter, resize((S, S), LANCZOS), then the reference's two normalisation lines (dataset_layoutganpp.py:335-336)."""
    from PIL import Image
    from layoutdetr_amd.training.dataset_layoutganpp import RGB_MEAN, RGB_STD
    img = Image.fromarray(page if kind is None else PF.pillow_filter(page, kind))
    bg = np.array(img.resize((S, S), Image.LANCZOS))
    mean = np.reshape(np.array(RGB_MEAN).astype(np.float32), (1, 1, 3))
    std = np.reshape(np.array(RGB_STD).astype(np.float32), (1, 1, 3))
    bg = (bg.astype(np.float32) / 255.0 - mean) / std
    return bg.transpose(2, 0, 1)


@pytest.mark.parametrize('S', [32, 64])
@pytest.mark.parametrize('kind', ['blur', 'edge'])
def test_background_to_tensor_with_filter(dev, kind, S):
    from layoutdetr_amd.training.dataset_layoutganpp import background_to_tensor
    page = np.random.RandomState(7).randint(0, 256, (40, 56, 3)).astype(np.uint8)
    got = background_to_tensor(torch.from_numpy(page).to(dev), S, page_filter=kind)
    want = _reference_background(page, S, kind)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, S, S)
    assert np.array_equal(got.cpu().numpy(), want), 'not bit-identical in fp32'
    plain = background_to_tensor(torch.from_numpy(page).to(dev), S)
    assert torch.equal(plain, background_to_tensor(torch.from_numpy(page).to(dev), S, page_filter=None)) and not torch.equal(plain, got)


def test_batch_backgrounds_two_page_sizes(dev):
    from layoutdetr_amd.training.dataset_layoutganpp import background_to_tensor, batch_backgrounds_to_device
    rs = np.random.RandomState(8)
    pages = [torch.from_numpy(rs.randint(0, 256, hw + (3,)).astype(np.uint8)) for hw in ((40, 56), (70, 33), (40, 56))]
    for kind in ('blur', 'edge', None):
        got = batch_backgrounds_to_device(pages, 32, dev, page_filter=kind)
        for i, p in enumerate(pages):
            assert torch.equal(got[i], background_to_tensor(p.to(dev), 32, page_filter=kind)), (kind, i)
    stacked = torch.stack([pages[0], pages[2]])
    assert torch.equal(batch_backgrounds_to_device(stacked, 32, dev, page_filter='blur'), batch_backgrounds_to_device(pages, 32, dev, page_filter='blur')[[0, 2]])
    with pytest.raises(ValueError):
        batch_backgrounds_to_device(torch.zeros((1, 3, 32, 32)), 32, dev, page_filter='edge')


# ---------------------------------------------------------------------------------------------------------------------------------
# command line


def test_generate_command_line_background_modes(dev, tmp_path):
    """--bg-preprocessing blur = the Python API on a page Pillow blurred beforehand (bit-identical inputs, so equal boxes), differs from none;
    jpeg reads the sibling file; the boxes are drawn over the original page."""
    import PIL.Image
    from layoutdetr_amd import generate
    from test_generate_gpu import _make_G
    from test_snapshot_gpu import _vocab
    vf = _vocab(tmp_path, {'sale', 'shop', 'now'})
    G = _make_G(dev, 64, seed=3, text_mode='encoder', tokenizer_vocab=str(vf), bert_num_encoder_layers=2, bert_num_heads=4)
    with open(tmp_path / 'snap.pkl', 'wb') as f:
        pickle.dump(dict(G=None, D=None, G_ema=copy.deepcopy(G).cpu(), augment_pipe=None, training_set_kwargs={}), f)
    rs = np.random.RandomState(0)
    page = rs.randint(0, 256, (40, 56, 3)).astype(np.uint8)
    other = rs.randint(0, 256, (30, 44, 3)).astype(np.uint8)
    (tmp_path / 'pages').mkdir()
    (tmp_path / 'pages_jpeg').mkdir()
    PIL.Image.fromarray(page).save(tmp_path / 'pages' / 'bg.png')
    PIL.Image.fromarray(other).save(tmp_path / 'pages_jpeg' / 'bg.jpg', quality=90)
    texts, labels, seeds = ['Sale', 'Shop now'], [0, 5], [1, 2, 3]

    def run(mode):
        out = tmp_path / 'out' / mode
        generate.main(['--ckpt', str(tmp_path / 'snap.pkl'), '--bg', str(tmp_path / 'pages' / 'bg.png'), '--bg-preprocessing', mode, '--strings', '|'.join(texts),
                       '--string-labels', 'header|button', '--seeds', '1-3', '--outfile', str(out)])
        assert PIL.Image.open(str(out) + '_bboxes.png').size == (56, 40)
        return json.load(open(str(out) + '.json'))['bbox_raw']

    def api(page_u8):
        Gl = generate.load_generator(str(tmp_path / 'snap.pkl'), dev, None)
        res = generate.generate_layouts(Gl, [torch.from_numpy(page_u8)], [texts], [labels], seeds, background_size=1024)
        return res.bbox_raw[0, :, :2].tolist()
    blur, none = run('blur'), run('none')
    assert blur == api(PF.pillow_filter(page, 'blur', 3.0))
    assert none == api(page) and blur != none
    assert run('3x_mask') == none
    assert run('jpeg') == api(np.array(PIL.Image.open(tmp_path / 'pages_jpeg' / 'bg.jpg').convert('RGB')))
    with pytest.raises(FileNotFoundError, match='pages_rec'):
        run('rec')


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics


def _metric_kwargs(tmp_path, monkeypatch, dev, G):
    from layoutdetr_amd.training.networks_layoutnet import LayoutNet
    zpath = C.stage_dataset(tmp_path)
    C.write_detector(tmp_path, LayoutNet)
    monkeypatch.chdir(tmp_path)
    return dict(G=G, dataset_kwargs=dict(class_name='layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset', path=zpath, use_labels=False, max_size=None,
                                         xflip=False, background_size=32), num_gpus=1, rank=0, device=dev)


class _Recorder(C.StubGenerator):
    """The stub generator, keeping the backgrounds it is called with."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, *args, background=None, **kwargs):
        self.seen.append(background.clone())
        return super().forward(*args, background=background, **kwargs)


def test_metric_batches_carry_the_filtered_backgrounds(dev, tmp_path, monkeypatch):
    """At the batch-assembly level: with background_filter='edge' G receives exactly background_to_tensor(page, S, page_filter='edge') of every
    item's page, and with None what it received before."""
    from layoutdetr_amd.metrics import metric_utils_layout as mu
    from layoutdetr_amd.training.dataset_layoutganpp import LayoutDataset, background_to_tensor
    kw = _metric_kwargs(tmp_path, monkeypatch, dev, None)
    ds = LayoutDataset(path=kw['dataset_kwargs']['path'], background_size=32)
    pages = [torch.as_tensor(ds[i][0]['background']).to(dev) for i in range(len(ds))]
    for flt in ('edge', None):
        G = _Recorder().to(dev)
        opts = mu.MetricOptions(**dict(kw, G=G), cache=False, batch_size=2, background_filter=flt)
        opts.dataset_kwargs.update(max_size=None, xflip=False)
        dataset = mu._construct(opts.dataset_kwargs)
        walk = mu._ItemWalk(opts, dataset, None, None, None)
        n = 0
        for bt, _fake, _real in mu._generator_batches(opts, walk, dataset):
            for b in range(bt['background'].shape[0]):
                assert torch.equal(bt['background'][b], background_to_tensor(pages[n], 32, page_filter=flt)), (flt, n)
                assert torch.equal(G.seen[-1][b], bt['background'][b])
                n += 1
        assert n == len(ds)


def test_calc_metric_reports_the_background_filter(dev, tmp_path, monkeypatch):
    from layoutdetr_amd.metrics import metric_main
    name = 'layout_fid50k_train'
    kw = _metric_kwargs(tmp_path, monkeypatch, dev, C.StubGenerator().to(dev))
    cache = tmp_path / 'cache'
    plain = metric_main.calc_metric(name, cache_dir=str(cache), **kw)
    files = sorted(p.name for p in cache.iterdir())
    none = metric_main.calc_metric(name, cache_dir=str(cache), background_filter=None, **kw)
    edge = metric_main.calc_metric(name, cache_dir=str(cache), background_filter='edge', **kw)
    assert plain.background_filter is None and none.background_filter is None and edge.background_filter == 'edge'
    assert none.results == plain.results
    # real-data statistics do not depend on the background: one cache file, the same name, whatever the filter
    assert sorted(p.name for p in cache.iterdir()) == files and len(files) == 1
    assert json.loads(json.dumps(dict(edge)))['background_filter'] == 'edge'
    assert edge.results[name] == plain.results[name]            # the stub generator ignores its background
