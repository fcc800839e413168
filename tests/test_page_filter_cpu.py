"""Page filters, the part that needs no GPU: the numpy restatement (tests/page_filter_common.py, the yardstick of the GPU tests) against Pillow,
generate.py's background-mode resolution and parser, and the "GPU memory only" errors of the Python surface."""
import os

import numpy as np
import pytest
import torch

import page_filter_common as PF


@pytest.mark.parametrize('pattern', ['random', 'checker'])
@pytest.mark.parametrize('hw', PF.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_restatement_equals_pillow(hw, pattern):
    """Bit for bit: GaussianBlur at radii 1, 3, 5 and the grey edge filter.  Guards the yardstick against a Pillow that behaves differently."""
    page = PF.pages(np.random.RandomState(hw[0] * 1000 + hw[1]), hw + (3,), pattern)
    for radius in (1, 3, 5):
        assert np.array_equal(PF.blur(page, radius), PF.pillow_filter(page, 'blur', radius)), f'blur radius {radius}'
    assert np.array_equal(PF.edge(page), PF.pillow_filter(page, 'edge'))


def test_box_radius_is_pillows_float_evaluation():
    """The stated constants at radius 3, and a sweep of radii: Pillow evaluates the box radius in C floats, and at a few radii (0.3, 1.35) the
    weight differs by one unit from a double evaluation, enough to move pixels."""
    assert PF.box_radius(3.0) == (2, 2876094, 1198373)
    assert PF.box_radius(0.3) == (0, 16273900, 251658)
    page = PF.pages(np.random.RandomState(5), (9, 40, 3), 'random')
    for radius in [0.05 * k for k in range(1, 101)]:
        assert np.array_equal(PF.blur(page, radius), PF.pillow_filter(page, 'blur', radius)), f'radius {radius}'


def test_restatement_takes_a_batch():
    pages = PF.pages(np.random.RandomState(2), (3, 7, 6, 3), 'random')
    for name, fn in PF.FILTERS.items():
        assert np.array_equal(fn(pages), np.stack([fn(p) for p in pages])), name


# ---------------------------------------------------------------------------------------------------------------------------------
# generate.py: (bg path, mode) -> (path to open, page_filter, size)


def test_resolve_background_all_eight_modes(tmp_path):
    from layoutdetr_amd import generate
    d = tmp_path / 'pages'
    d.mkdir()
    bg = str(d / 'banner.png')
    open(bg, 'wb').close()
    assert sorted(generate.BG_MODES) == sorted(['256', '128', 'blur', 'jpeg', 'rec', '3x_mask', 'edge', 'none'])
    assert generate.resolve_background(bg, 'none') == (bg, None, 1024)
    assert generate.resolve_background(bg, '3x_mask') == (bg, None, 1024)              # falls through to 'none' in the reference
    assert generate.resolve_background(bg, '256') == (bg, None, 256)
    assert generate.resolve_background(bg, '128') == (bg, None, 128)
    assert generate.resolve_background(bg, 'blur') == (bg, 'blur', 1024)
    assert generate.resolve_background(bg, 'edge') == (bg, 'edge', 1024)
    # the sibling files: <dir>_jpeg/<name with .png -> .jpg>, <dir>_rec/<name>
    jpeg, rec = str(tmp_path / 'pages_jpeg' / 'banner.jpg'), str(tmp_path / 'pages_rec' / 'banner.png')
    for mode, want in (('jpeg', jpeg), ('rec', rec)):
        with pytest.raises(FileNotFoundError) as e:
            generate.resolve_background(bg, mode)
        assert want in str(e.value), 'the error names the path that was looked for'
        os.makedirs(os.path.dirname(want))
        open(want, 'wb').close()
        assert generate.resolve_background(bg, mode) == (want, None, 1024)
    with pytest.raises(ValueError):
        generate.resolve_background(bg, 'sharpen')


def test_resolve_background_bare_file_name(tmp_path, monkeypatch):
    from layoutdetr_amd import generate
    d = tmp_path / 'here'
    (tmp_path / 'here_rec').mkdir()
    d.mkdir()
    open(tmp_path / 'here_rec' / 'p.png', 'wb').close()
    monkeypatch.chdir(d)
    assert os.path.samefile(generate.resolve_background('p.png', 'rec')[0], tmp_path / 'here_rec' / 'p.png')


def test_parser_takes_the_eight_choices_and_no_other():
    from layoutdetr_amd import generate
    base = ['--ckpt', 'x.pkl', '--bg', 'b.png', '--strings', 'a|b', '--string-labels', 'header|button', '--outfile', 'o']
    assert generate.parse_args(base).bg_preprocessing == 'none'
    for mode in ['256', '128', 'blur', 'jpeg', 'rec', '3x_mask', 'edge', 'none']:
        assert generate.parse_args(base + ['--bg-preprocessing', mode]).bg_preprocessing == mode
    with pytest.raises(SystemExit):
        generate.parse_args(base + ['--bg-preprocessing', 'sharpen'])


# ---------------------------------------------------------------------------------------------------------------------------------
# no CPU fallback


def test_cpu_tensors_are_refused():
    from layoutdetr_amd.training.dataset_layoutganpp import PAGE_FILTER_TILE, background_to_tensor, batch_backgrounds_to_device, filter_pages
    assert PAGE_FILTER_TILE == 64
    page = torch.zeros((5, 4, 3), dtype=torch.uint8)
    for kind in ('blur', 'edge'):
        with pytest.raises(RuntimeError, match='GPU memory'):
            filter_pages(page, kind)
        with pytest.raises(RuntimeError, match='GPU memory'):
            background_to_tensor(page, 8, page_filter=kind)
    with pytest.raises(ValueError):                               # float backgrounds are already resized: nothing to filter
        batch_backgrounds_to_device(torch.zeros((1, 3, 8, 8)), 8, torch.device('cpu'), page_filter='blur')
    with pytest.raises(ValueError):
        batch_backgrounds_to_device(page[None], 8, torch.device('cpu'), page_filter='sharpen')


def test_metric_options_background_filter():
    from layoutdetr_amd.metrics.metric_utils_layout import MetricOptions
    assert MetricOptions(device=torch.device('cpu')).background_filter is None
    assert MetricOptions(device=torch.device('cpu'), background_filter='edge').background_filter == 'edge'
    with pytest.raises(ValueError):
        MetricOptions(device=torch.device('cpu'), background_filter='sharpen')
