"""No GPU: what tests/test_resampling_gpu.py relies on.  The case tables of tests/resampling_common.py reach every path name of the three
families (the predicates restate the host-side selection of csrc/upfirdn2d.hip, csrc/demod.hip, csrc/resample.hip and their Python wrappers) and
every value of every factor; the float64 references agree with an independent form; three deliberately wrong references are caught at the bounds
the GPU file uses; and the recorded float32 yardsticks are what this machine measures."""
import numpy as np
import pytest
import torch

import resampling_common as R
from oracle import resample_ref

R.limit_threads()


# ------------------------------------------------------------------------------------------------------------------------ path coverage
@pytest.mark.parametrize('family,cases,paths,predicate', [
    ('upfirdn', R.UPFIRDN_CASES, R.UPFIRDN_PATHS, R.upfirdn_paths), ('demod', R.DEMOD_CASES, R.DEMOD_PATHS, R.demod_paths),
    ('resize', R.RESIZE_CASES, R.RESIZE_PATHS, R.resize_paths)], ids=['upfirdn', 'demod', 'resize'])
def test_every_path_is_reached_and_none_is_unknown(family, cases, paths, predicate):
    assert len(set(paths)) == len(paths)
    seen = {}
    for c in cases:
        names = predicate(c)
        assert names, c['name']
        unknown = names - set(paths)
        assert not unknown, f'{family} {c["name"]}: unknown path {sorted(unknown)}'
        for n in names:
            seen.setdefault(n, c['name'])
    missing = [p for p in paths if p not in seen]
    assert not missing, f'{family}: no case takes {missing}'


def test_upfirdn_predicate_on_the_shapes_the_kernel_comments_name():
    def fir(N, C, oH, oW, **kw):
        c = R.uf_case('probe', (N, C, oH + 1, oW + 1), 'cl', **kw)
        return R.upfirdn_paths(c)
    assert {'fir4x4/TR4', 'fir4x4/xcd_map/full'} <= fir(1, 64, 128, 64)                 # 64 blocks
    assert {'fir4x4/TR4', 'fir4x4/xcd_map/padded_grid'} <= fir(1, 64, 130, 64)          # 66 blocks, padded to 72
    assert 'fir4x4/identity_map' in fir(1, 64, 124, 64)                                 # 62 blocks
    assert 'fir4x4/TR4' in fir(1, 64, 257, 255)                                         # 1,048,560 quads: 16 short of 2^20
    assert 'fir4x4/TR8' in fir(1, 64, 257, 257)
    assert 'fir4x4/TR8' in fir(4, 32, 257, 131)                                         # test_upfirdn2d_up_layer_fir_register_tiled's large shape
    assert 'fir4x4/TR4' in fir(1, 8, 8, 8) and 'nhwc4' in fir(1, 8, 7, 9)
    assert 'planar/stride_loop' in R.upfirdn_paths(R.uf_case('probe', (1, 3, 841, 841)))
    assert 'planar/single_round' in R.upfirdn_paths(R.uf_case('probe', (1, 2, 1025, 1025)))        # 2,097,152 outputs: exactly the capped grid


def test_upfirdn_cross_is_full_and_every_layout_meets_every_factor_value():
    cross = [c for c in R.UPFIRDN_CASES if c['group'].startswith('cross-')]
    keys = {(c['up'], c['down'], c['filt'], c['pad'], c['flip'], c['gain']) for c in cross}
    assert len(keys) == len(cross) == len(R.UPDOWN) * len(R.FILTERS) * len(R.PADS) * 2 * len(R.GAINS)
    forms = {(c['layout'], c['shape'][1]) for c in cross}
    assert {l for l, _ in forms} == set(R.LAYOUTS)
    for form in forms:
        mine = [c for c in cross if (c['layout'], c['shape'][1]) == form]
        assert {c['filt'] for c in mine} == set(R.FILTERS) and {c['pad'] for c in mine} == set(R.PADS.values()), form
        assert {(c['up'], c['down']) for c in mine} == set(R.UPDOWN) and {c['flip'] for c in mine} == {False, True}, form
        assert {c['gain'] for c in mine} == set(R.GAINS), form
    assert all(u in (1, 2, 3) for ud in R.UPDOWN for pair in ud for u in pair)
    assert any((c['shape'][2] * c['up'][1] + c['pad'][2] + c['pad'][3] - R.filter_size(c['filt'])[1]) % c['down'][1] for c in cross)      # a remainder in the backward's pad formula


def test_demod_table_has_every_value_of_every_factor():
    for key, vals in (('B', R.DEMOD_B), ('I', R.DEMOD_I), ('O', R.DEMOD_O), ('K', R.DEMOD_K), ('layout', R.DEMOD_LAYOUTS)):
        assert {c[key] for c in R.DEMOD_CASES} >= set(vals), key
    assert {(c['B'], c['I']) for c in R.DEMOD_CASES} >= {(B, I) for B in R.DEMOD_B for I in R.DEMOD_I}
    for B in R.DEMOD_B:
        assert {c['layout'] for c in R.DEMOD_CASES if c['B'] == B} == set(R.DEMOD_LAYOUTS), B
    assert sum(c['zero_row'] is not None for c in R.DEMOD_CASES) >= 1
    assert all(c['B'] * c['O'] * c['I'] * c['K'] ** 2 <= R.DEMOD_REF_MAX for c in R.DEMOD_CASES)


def test_layouts_are_what_the_predicate_assumes():
    """build_input makes the strides and the offset layout_geometry reports, with the values of the dense tensor."""
    for shape in (R.BASE_SHAPE, R.BASE_SHAPE_C6):
        x = torch.randn(shape)
        for layout in R.LAYOUTS:
            xv = x[0:1].expand(shape).contiguous() if layout == 'nchw_expanded' else x
            v = R.build_input(xv, layout)
            _, _, off, st = R.layout_geometry(shape, layout)
            assert tuple(v.stride()) == tuple(st) and v.storage_offset() == off and torch.equal(v, xv), (shape, layout)


# ------------------------------------------------------------------------------------------------------------------------ references
DIRECT_CASES = [R.uf_case('direct-a', (2, 3, 5, 6), filt='4x4', up=(2, 1), down=(1, 3), pad=(3, 0, -1, 2), flip=False, gain=1.5),
                R.uf_case('direct-b', (1, 2, 6, 5), filt='sep8', up=(3, 2), down=(2, 3), pad=(2, 5, 4, 3), flip=True, gain=4.0)]


@pytest.mark.parametrize('c', DIRECT_CASES, ids=[c['name'] for c in DIRECT_CASES])
def test_upfirdn_reference_equals_the_quadruple_loop(c):
    for exact in (False, True):
        x, _ = R.uf_inputs(c, exact)
        f = R.make_filter(c['filt'], exact)
        a = R.upfirdn_ref(x, f, c['up'], c['down'], c['pad'], c['flip'], c['gain'])
        b = R.upfirdn_direct(x, f, c['up'], c['down'], c['pad'], c['flip'], c['gain'])
        assert a.shape == b.shape
        assert R.rel_err(a, b) <= (0.0 if exact else 1e-13)
    # with the gain inside, as ops_ref applies it (gain ** (ndim / 2) on the taps), the same to rounding
    x, _ = R.uf_inputs(c, False)
    f = R.make_filter(c['filt'], False)
    inside = R.ops_ref.upfirdn2d(x.double(), f.double(), up=c['up'], down=c['down'], padding=list(c['pad']), flip_filter=c['flip'], gain=c['gain'])
    assert R.rel_err(inside, R.upfirdn_ref(x, f, c['up'], c['down'], c['pad'], c['flip'], c['gain'])) <= 1e-13


def test_exact_inputs_make_float32_and_float64_agree_to_zero():
    """Integers in [-8, 8], dyadic taps, gains 4 and 1.5: every partial sum is a float32, so the float32 oracle equals the float64 one."""
    for c in R.UPFIRDN_CASES[::7] + R.UPFIRDN_CASES[-7:]:
        if max(c['shape']) > 300:
            continue
        y64, dx64, _ = R.uf_reference_cached(c['name'], True)
        y32, dx32, _ = R.uf_reference(c, True, R.F32)
        assert torch.equal(y32.double(), y64) and torch.equal(dx32.double(), dx64), c['name']
        assert bool((y64 != 0).any()) and bool((dx64 != 0).any())


def test_demod_reference_equals_the_w2_form():
    for c in R.DEMOD_CASES[::3] + R.DEMOD_CASES[-4:]:
        w, s, g, _ = R.demod_inputs(c)
        for a, b, what in zip(R.demod_reference_cached(c['name']), R.demod_w2_ref(w, s, g), ('dcoefs', 'dweight', 'dstyles')):
            assert R.rel_err(a, b) <= 1e-13, (c['name'], what)
        if c['zero_row'] is not None:
            d, _, ds = R.demod_reference_cached(c['name'])
            assert bool((d[c['zero_row']] == R.as_f32(R.DEMOD_EPS) ** -0.5).all()) and not bool(ds[c['zero_row']].any())


def test_resample_reference_equals_pillow():
    Image = pytest.importorskip('PIL.Image')
    for c in R.RESIZE_CASES:
        imgs = R.resize_inputs(c)
        u8, chw = R.resize_reference_cached(c['name'])
        for i in range(c['n']):
            pil = np.asarray(Image.fromarray(imgs[i]).resize((c['out_w'], c['out_h']), Image.LANCZOS))
            assert np.array_equal(pil, u8[i]), (c['name'], i)
        assert chw.dtype == np.float32 and chw.shape == (c['n'], 3, c['out_h'], c['out_w'])


def test_resize_tap_counts_at_the_unrolled_branch():
    for name, taps, used in (('taps31', 31, 30), ('taps33', 33, 30), ('taps33-32-used', 33, 32)):
        c = R.RESIZE_BY_NAME[name]
        bounds, _, ks = resample_ref.precompute_coeffs(c['H'], c['out_h'])
        assert ks == taps and bounds[:, 1].max() == used, name          # the window, and the taps the middle rows use of it


# ------------------------------------------------------------------------------------------------------------------------ wrong references
def test_wrong_references_are_caught_at_the_gpu_bounds():
    """A float32 evaluation that is wrong in one of three ways misses the bound the GPU file uses, where the right one is inside it."""
    picks = [next(c for c in R.UPFIRDN_CASES if c['filt'] == filt and (c['up'], c['down']) == R.UPDOWN[ud] and c['flip'] == flip)
             for filt, ud, flip in (('4x4', 0, False), ('sep8', 1, True))]
    for c in picks:
        name = c['name']
        y64, _, _ = R.uf_reference_cached(name, False)
        assert R.rel_err(R.uf_reference(c, False, R.F32)[0], y64) <= R.fp32_bound('upfirdn_y')
        not_flipped = R.uf_reference(dict(c, flip=not c['flip']), False, R.F32)[0]
        twice = R.uf_reference(c, False, R.F32)[0] * c['gain']
        for wrong, what in ((not_flipped, 'filter not flipped'), (twice, 'gain applied twice')):
            assert R.rel_err(wrong, y64) > R.fp32_bound('upfirdn_y') and R.elem_rel_err(wrong, y64) > R.fp32_bound('upfirdn_y_elem'), (name, what)
    zero = [c for c in R.DEMOD_CASES if c['zero_row'] is not None]
    assert zero
    for c in zero:
        w, s, g, _ = R.demod_inputs(c)
        d64 = R.demod_reference_cached(c['name'])[0]
        assert R.elem_rel_err(R.demod_w2_ref(w, s, g, R.F32)[0], d64) <= R.fp32_bound('demod_d_elem')
        no_eps = R.demod_w2_ref(w, s, g, R.F32, eps=0.0)[0]
        assert not R.elem_rel_err(no_eps, d64) <= R.fp32_bound('demod_d_elem'), c['name']


# ------------------------------------------------------------------------------------------------------------------------ yardstick
def test_fp32_baseline_is_what_this_machine_measures():
    got = R.measure_fp32_baselines()
    for key, recorded in R.FP32_BASELINE.items():
        print(f'[resampling] {key}: recorded {recorded:.3e}, measured {got[key]:.3e}')
    for key, recorded in R.FP32_BASELINE.items():
        assert got[key] / 4.0 <= recorded <= got[key] * 4.0, f'{key}: recorded {recorded:.3e}, measured {got[key]:.3e}'
    for key, project in R.PROJECT_BOUND.items():
        assert R.fp32_bound(key) <= project
