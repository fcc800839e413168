"""The CPU half of the plane-format conv engine's parity suite (tests/p3_engine_common.py, tests/test_p3_engine_gpu.py): no GPU, no kernel library.

It proves what the GPU file relies on: every path name is reached by a table case and none is unknown; the policy model agrees with the launch records
tests/test_p3_gpu.py already holds for the bench shapes and with a brute-force statement of the patch conditions; the float64 references equal
F.conv2d and its autograd (and a naive loop on three tiny cases); the exact classes' preconditions hold, so that "bit for bit" is a fair demand; twelve
deliberately wrong references are rejected at the GPU file's bars; and the float32 yardsticks in FP32_BASELINE are what this machine measures."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import p3_engine_common as P

P.limit_threads()
F64, F32 = P.F64, P.F32


def _whiches(c):
    return (0, 1) if c['entry'] == 'dual' else (0,)


# ------------------------------------------------------------------------------------------------------------------------ paths and the model
def test_every_path_is_reached_and_none_is_unknown():
    seen = set()
    for c in P.ALL_CASES:
        f, paths = P.model(c)
        unknown = [p for p in paths if p not in P.P3_PATHS]
        assert not unknown, (c['name'], unknown)
        assert not [p for p in paths if p in P.P3_UNREACHABLE], c['name']
        seen |= set(paths)
    seen |= {'reject/' + r['name'] for r in P.REJECT_CASES}
    assert sorted(set(P.P3_PATHS) - seen) == []
    assert not set(P.P3_UNREACHABLE) & set(P.P3_PATHS)
    # every epilogue branch on both kernels, every cold path at the tile it names
    assert P.model(P.BY_NAME['k_nt128'])[0]['bm'] == 128 and P.model(P.BY_NAME['k_nt64'])[0]['bm'] == 64


def test_table_cases_pass_the_entry_checks_and_reject_cases_do_not():
    for c in P.ALL_CASES:
        assert P.entry_accepts(c['entry'], c['geom']), c['name']
    for r in P.REJECT_CASES:
        assert not P.entry_accepts(r['entry'], r['geom'], r['null'], r['oh_delta']), r['name']
    # each reject case differs from an accepted call in the one clause it names
    assert P.entry_accepts('fwd', P._RB) and P.entry_accepts('dual', P._RB) and P.entry_accepts('dgrad', P._RB) and P.entry_accepts('wgrad', P._RB) and P.entry_accepts('pair', P._RB)


def test_model_gives_the_launch_records_of_the_bench_shapes():
    import test_p3_gpu as old
    for N, H, W, Ci, Co, k, s, pad, want in old.BENCH_FWD_CASES:
        f, _ = P.model_fwd((N, H, W, Ci, Co, k, k, s, pad))
        for key, v in want.items():
            assert v(f[key]) if callable(v) else f[key] == v, ((N, H, W, Ci, Co, k, s, pad), key, f)
    for geom, kind in old.BENCH_PAIR_KIND.items():
        N, H, W, Ci, Co, k, s, pad = geom
        f, _ = P.model_pair((N, H, W, Ci, Co, k, k, s, pad))
        assert f['kind'] == kind and f['ncls'] == (s * s if (s > 1 and kind == 4) else 1), (geom, f)
    # test_p3_gpu.py's FWD_CASES names 2 x 4 x 4 x 512 -> 64 a patch-kernel case ("many images per tile"): it is not (NG = 18 > 13)
    assert P.c3_geometry(2, 4, 4) == (None, 'NG_gt_13') and P.model_fwd((2, 4, 4, 512, 64, 3, 3, 1, 1))[0]['kind'] == 1


def test_c3_geometry_model_against_the_patch_conditions():
    for H, W in itertools.product(range(1, 65), repeat=2):
        g, why = P.c3_geometry(3, H, W)
        want = P.c3_geometry_brute(H, W)
        assert (None if g is None else (g['PW'], g['PH'], g['NP'])) == want, (H, W, g, why, want)
        if g:
            assert g['mtiles'] == -(-3 * g['ppi'] // g['NP']) and g['NG'] <= 13
    assert P.c3_accepted_geometries() == sorted(P.C3_GEOMETRIES)
    assert ['c3/geom/%dx%dx%d' % g for g in P.C3_GEOMETRIES] == [p for p in P.P3_PATHS if p.startswith('c3/geom/')]


# ------------------------------------------------------------------------------------------------------------------------ references
def _nchw(v):
    return v.permute(0, 3, 1, 2)


def _torch_outputs(c, t, which):
    """float64 F.conv2d and its autograd: the contraction of every output family, before the epilogue."""
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    out = {}
    if c['entry'] in ('fwd', 'dual'):
        out['y'] = F.conv2d(_nchw(t['x'].double()), _nchw(t['w'].double()), stride=s, padding=pad).permute(0, 2, 3, 1)
        return out
    dy = t['dy']
    x = t['x'] if 'x' in t else torch.zeros(N, H, W, Ci)
    w = t['w'] if 'w' in t else torch.zeros(Co, KH, KW, Ci)
    if c['name'] == 'w_big_pixel_index':      # images whose dY is zero add nothing: F.conv2d on the others
        keep = (dy.reshape(N, -1) != 0).any(1)
        dy, x = dy[keep], x[keep]
    w64 = w.double()
    if c['row_scale'] and c['entry'] != 'wgrad':
        w64 = (w.double() * t['row_scale'].double()[:, None, None, None]).float().double()
    xd = _nchw(x.double()).clone().requires_grad_(True)
    wd = _nchw(w.double()).clone().requires_grad_(True)
    gx, = torch.autograd.grad(F.conv2d(xd, _nchw(w64), stride=s, padding=pad), xd, _nchw(dy.double()))
    gw, = torch.autograd.grad(F.conv2d(xd.detach(), wd, stride=s, padding=pad), wd, _nchw(dy.double()))
    out['dx'], out['dw'] = gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1)
    return out


@pytest.mark.parametrize('name', [c['name'] for c in P.VALUE_CASES])
def test_references_equal_float64_conv2d_and_autograd(name):
    c = P.BY_NAME[name]
    cls = 'rounding' if 'rounding' in c['classes'] else c['classes'][0]
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    for which in _whiches(c):
        t = P.inputs(name, cls, which)
        th = _torch_outputs(c, t, which)
        if c['entry'] in ('fwd', 'dual'):
            acc, S = P.conv_fwd_ref(t['x'], t['w'], s, pad)
            assert (acc - th['y']).abs().max() <= 1e-12 * S.max()
            assert (S >= acc.abs() * (1 - 1e-12)).all()
        if c['entry'] in ('dgrad', 'pair'):
            w = t['w'].double()
            if c['row_scale']:
                w = (w * t['row_scale'].double()[:, None, None, None]).float().double()
            acc, S = P.conv_dgrad_ref(t['dy'], w, s, pad, H, W)
            assert (acc - th['dx']).abs().max() <= 1e-12 * S.max().clamp_min(1e-300)
        if c['entry'] in ('wgrad', 'pair'):
            acc, S = P.conv_wgrad_ref(t['x'], t['dy'], KH, KW, s, pad)
            assert (acc - th['dw']).abs().max() <= 1e-12 * S.max().clamp_min(1e-300)


def _naive(x, w, s, pad):
    N, H, W, Ci = x.shape
    Co, KH, KW, _ = w.shape
    OH, OW = P.out_hw(H, W, KH, KW, s, pad)
    y = torch.zeros(N, OH, OW, Co, dtype=F64)
    for n, oy, ox, co, kh, kw in itertools.product(range(N), range(OH), range(OW), range(Co), range(KH), range(KW)):
        iy, ix = oy * s - pad + kh, ox * s - pad + kw
        if 0 <= iy < H and 0 <= ix < W:
            y[n, oy, ox, co] += float((x[n, iy, ix].double() * w[co, kh, kw].double()).sum())
    return y


@pytest.mark.parametrize('geom', [(1, 4, 5, 3, 2, 3, 3, 1, 1), (2, 3, 5, 2, 3, 1, 3, 1, 0), (1, 5, 6, 2, 2, 3, 3, 2, 1)], ids=['3x3', '1x3', 'stride2'])
def test_references_equal_a_naive_loop(geom):
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, KH, KW, Ci, generator=g)
    y = _naive(x, w, s, pad)
    assert (P.conv_fwd_ref(x, w, s, pad)[0] - y).abs().max() < 1e-13
    # the gradients through the same loop: <dy, conv(x, w)> is linear in x and in w
    dy = torch.randn(y.shape, generator=g)
    dx, _ = P.conv_dgrad_ref(dy, w, s, pad, H, W)
    dw, _ = P.conv_wgrad_ref(x, dy, KH, KW, s, pad)
    for i in range(0, x.numel(), 7):
        e = torch.zeros(x.numel()); e[i] = 1
        assert abs(float((_naive(e.reshape(x.shape), w, s, pad) * dy.double()).sum()) - float(dx.reshape(-1)[i])) < 1e-12
    for i in range(0, w.numel(), 5):
        e = torch.zeros(w.numel()); e[i] = 1
        assert abs(float((_naive(x, e.reshape(w.shape), s, pad) * dy.double()).sum()) - float(dw.reshape(-1)[i])) < 1e-12


# ------------------------------------------------------------------------------------------------------------------------ exactness
def _exact_cases(cls):
    return [c['name'] for c in P.VALUE_CASES if cls in c['classes']]


@pytest.mark.parametrize('name', _exact_cases('grid'))
def test_grid_preconditions(name):
    """sum |terms| in units of the quantum below 2^24 for every output, operands within 16 significant bits, and an fp32 evaluation in reversed
    order of the reduction gives the float64 bits."""
    c = P.BY_NAME[name]
    for which in _whiches(c):
        t = P.inputs(name, 'grid', which)
        for k in ('x', 'w', 'dy'):
            if k in t:
                hi, mid, lo = P.bf16_planes(t[k])
                assert bool((lo == 0).all()) and bool((mid != 0).any()), k
        ref = P.reference(name, 'grid', which)
        quantum = 1.0
        for fam, (v, pre, S) in ref.items():
            assert float(S.max()) / quantum < 2 ** 24, (fam, float(S.max()))
            assert bool((v == v.round()).all())
        revs = {}
        if c['entry'] in ('fwd', 'dual'):
            revs['y'] = dict(t, x=t['x'].flip(-1), w=t['w'].flip(-1))                       # the channels of every tap in reversed order
        if c['entry'] in ('dgrad', 'pair'):
            revs['dx'] = dict(t, dy=t['dy'].flip(-1), w=t['w'].flip(0))                    # the output channels in reversed order
            if c['row_scale']:
                revs['dx']['row_scale'] = t['row_scale'].flip(0)
        if c['entry'] in ('wgrad', 'pair'):
            revs['dw'] = dict(t, dy=t['dy'].flip(0), x=t['x'].flip(0))                     # the images in reversed order
        for fam, (v, pre, S) in ref.items():
            assert P.bit_equal(P.case_outputs(c, revs[fam], F32, which=which)[fam][0], v) == 0, fam


@pytest.mark.parametrize('name', sorted(set(_exact_cases('select') + _exact_cases('select_w'))))
def test_select_preconditions(name):
    """At most one non-zero product per output, finite, and the one additive term (if any) close enough in exponent for the float64 sum to be exact."""
    c = P.BY_NAME[name]
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    for cls in [k for k in ('select', 'select_w') if k in c['classes']]:
        for which in _whiches(c):
            t = P.inputs(name, cls, which)
            nz = {k: (v != 0).double() for k, v in t.items() if k in ('x', 'w', 'dy')}
            e = c['epi2'] if (which == 1 and c['epi2'] is not None) else c['epi']
            assert P.additive_terms(e) <= 1
            counts = []
            if c['entry'] in ('fwd', 'dual'):
                counts.append(P.conv_fwd_ref(nz['x'], nz['w'], s, pad)[0])
            if c['entry'] in ('dgrad', 'pair'):
                counts.append(P.conv_dgrad_ref(nz['dy'], nz['w'], s, pad, H, W)[0])
            if c['entry'] in ('wgrad', 'pair'):
                counts.append(P.conv_wgrad_ref(nz['x'], nz['dy'], KH, KW, s, pad)[0])
            for cnt in counts:
                assert float(cnt.max()) == 1.0, float(cnt.max())
            ref = P.reference(name, cls, which)
            bare = P.case_outputs(c, {k: (torch.zeros_like(v) if k in ('bias', 'res_p3', 'res_f32', 'dw0') else v) for k, v in t.items()}, F64, which=which)
            for fam, (v, pre, S) in ref.items():
                assert bool(torch.isfinite(v).all()) and float(S.max()) < P.FLT_MAX
                assert float((v != 0).double().mean()) > 0.02, 'almost every output is zero: the case pins nothing'
                full = v if pre is None else pre
                base = bare[fam][0] if pre is None else bare[fam][1]
                assert bool((base.float().double() == base).all()), 'the product alone is no fp32 number'
                added = [t[k].double() for k in (('dw0',) if fam == 'dw' else ('bias', 'res_p3', 'res_f32')) if k in t]
                assert len(added) <= 1
                if added:      # the float64 sum of the product and the one additive term is exact: taking the term away again gives the product
                    assert torch.equal(full - added[0], base), 'the float64 sum rounded'


def test_rounding_inputs_cut_about_half_and_few_sit_on_the_edge():
    for c in P.rounding_cases():
        for which in _whiches(c):
            e = c['epi2'] if (which == 1 and c['epi2'] is not None) else c['epi']
            ref = P.reference(c['name'], 'rounding', which)
            K = P.reduction_length(c)
            for fam, (v, pre, S) in ref.items():
                share = P.near_zero_share(pre if (e['relu'] and fam != 'dw') else None, S, P.bound(fam, K[fam], elem=True))
                assert share < 0.01, (c['name'], fam, share)
                if fam != 'dw' and (e['relu'] or e['mask']):
                    cut = float((v == 0).double().mean())
                    assert 0.25 < cut < 0.85, (c['name'], fam, cut)


# ------------------------------------------------------------------------------------------------------------------------ wrong references
WRONG = [
    # mutation, case, class that must reject it
    ('drop_tap_at_border', 'f_3x3_nonpatch', 'select'), ('drop_tap_at_border', 'f_3x3_nonpatch', 'rounding'),
    ('pad_minus_1', 'f_3x3p2', 'select'), ('pad_minus_1', 'f_3x3p2', 'rounding'),
    ('swap_khkw', 'f_1x3', 'select'), ('swap_khkw', 'f_4x8p3', 'rounding'),
    ('swap_parity', 'd_s2_3x3_odd', 'select'), ('swap_parity', 'd_s2_3x3_odd', 'rounding'),
    ('last_pixel_tile_missing', 'w_lt8_C96', 'rounding'), ('last_pixel_tile_missing', 'w_lt8_C96', 'grid'),
    ('alpha_omitted', 'e_nt_alpha_f32', 'select'), ('alpha_omitted', 'e_c3_full', 'rounding'),
    ('scale_8_channels_off', 'e_nt_scale_p3', 'select'), ('scale_8_channels_off', 'e_c3_scale_bias_resp3', 'rounding'),
    ('relu_before_residual', 'e_nt_full', 'grid'), ('relu_before_residual', 'e_c3_full', 'rounding'),
    ('mask_from_y', 'e_nt_resf32_mask', 'select'), ('mask_from_y', 'e_c3_full', 'rounding'),
    ('no_mid_mid', 'f_3x3_nonpatch', 'grid'), ('no_mid_mid', 'c_8x8x2_half', 'grid'),
    ('no_hi_lo', 'f_3x3_nonpatch', 'select_w'), ('no_hi_lo', 'c_8x8x2_half', 'select_w'),
    ('no_mid_mid', 'f_3x3_nonpatch', 'rounding'), ('no_hi_lo', 'f_3x3_nonpatch', 'rounding'),
    ('unused_row_copies_neighbour', 'd_s2_2x2_border', 'select'), ('unused_row_copies_neighbour', 'd_s2_2x2_border', 'rounding'),
]


@pytest.mark.parametrize('mut,name,cls', WRONG, ids=['%s-%s-%s' % w for w in WRONG])
def test_wrong_references_are_rejected_at_the_gpu_bars(mut, name, cls):
    c = P.BY_NAME[name]
    t = P.inputs(name, cls)
    ref = P.reference(name, cls)
    bad = P.case_outputs(c, t, F64, mut=mut)
    K = P.reduction_length(c)
    rejected = False
    for fam, (v, pre, S) in ref.items():
        got = bad[fam][0].float()          # what a kernel computing the wrong thing would store
        if cls == 'rounding':
            rejected |= P.rel_err(got, v, S) > P.bound(fam, K[fam]) or P.elem_rel_err(got, v, S) > P.bound(fam, K[fam], elem=True)
        else:
            rejected |= P.bit_equal(got, v) > 0
    assert rejected


# ------------------------------------------------------------------------------------------------------------------------ yardsticks
def test_fp32_baselines_are_what_this_machine_measures():
    got = P.measure_fp32_baselines()
    print('measured:', {k: float('%.3g' % v) for k, v in sorted(got.items())})
    assert set(got) == set(P.FP32_BASELINE)
    for k, v in got.items():
        assert P.FP32_BASELINE[k] / 1.5 <= v <= P.FP32_BASELINE[k] * 1.5, (k, v, P.FP32_BASELINE[k])
    # FP32_FACTOR x yardstick against the project's older ceiling: where it is above, the ceiling is the bound (P.bound takes the smaller) and the bucket is named
    above = [k for k, v in P.FP32_BASELINE.items() if '_elem' not in k and P.FP32_FACTOR * v >= P.PROJECT_BOUND[k.split('/')[0]]]
    assert sorted(above) == sorted(P.YARDSTICK_ABOVE_CEILING)
    for fam, K in (('y', 4608), ('dx', 1024)):
        assert P.bound(fam, K) == P.PROJECT_BOUND[fam]
