"""ldetr_sg2_handoff_f32 (csrc/misc_ops.hip), the element-wise chain between two contraction launches of the StyleGAN2 synthesis
backward, against a float64 torch evaluation of its formulas on seeded inputs.  Bounds are those of the layer test for the same
quantities (test_modulated_conv_layers_vs_oracle): 5e-5 for dv and the bias sums, 1e-4 for the style and demodulation sums, relative
to the reference's largest magnitude."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA, GAIN = 0.2, math.sqrt(2)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def assert_close(a, b, tol, what=''):
    e = rel_err(a, b)
    assert e <= tol, f'{what}: rel err {e:.3e} > {tol:.1e}'


def _inputs(B, P, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(B, P, C)
    x = torch.where(x.abs() < 1e-3, torch.full_like(x, 0.5), x)          # away from zero: both evaluations take the same slope
    return dict(dxs=r(B, P, C), x=x, dy=r(B, P, 3), s_conv=r(B, C) * 0.5 + 1.0, s_rgb=r(B, C) * 0.5 + 1.0, w_rgb=r(3, C) / math.sqrt(C),
                bias=r(C) * 0.1, demod=r(B, C).abs() + 0.5,
                # starting values of the accumulation targets: the kernel adds to what is there
                ds_conv0=r(B, C), dws0=r(B, 3, C), dbias_rgb0=r(3), dbias0=r(C), ddemod0=r(B, C))


def _reference(t, conv, rgb):
    d = {k: v.double() for k, v in t.items()}
    x = d['x']
    g = torch.zeros_like(x)
    out = {}
    if conv:
        g = g + d['dxs'] * d['s_conv'][:, None, :]
        out['ds_conv'] = d['ds_conv0'] + (d['dxs'] * x).sum(1)
    if rgb:
        g = g + d['s_rgb'][:, None, :] * torch.einsum('bpk,kc->bpc', d['dy'], d['w_rgb'])
        out['dws'] = d['dws0'] + torch.einsum('bpk,bpc->bkc', d['dy'], x)
        out['dbias_rgb'] = d['dbias_rgb0'] + d['dy'].sum((0, 1))
    pos = x > 0
    dv = g * torch.where(pos, GAIN, GAIN * ALPHA)
    pre = x / torch.where(pos, GAIN, GAIN * ALPHA)
    out['dv'] = dv
    out['dbias'] = d['dbias0'] + dv.sum((0, 1))
    out['ddemod'] = d['ddemod0'] + (dv * (pre - d['bias'])).sum(1) / d['demod']
    return out


def _run(dev, t, conv, rgb, alias):
    from layoutdetr_amd.hip import core
    c = {k: v.to(dev).contiguous() for k, v in t.items()}
    dxs = c['dxs'].clone() if conv else None
    dv = dxs if (conv and alias) else torch.empty_like(c['x'])
    ds_conv, dws, dbias_rgb, dbias, ddemod = [c[k].clone() for k in ('ds_conv0', 'dws0', 'dbias_rgb0', 'dbias0', 'ddemod0')]
    p = core.ptr
    core.check(core.lib().ldetr_sg2_handoff_f32(p(dxs), p(c['x']), p(c['dy']) if rgb else None, p(dv), p(c['s_conv']) if conv else None,
                                                p(c['s_rgb']) if rgb else None, p(c['w_rgb']) if rgb else None, p(c['bias']), p(c['demod']),
                                                p(ds_conv) if conv else None, p(dws) if rgb else None, p(dbias_rgb) if rgb else None, p(dbias),
                                                p(ddemod), c['x'].shape[0], c['x'].shape[1], c['x'].shape[2], ALPHA, GAIN, core.stream()), 'sg2_handoff')
    torch.cuda.synchronize()
    if conv and not alias:
        assert torch.equal(dxs, c['dxs']), 'dxs was written although dv does not alias it'
    return dict(dv=dv, ds_conv=ds_conv, dws=dws, dbias_rgb=dbias_rgb, dbias=dbias, ddemod=ddemod)


def _check(got, ref, conv, rgb):
    assert_close(got['dv'], ref['dv'], 5e-5, 'dv')
    assert_close(got['dbias'], ref['dbias'], 5e-5, 'dbias')
    assert_close(got['ddemod'], ref['ddemod'], 1e-4, 'ddemod')
    if conv:
        assert_close(got['ds_conv'], ref['ds_conv'], 1e-4, 'ds_conv')
    if rgb:
        assert_close(got['dws'], ref['dws'], 1e-4, 'dws_rgb')
        assert_close(got['dbias_rgb'], ref['dbias_rgb'], 5e-5, 'dbias_rgb')


MODES = [(True, True), (True, False), (False, True)]          # (conv gradient present, rgb gradient present)
# C = 4: one quad, 256 row lanes; 32; 512: two row lanes; 1028: a second channel chunk with one active quad.
# P = 1; 37: no multiple of the four-row trip; B = 2, P = 8192, C = 32: 2048 blocks share the bias sum -> partial-sum workspace + finish launch.
SHAPES = [(1, 1, 4), (3, 37, 4), (1, 37, 32), (3, 1, 32), (3, 37, 512), (1, 37, 1028), (3, 5, 1028), (2, 8192, 32)]


@pytest.mark.parametrize('conv,rgb', MODES)
@pytest.mark.parametrize('B,P,C', SHAPES)
def test_handoff_vs_float64(dev, B, P, C, conv, rgb):
    t = _inputs(B, P, C, seed=1000 + B * 7 + P + C)
    ref = _reference(t, conv, rgb)
    for alias in ((True, False) if conv else (False,)):
        _check(_run(dev, t, conv, rgb, alias), ref, conv, rgb)


def test_handoff_without_demod_sum_or_bias(dev):
    """ddemod is optional, and a layer without a bias has bias = NULL (= 0)."""
    from layoutdetr_amd.hip import core
    t = _inputs(2, 37, 32, seed=7)
    ref = _reference(dict(t, bias=torch.zeros(32)), True, False)
    c = {k: v.to(dev).contiguous() for k, v in t.items()}
    p = core.ptr
    for with_dd in (True, False):
        dv = torch.empty_like(c['x']); ds, db, dd = c['ds_conv0'].clone(), c['dbias0'].clone(), c['ddemod0'].clone()
        core.check(core.lib().ldetr_sg2_handoff_f32(p(c['dxs']), p(c['x']), None, p(dv), p(c['s_conv']), None, None, None, p(c['demod']) if with_dd else None,
                                                    p(ds), None, None, p(db), p(dd) if with_dd else None, 2, 37, 32, ALPHA, GAIN, core.stream()), 'sg2_handoff')
        assert_close(dv, ref['dv'], 5e-5, 'dv'); assert_close(db, ref['dbias'], 5e-5, 'dbias'); assert_close(ds, ref['ds_conv'], 1e-4, 'ds_conv')
        if with_dd:
            assert_close(dd, ref['ddemod'], 1e-4, 'ddemod')
        else:
            assert torch.equal(dd, c['ddemod0'])


def test_handoff_rejects_bad_arguments(dev):
    from layoutdetr_amd.hip import core
    x = torch.zeros(1, 4, 6, device=dev)
    with pytest.raises(RuntimeError):
        core.check(core.lib().ldetr_sg2_handoff_f32(None, core.ptr(x), None, core.ptr(x), None, None, None, None, None, None, None, None, core.ptr(x), None,
                                                    1, 4, 8, ALPHA, GAIN, core.stream()), 'sg2_handoff')     # neither gradient
    with pytest.raises(RuntimeError):
        core.check(core.lib().ldetr_sg2_handoff_f32(core.ptr(x), core.ptr(x), None, core.ptr(x), core.ptr(x), None, None, None, None, core.ptr(x), None, None,
                                                    core.ptr(x), None, 1, 4, 6, ALPHA, GAIN, core.stream()), 'sg2_handoff')     # C no multiple of 4
