"""Every path of the FIR resampling kernels (csrc/upfirdn2d.hip), the demodulation coefficients (csrc/demod.hip) and the page resize
(csrc/resample.hip) against float64.  Tables, references and the path predicates are in tests/resampling_common.py;
tests/test_resampling_ref_cpu.py proves that the tables reach every path and that the references are right.

upfirdn2d: every table case runs twice.  Exact: integer inputs and dyadic taps, where every partial sum is a float32, so y and dx must EQUAL the
float64 reference whatever the order of summation (a wrong tap, a wrong index, a missed or repeated store all show).  Rounding: positive random
inputs, y and dx within 4 x the float32 yardstick, max-normalised and element by element.  Cases marked 'abi' call ldetr_upfirdn2d_f32 themselves
with the output NaN-filled and a NaN guard band behind it; the others go through torch_utils.ops.upfirdn2d.  dx always comes from the autograd
Function, with the upstream gradient in the memory format of y.  One case runs the backward of the backward; the same data through fir4x4 and the
planar kernel must agree bit for bit (the claim of the kernel's comment).

demod: ldetr_demod_fwd_f32 / ldetr_demod_bwd_f32 with NaN-filled outputs on every case with B <= 64: gradients stored, summed into a non-zero
buffer, each alone; B = 65 through demod_coefs' GEMM form.  Page resize: ldetr_resize_normalize_u8 with prefilled outputs, bit-equal to
oracle.resample_ref (which the CPU file pins to Pillow).  Every case prints its figures before it asserts.

Largest measured errors (MI355X; float32 yardstick; bound): upfirdn y 2.4e-7 (2.4e-7; 9.5e-7), element-wise 3.7e-7 (3.7e-7; 1.5e-6); dx 2.4e-7
(2.5e-7; 1.0e-6), element-wise 3.6e-7 (3.7e-7; 1.5e-6); fused epilogue 1.8e-7 (1.7e-7; 6.9e-7); second order 1.1e-7 (1.1e-7; 4.5e-7); fir4x4 against
the planar kernel 0.0: the comment's claim holds, with and without the epilogue.  demod dcoefs 1.6e-7 (3.9e-7; 1.5e-6), element-wise 2.1e-7
(4.9e-7; 2.0e-6); dweight 4.6e-7 (4.4e-7; 1.8e-6), element-wise 5.5e-7 (1.0e-6; 4.1e-6); dstyles 3.0e-7 (7.9e-7; 3.2e-6), element-wise 5.3e-7
(1.2e-6; 4.6e-6); W2 2.6e-7 (6.0e-7 for nine taps).  Every exact case equal, the page resize bit-equal.  160 tests over 400 upfirdn, 45 demod and
15 resize cases in 9.6 s, the slowest 1.1 s (the first, which loads the library; then the 1026 x 1026 stride-loop case, 1.1 s)."""
import ctypes

import numpy as np
import pytest
import torch

import resampling_common as R

pytestmark = pytest.mark.gpu

R.limit_threads()
GUARD = 4096          # floats of NaN behind an output
NAN = float('nan')


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


class Figures(object):
    """Collects (name, error, bound) and exact conditions, prints each, asserts them together at the end of a test."""

    def __init__(self):
        self.rows, self.flags = [], []

    def value(self, case, name, e, tol):
        self.rows.append((case, name, e, tol))

    def both(self, case, key, a, b, elem=True):
        self.value(case, key, R.rel_err(a, b), R.fp32_bound(key))
        if elem:
            self.value(case, key + '_elem', R.elem_rel_err(a, b), R.fp32_bound(key + '_elem'))

    def exact(self, case, name, ok):
        self.flags.append((case, name, bool(ok)))

    def check(self):
        for case, name, e, tol in self.rows:
            print(f'[resampling] {case}: {name} err {e:.3e} (bound {tol:.2e})')
        bad = [f'{case} {name}: {e:.3e} > {tol:.2e}' for case, name, e, tol in self.rows if not e <= tol] + \
              [f'{case} {name}: not exact' for case, name, ok in self.flags if not ok]
        for b in bad:
            print('[resampling] FAILED ' + b)
        assert not bad, '; '.join(bad[:12]) + (f' (+{len(bad) - 12} more)' if len(bad) > 12 else '')


# ------------------------------------------------------------------------------------------------------------------------ upfirdn2d
def abi_upfirdn(xv, f2d, up, down, pad, flip, gain, bias=None, act=False):
    """ldetr_upfirdn2d_f32 as torch_utils/ops/upfirdn2d.py:_kernel_call calls it, into a NaN-filled buffer -> (y, the guard band behind it)."""
    from layoutdetr_amd.hip import core
    N, C, H, W = xv.shape
    fh, fw = f2d.shape
    oW, oH = R.out_size(W, up[0], pad[0], pad[1], fw, down[0]), R.out_size(H, up[1], pad[2], pad[3], fh, down[1])
    n = N * C * oH * oW
    buf = torch.full((n + GUARD,), NAN, device=xv.device)
    cl = xv.stride(1) == 1 and C > 1
    y = buf[:n].view(N, oH, oW, C).permute(0, 3, 1, 2) if cl else buf[:n].view(N, C, oH, oW)
    xs, ys = (ctypes.c_int64 * 4)(*xv.stride()), (ctypes.c_int64 * 4)(*y.stride())
    core.check(core.lib().ldetr_upfirdn2d_f32(
        core.ptr(xv), core.ptr(f2d), core.ptr(y), N, C, H, W, xs, fh, fw, f2d.stride(0), f2d.stride(1), up[0], up[1], down[0], down[1],
        pad[0], pad[1], pad[2], pad[3], 1 if flip else 0, float(gain), oH, oW, ys, core.ptr(bias), 1 if act else 0, R.ACT_ALPHA, R.ACT_GAIN,
        core.stream()), 'upfirdn2d')
    return y, buf[n:]


def run_upfirdn(dev, c, exact, fig):
    """-> (y, dx) of the kernels for a table case, dense on the CPU."""
    from layoutdetr_amd.torch_utils.ops import upfirdn2d
    x, bias = R.uf_inputs(c, exact)
    f = R.make_filter(c['filt'], exact)
    fd = f.to(dev) if f is not None else None
    xv = R.build_input(x.to(dev), c['layout']).requires_grad_(True)
    _, _, offset, strides = R.layout_geometry(c['shape'], c['layout'])
    assert tuple(xv.stride()) == tuple(strides) and xv.data_ptr() % 16 == 4 * (offset % 4)          # what the path predicate assumes
    kw = dict(up=list(c['up']), down=list(c['down']), padding=list(c['pad']), flip_filter=c['flip'], gain=c['gain'])
    yw = upfirdn2d.upfirdn2d(xv, fd, **kw)
    _, _, g = R.uf_reference_cached(c['name'], exact)
    (dx,) = torch.autograd.grad(yw, xv, torch.empty_like(yw).copy_(g.to(dev)))
    y = yw.detach()
    if c['via'] == 'abi':
        assert f is not None and f.ndim == 2
        y, band = abi_upfirdn(xv.detach(), fd, c['up'], c['down'], c['pad'], c['flip'], c['gain'], bias.to(dev) if bias is not None else None, bool(c['act']))
        fig.exact(c['name'], 'guard band behind y untouched', band.isnan().all())
        if not c['act']:
            fig.exact(c['name'], 'wrapper and C entry agree bit for bit', torch.equal(y, yw.detach()))
    return y.cpu(), dx.cpu()


@pytest.mark.parametrize('group', R.UPFIRDN_GROUPS)
def test_upfirdn_exact_inputs_equal_float64(dev, group):
    fig = Figures()
    for c in (c for c in R.UPFIRDN_CASES if c['group'] == group):
        y64, dx64, _ = R.uf_reference_cached(c['name'], True)
        y, dx = run_upfirdn(dev, c, True, fig)
        fig.exact(c['name'], f'y equals float64 (paths {sorted(R.upfirdn_paths(c))})', y.shape == y64.shape and torch.equal(y.double(), y64))
        fig.exact(c['name'], 'dx equals float64', dx.shape == dx64.shape and torch.equal(dx.double(), dx64))
    fig.check()


@pytest.mark.parametrize('group', R.UPFIRDN_GROUPS)
def test_upfirdn_rounding_within_the_float32_yardstick(dev, group):
    fig = Figures()
    for c in (c for c in R.UPFIRDN_CASES if c['group'] == group):
        y64, dx64, _ = R.uf_reference_cached(c['name'], False)
        y, dx = run_upfirdn(dev, c, False, fig)
        if c['act']:
            fig.both(c['name'], 'upfirdn_act', y, y64, elem=False)
        else:
            fig.both(c['name'], 'upfirdn_y', y, y64)
        fig.both(c['name'], 'upfirdn_dx', dx, dx64)
    fig.check()


def test_upfirdn_second_order(dev):
    """The backward of the backward (torch_utils/ops/upfirdn2d.py:116-127 re-entered): d<dx, v>/dg is the forward operator applied to v."""
    from layoutdetr_amd.torch_utils.ops import upfirdn2d
    c = R.SECOND_ORDER_CASE
    y64, dx64, ddy64, g, v = R.second_order_ref(c)
    x, _ = R.uf_inputs(c, False)
    xv = R.build_input(x.to(dev), c['layout']).requires_grad_(True)
    y = upfirdn2d.upfirdn2d(xv, R.make_filter(c['filt'], False).to(dev), up=list(c['up']), down=list(c['down']), padding=list(c['pad']), flip_filter=c['flip'], gain=c['gain'])
    gd = torch.empty_like(y).copy_(g.to(dev)).requires_grad_(True)
    (dx,) = torch.autograd.grad(y, xv, gd, create_graph=True)
    (ddy,) = torch.autograd.grad(dx, gd, torch.empty_like(dx).copy_(v.to(dev)))
    fig = Figures()
    fig.both(c['name'], 'upfirdn_y', y, y64)
    fig.both(c['name'], 'upfirdn_dx', dx, dx64)
    fig.both(c['name'], 'upfirdn_ddy', ddy, ddy64, elem=False)
    fig.check()


@pytest.mark.parametrize('helper,filt,factor,padding,flip,gain', R.HELPER_CASES)
def test_upfirdn_helpers(dev, helper, filt, factor, padding, flip, gain):
    """filter2d / upsample2d / downsample2d derive their pads as the reference does."""
    from layoutdetr_amd.torch_utils.ops import upfirdn2d
    x = torch.randn(2, 3, 14, 15, generator=torch.Generator().manual_seed(620)).abs() + 0.1
    f = R.make_filter(filt, False)
    ref = R.helper_ref(helper, x, f, factor, padding, flip, gain)
    kw = dict(padding=padding, flip_filter=flip, gain=gain)
    if helper == 'upsample2d':
        kw['up'] = factor
    elif helper == 'downsample2d':
        kw['down'] = factor
    y = getattr(upfirdn2d, helper)(x.to(dev), f.to(dev) if f is not None else None, **kw)
    fig = Figures()
    assert y.shape == ref.shape
    fig.both(f'{helper}-{filt}', 'upfirdn_y', y, ref)
    if helper == 'filter2d' and filt == '4x4':       # a 1-D filter with one tap is squared into a 1 x 1 (torch_utils/ops/upfirdn2d.py:104-105)
        one = torch.tensor([0.5])
        fig.both('one-tap-1d', 'upfirdn_y', upfirdn2d.upfirdn2d(x.to(dev), one.to(dev), gain=1.5), R.upfirdn_ref(x, one, (1, 1), (1, 1), (0, 0, 0, 0), False, 1.5))
    fig.check()


def is_power_of_two(v):
    return np.frexp(v)[0] == 0.5


@pytest.mark.parametrize('c', R.BIT_IDENTITY_CASES, ids=[c['name'] for c in R.BIT_IDENTITY_CASES])
def test_fir4x4_is_bit_identical_to_the_planar_kernel(dev, c):
    """csrc/upfirdn2d.hip:148-149: the same (jy, jx)-ordered fma chain, so with a power-of-two gain (fir4x4 multiplies the taps by it, the planar
    kernel the sum) the same bits.  The channels_last view one float into its buffer is what forces the planar kernel."""
    assert is_power_of_two(c['gain'])
    other = dict(c, layout='cl_offset1')
    assert any(p.startswith('fir4x4/') for p in R.upfirdn_paths(c)) and 'planar/cl_misaligned' in R.upfirdn_paths(other)
    x = torch.randn(c['shape'], generator=torch.Generator().manual_seed(630 + c['seed']))
    f = R.make_filter('4x4', False).to(dev)
    fig = Figures()
    for act, bias in ((False, None), (True, torch.randn(c['shape'][1], generator=torch.Generator().manual_seed(631)).to(dev))):
        ys = []
        for layout in (c['layout'], 'cl_offset1'):
            y, band = abi_upfirdn(R.build_input(x.to(dev), layout), f, c['up'], c['down'], c['pad'], c['flip'], c['gain'], bias, act)
            fig.exact(c['name'], f'guard band ({layout})', band.isnan().all())
            ys.append(y.cpu())
        fig.exact(c['name'], f'fir4x4 == planar, act {act}', torch.equal(ys[0], ys[1]) and not bool(ys[0].isnan().any()))
        fig.value(c['name'], f'largest difference, act {act}', (ys[0].double() - ys[1].double()).abs().max().item(), 0.0)
    fig.check()


# ------------------------------------------------------------------------------------------------------------------------ demod
def demod_fwd(dev, wv, sd):
    from layoutdetr_amd.hip import core
    (O, I, K, _), B = wv.shape, sd.shape[0]
    d = torch.full((B, O), NAN, device=dev)
    w2 = torch.full((O, I), NAN, device=dev)
    st = wv.stride()
    rc = core.lib().ldetr_demod_fwd_f32(core.ptr(wv), st[0], st[1], st[2], st[3], core.ptr(sd), core.ptr(d), core.ptr(w2), B, O, I, K, K, R.DEMOD_EPS, core.stream())
    return rc, d, w2


def demod_bwd(dev, wv, sd, d, w2, gd, dw, accumulate, ds):
    from layoutdetr_amd.hip import core
    (O, I, K, _), B = wv.shape, sd.shape[0]
    st = wv.stride()
    assert dw is None or dw.stride() == st
    core.check(core.lib().ldetr_demod_bwd_f32(core.ptr(wv), st[0], st[1], st[2], st[3], core.ptr(sd), core.ptr(d), core.ptr(w2), core.ptr(gd), core.ptr(dw),
                                              1 if accumulate else 0, core.ptr(ds), B, O, I, K, K, core.stream()), 'demod_bwd')


def like_weight(dev, c, w, fill):
    """A gradient buffer with the strides of the case's weight, holding `fill` (a tensor or a value); -> (view, whole buffer)."""
    v, buf = R.demod_weight_layout(torch.full_like(w, NAN).to(dev), c['layout'])
    if isinstance(fill, torch.Tensor):
        v.copy_(fill.to(dev))
    else:
        v.fill_(fill)
    return v, buf


DEMOD_ABI = [c['name'] for c in R.DEMOD_CASES if c['B'] <= R.DEMOD_MAXB]
DEMOD_GEMM = [c['name'] for c in R.DEMOD_CASES if c['B'] > R.DEMOD_MAXB]


@pytest.mark.parametrize('name', DEMOD_ABI)
def test_demod_kernels(dev, name):
    from layoutdetr_amd.hip import core
    c = R.DEMOD_BY_NAME[name]
    w, s, g, dw0 = R.demod_inputs(c)
    d64, dw64, ds64 = R.demod_reference_cached(name)
    wv, _ = R.demod_weight_layout(w.to(dev), c['layout'])
    sd, gd = s.to(dev), g.to(dev)
    fig = Figures()
    rc, d, w2 = demod_fwd(dev, wv, sd)
    core.check(rc, 'demod_fwd')
    fig.both(name, 'demod_d', d, d64)
    # W2 is a sum of at most 9 squares, all positive: (taps + 1) roundings of 2^-24 each at the most
    fig.value(name, 'W2 elem', R.elem_rel_err(w2, w.double().square().sum([2, 3])), (c['K'] ** 2 + 1) * 2.0 ** -24)
    # stored: both gradients, into NaN
    dw, dwbuf = like_weight(dev, c, w, NAN)
    ds = torch.full_like(sd, NAN)
    demod_bwd(dev, wv, sd, d, w2, gd, dw, False, ds)
    fig.both(name, 'demod_dw', dw, dw64)
    fig.both(name, 'demod_ds', ds, ds64)
    fig.exact(name, 'nothing written outside the weight gradient', int(dwbuf.isnan().sum()) == dwbuf.numel() - w.numel())
    if c['zero_row'] is not None:
        fig.exact(name, 'zero style row: d = rsqrt(eps), ds = 0', bool((d[c['zero_row']].cpu().double() - d64[c['zero_row']]).abs().max() <= 1e4 * R.fp32_bound('demod_d_elem'))
                  and not bool(ds[c['zero_row']].any()))
    # summed into a buffer that starts non-zero, scaled to the size of the gradient: the buffer plus the gradient, one more rounding
    start = dw0 * dw64.abs().max().float()
    acc, accbuf = like_weight(dev, c, w, start)
    demod_bwd(dev, wv, sd, d, w2, gd, acc, True, None)
    want = start.double() + dw64
    fig.value(name, 'dw accumulated', (acc.cpu().double() - want).abs().max().item(), R.fp32_bound('demod_dw') * dw64.abs().max().item() + 2.0 ** -24 * want.abs().max().item())
    fig.exact(name, 'nothing written outside the accumulated gradient', int(accbuf.isnan().sum()) == accbuf.numel() - w.numel())
    # each gradient alone: the same kernels on the same inputs, so the same bits
    dw1, _ = like_weight(dev, c, w, NAN)
    demod_bwd(dev, wv, sd, d, w2, gd, dw1, False, None)
    ds1 = torch.full_like(sd, NAN)
    demod_bwd(dev, wv, sd, d, w2, gd, None, False, ds1)
    fig.exact(name, 'dw alone equals dw of the joint call', torch.equal(dw1, dw))
    fig.exact(name, 'ds alone equals ds of the joint call', torch.equal(ds1, ds))
    fig.check()


@pytest.mark.parametrize('name', DEMOD_GEMM)
def test_demod_gemm_form_past_64_samples(dev, name):
    """hip/modconv.py:310-312: the C entry refuses B > 64 (before it launches anything), demod_coefs takes the GEMM form."""
    from layoutdetr_amd.hip.modconv import demod_coefs
    c = R.DEMOD_BY_NAME[name]
    w, s, g, _ = R.demod_inputs(c)
    d64, dw64, ds64 = R.demod_reference_cached(name)
    wv, _ = R.demod_weight_layout(w.to(dev), c['layout'])
    rc, d, _ = demod_fwd(dev, wv, s.to(dev))
    assert rc != 0 and bool(d.isnan().all())
    wv.requires_grad_(True)
    sd = s.to(dev).requires_grad_(True)
    d = demod_coefs(wv, sd)
    dw, ds = torch.autograd.grad(d, (wv, sd), g.to(dev))
    fig = Figures()
    fig.both(name, 'demod_d', d, d64)
    fig.both(name, 'demod_dw', dw, dw64)
    fig.both(name, 'demod_ds', ds, ds64)
    fig.check()


@pytest.mark.parametrize('name', [n for n in DEMOD_ABI if R.DEMOD_BY_NAME[n]['layout'] != 'slice'][::5])
def test_demod_autograd_route(dev, name):
    """The same through demod_coefs (_DemodFn): gradients to the weight in its own memory layout and to the styles."""
    from layoutdetr_amd.hip.modconv import demod_coefs
    c = R.DEMOD_BY_NAME[name]
    w, s, g, _ = R.demod_inputs(c)
    d64, dw64, ds64 = R.demod_reference_cached(name)
    wv, _ = R.demod_weight_layout(w.to(dev), c['layout'])
    wv.requires_grad_(True)
    sd = s.to(dev).requires_grad_(True)
    d = demod_coefs(wv, sd)
    dw, ds = torch.autograd.grad(d, (wv, sd), g.to(dev))
    fig = Figures()
    fig.both(name, 'demod_d', d, d64)
    fig.both(name, 'demod_dw', dw, dw64)
    fig.both(name, 'demod_ds', ds, ds64)
    fig.check()


# ------------------------------------------------------------------------------------------------------------------------ page resize
def resize_run(dev, imgs, out_h, out_w, outputs, images=None):
    """ldetr_resize_normalize_u8 on uint8 [n, H, W, 3] with every buffer it may write prefilled (0xFF, NaN) -> (rc, u8, chw, tmp)."""
    from layoutdetr_amd.hip import core
    from layoutdetr_amd.training.dataset_layoutganpp import RGB_MEAN, RGB_STD, resample_coeffs
    n, H, W, _ = imgs.shape
    src = torch.from_numpy(imgs).to(dev)
    hb, hk, hks = resample_coeffs(W, out_w, dev)
    vb, vk, vks = resample_coeffs(H, out_h, dev)
    tmp = torch.full((n, H, out_w, 3), 255, dtype=torch.uint8, device=dev)
    u8 = torch.full((n, out_h, out_w, 3), 255, dtype=torch.uint8, device=dev)
    chw = torch.full((n, 3, out_h, out_w), NAN, device=dev)
    m = [float(np.float32(v)) for v in RGB_MEAN]
    s = [float(np.float32(v)) for v in RGB_STD]
    rc = core.lib().ldetr_resize_normalize_u8(core.ptr(src), n if images is None else images, H, W, out_h, out_w, core.ptr(hb), core.ptr(hk), hks, core.ptr(vb),
                                              core.ptr(vk), vks, core.ptr(tmp), core.ptr(u8) if outputs != 'chw_only' else None,
                                              core.ptr(chw) if outputs != 'u8_only' else None, m[0], m[1], m[2], s[0], s[1], s[2], core.stream())
    return rc, u8.cpu().numpy(), chw.cpu().numpy(), tmp.cpu().numpy()


@pytest.mark.parametrize('name', [c['name'] for c in R.RESIZE_CASES])
def test_resize_is_bit_equal_to_the_reference(dev, name):
    from layoutdetr_amd.hip import core
    c = R.RESIZE_BY_NAME[name]
    imgs = R.resize_inputs(c)
    ref_u8, ref_chw = R.resize_reference_cached(name)
    rc, u8, chw, _ = resize_run(dev, imgs, c['out_h'], c['out_w'], c['outputs'])
    core.check(rc, 'resize_normalize_u8')
    print(f'[resampling] {name}: paths {sorted(R.resize_paths(c))}')
    if c['outputs'] != 'chw_only':
        assert np.array_equal(u8, ref_u8), f'{name}: uint8, {int((u8 != ref_u8).sum())} bytes differ'
    else:
        assert bool((u8 == 255).all()), f'{name}: the uint8 output was not asked for'
    if c['outputs'] != 'u8_only':
        assert np.array_equal(chw, ref_chw), f'{name}: float, {int((chw != ref_chw).sum())} values differ'
    else:
        assert bool(np.isnan(chw).all()), f'{name}: the float output was not asked for'
    # batch independence: the last image alone
    _, u8_1, chw_1, _ = resize_run(dev, imgs[-1:], c['out_h'], c['out_w'], 'both')
    assert np.array_equal(u8_1[0], ref_u8[-1]) and np.array_equal(chw_1[0], ref_chw[-1]), f'{name}: the last image alone'


def test_resize_coefficient_tables_equal_the_reference(dev):
    """ldetr_resample_coeffs (csrc/resample.hip:102-113 around the host builder, csrc/pil_resample.hpp:59-90): bounds and 22-bit weights, tap-major."""
    from layoutdetr_amd.training.dataset_layoutganpp import resample_coeffs
    from oracle import resample_ref
    for n_in, n_out in sorted({(c['W'], c['out_w']) for c in R.RESIZE_CASES} | {(c['H'], c['out_h']) for c in R.RESIZE_CASES}):
        bounds, kk, ks = resample_ref.precompute_coeffs(n_in, n_out)
        b, k, ksize = resample_coeffs(n_in, n_out, dev)
        assert ksize == ks and np.array_equal(b.cpu().numpy(), bounds) and np.array_equal(k.cpu().numpy(), kk.T), (n_in, n_out)
        assert bool((kk < 0).any()) or n_in == n_out


def test_resize_of_zero_images_touches_nothing(dev):
    c = R.RESIZE_BY_NAME['base-odd']
    rc, u8, chw, tmp = resize_run(dev, R.resize_inputs(c), c['out_h'], c['out_w'], 'both', images=0)
    assert rc == 0 and bool((u8 == 255).all()) and bool(np.isnan(chw).all()) and bool((tmp == 255).all())
