"""Every host-side path of the element-wise and row-streaming kernels against float64: the optimiser pass (csrc/optim.hip), bias_act
(csrc/bias_act.hip), the toRGB forward / backward / finish kernels and the 3x3 stride-2 max-pool (csrc/misc_ops.hip).  References, case tables
and the path predicates whose names appear in the test ids are in tests/streaming_common.py; tests/test_streaming_ref_cpu.py proves that the
tables reach every path.  Bounds: selections and copies are exact; families with a project bound keep it (bias_act 2e-6 / 5e-6, optimiser 1e-6,
toRGB gradients 5e-5 / 1e-4 as in test_sg2_handoff_gpu.py, the contraction engine's forward 3e-6 as in test_conv2d_fwd_bwd); the rest is held to
4 x the error of the same formula evaluated in float32 by torch on the CPU (streaming_common.FP32_BASELINE).  Every element of every output is
compared."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import streaming_common as S

pytestmark = pytest.mark.gpu

S.limit_threads()
TOL_ENGINE_Y = 3e-6       # test_conv2d_fwd_bwd: the contraction engine's forward, which hip.modconv.torgb_fwd falls back to


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def pid(path):
    return path.replace('/', '.')


def _core():
    from layoutdetr_amd.hip import core
    return core


# ------------------------------------------------------------------------------------------------------------------------ optimiser
@functools.lru_cache(maxsize=None)
def _big():
    """Inputs of the one past-the-cap case, shared (read-only) by the four entry points."""
    return S.optim_inputs(S.OPT_BIG, seed=1)


def _adam_gpu(dev, t, steps, betas, fuse, first_step=1, ema_beta=None):
    core = _core()
    p, m, v = t['p'].to(dev), t['m'].to(dev), t['v'].to(dev)
    pe = t['pe'].to(dev) if ema_beta is not None else None
    s, n = S.SANITIZE, t['p'].numel()
    for k in range(steps):
        g = S.step_gradient(t['g'], k + 1)
        gd = (S.poison(g) if fuse else g).to(dev)
        # fuse 0: gscale and the replacement values are ignored
        args = (core.ptr(p), core.ptr(gd), core.ptr(m), core.ptr(v), n, first_step + k, S.OPT_LR, betas[0], betas[1], S.OPT_EPS,
                fuse, s['gscale'], s['nan'], s['posinf'], s['neginf'])
        if pe is None:
            core.check(core.lib().ldetr_adam_step_f32(*args, core.stream()), 'adam_step')
        else:
            core.check(core.lib().ldetr_adam_ema_step_f32(*args, core.ptr(pe), ema_beta, core.stream()), 'adam_ema_step')
    torch.cuda.synchronize()
    return p, m, v, pe


def _check_adam(got, ref, p0):
    p, m, v = got
    p64, m64, v64 = ref
    e_p, e_u, e_m, e_v = S.rel_err(p, p64), S.update_rel_err(p, p64, p0), S.elem_rel_err(m, m64), S.elem_rel_err(v, v64)
    print(f'adam: p {e_p:.3e} (max-normalised), {e_u:.3e} of the update; m {e_m:.3e}, v {e_v:.3e} (per element)')
    assert bool(torch.isfinite(p).all())
    assert e_p <= S.TOL_OPT_P                             # project bound (test_adam_sanitize_ema)
    assert e_u <= S.fp32_bound('adam_p_update')           # float32 torch on the CPU: 4.86e-6 -> 1.9e-5
    assert e_m <= S.fp32_bound('adam_m')                  # 1.39e-7 -> 5.6e-7
    assert e_v <= S.fp32_bound('adam_v')                  # 1.48e-7 -> 5.9e-7


def _opt_id(n):
    return f'n{n}-{S.optim_path(n)}'


@pytest.mark.parametrize('fuse', [0, 1], ids=['fuse0', 'fuse1'])
@pytest.mark.parametrize('betas', S.OPT_BETAS, ids=[f'beta1_{b[0]}' for b in S.OPT_BETAS])
@pytest.mark.parametrize('n', S.OPT_SIZES, ids=_opt_id)
def test_adam_three_steps(dev, n, betas, fuse):
    t = S.optim_inputs(n, seed=n)
    got = _adam_gpu(dev, t, 3, betas, fuse)
    _check_adam(got[:3], S.adam_run(t, 3, betas, fuse), t['p'])


def test_adam_step_1000_from_a_running_state_beta1_0_9(dev):
    t = S.optim_step1000_inputs()
    got = _adam_gpu(dev, t, 1, S.OPT_BETAS[0], 0, first_step=1000)
    _check_adam(got[:3], S.adam_run(t, 1, S.OPT_BETAS[0], 0, first_step=1000), t['p'])


def test_adam_many_rounds_past_the_cap_beta1_0_9(dev):
    """16.8 M elements: blocks 0 .. 3 make a second round of the chunk loop, the last chunk is ragged, three elements go through the scalar tail;
    NaN / Inf sit in the first quad, a second-round chunk, the last chunk and the tail."""
    assert S.optim_path(S.OPT_BIG) == 'many_rounds'
    t = _big()
    got = _adam_gpu(dev, t, 1, S.OPT_BETAS[0], 1)
    _check_adam(got[:3], S.adam_run(t, 1, S.OPT_BETAS[0], 1), t['p'])


@pytest.mark.parametrize('n', S.OPT_SIZES + [S.OPT_BIG], ids=_opt_id)
def test_adam_ema_is_adam_then_lerp(dev, n):
    """The first step from zero moments: ldetr_adam_ema_step_f32 == ldetr_adam_step_f32 followed by ldetr_ema_lerp_f32, bit for bit (the identity
    of test_adam_sanitize_ema, at every size).  It is a property of zero moments only: the two instantiations of adam_kernel contract
    b1 m + (1 - b1) g differently (the EMA one rounds both products in one lane of the quad, the plain one fuses), which is invisible while
    b1 m == 0.  So the second step, from running moments, holds the fused pass to float64 like any other Adam step, and its EMA to the EMA's bound."""
    core = _core()
    big = n == S.OPT_BIG
    t = _big() if big else S.optim_inputs(n, seed=n)
    steps, beta = (1 if big else 2), 0.999
    b1, b2 = S.OPT_BETAS[0]
    s = S.SANITIZE
    pa, ma, va, ea = _adam_gpu(dev, t, 1, S.OPT_BETAS[0], 1, ema_beta=beta)
    pb, mb, vb, eb = t['p'].to(dev), t['m'].to(dev), t['v'].to(dev), t['pe'].to(dev)
    gd = S.poison(S.step_gradient(t['g'], 1)).to(dev)
    core.check(core.lib().ldetr_adam_step_f32(core.ptr(pb), core.ptr(gd), core.ptr(mb), core.ptr(vb), n, 1, S.OPT_LR, b1, b2, S.OPT_EPS,
                                              1, s['gscale'], s['nan'], s['posinf'], s['neginf'], core.stream()), 'adam_step')
    core.check(core.lib().ldetr_ema_lerp_f32(core.ptr(eb), core.ptr(pb), n, beta, core.stream()), 'ema_lerp')
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb)
    if steps > 1:
        pa, ma, va, ea = _adam_gpu(dev, t, steps, S.OPT_BETAS[0], 1, ema_beta=beta)
    p64, m64, v64, e64 = t['p'], t['m'], t['v'], t['pe']
    for k in range(steps):
        g = S.poison(S.step_gradient(t['g'], k + 1))
        p64, m64, v64, e64 = S.adam_ref(p64, g, m64, v64, k + 1, S.OPT_LR, b1, b2, S.OPT_EPS, s, pe=e64, ema_beta=beta)
    e = S.rel_err(ea, e64)
    print(f'adam_ema: p_ema {e:.3e}')
    assert e <= S.TOL_OPT_P
    _check_adam((pa, ma, va), (p64, m64, v64), t['p'])


@pytest.mark.parametrize('n', S.OPT_SIZES + [S.OPT_BIG], ids=_opt_id)
def test_ema_lerp(dev, n):
    core = _core()
    t = _big() if n == S.OPT_BIG else S.optim_inputs(n, seed=n)
    pe, p = t['pe'].to(dev), t['p'].to(dev)
    core.check(core.lib().ldetr_ema_lerp_f32(core.ptr(pe), core.ptr(p), n, 0.999, core.stream()), 'ema_lerp')
    assert torch.equal(p.cpu(), t['p']), 'p is read only'
    e = S.rel_err(pe, S.ema_ref(t['pe'], t['p'], 0.999))
    print(f'ema_lerp: {e:.3e}')
    assert e <= S.TOL_OPT_P


@pytest.mark.parametrize('n', S.OPT_SIZES + [S.OPT_BIG], ids=_opt_id)
def test_grad_sanitize_is_exact(dev, n):
    core = _core()
    t = _big() if n == S.OPT_BIG else S.optim_inputs(n, seed=n)
    g = S.poison(t['g'])
    s = S.SANITIZE
    gd = g.to(dev)
    core.check(core.lib().ldetr_grad_sanitize_f32(core.ptr(gd), n, s['gscale'], s['nan'], s['posinf'], s['neginf'], core.stream()), 'grad_sanitize')
    want = S.sanitize_ref(g, s['gscale'], s['nan'], s['posinf'], s['neginf'])        # float32: scaling by 0.5 is exact
    assert bool(torch.isfinite(want).all()) and torch.equal(gd.cpu(), want)


# ------------------------------------------------------------------------------------------------------------------------ bias_act
def _ba_id(c):
    return f"{c['name']}-{pid(S.bias_act_path(c))}"


def _ba_abi(dev, c, x, b, dy, ddx, y64):
    """One ldetr_bias_act_f32 call with the operands the autograd wrapper would hand over for this gradient order
    (torch_utils/ops/bias_act.py:69, :91, :103): -> the output as a flat CPU tensor."""
    core = _core()
    n, size_b, step_b = S.bias_act_geometry(c)
    off = c['offset']

    def buf(t):
        if t is None:
            return None
        d = torch.empty(n + 4, device=dev)[off:off + n]
        d.copy_(t.reshape(-1).to(dev))
        return d
    act, grad = c['act'], c['grad']
    need_x = act in ('swish', 'gelu') or act in S.HAS_2ND
    need_y = act not in ('linear', 'swish', 'gelu')
    xd = buf(x)
    if grad == 0:
        args = (xd, None, None, None)
    else:
        xref = xd if need_x else None
        yref = buf(y64.float()) if need_y else None
        args = (buf(dy), xref, yref, None) if grad == 1 else (buf(ddx), xref, yref, buf(dy))
    out = args[0] if c['inplace'] else buf(torch.full((n,), math.nan))
    bd = b.to(dev) if b is not None else None
    keep = [a.clone() if a is not None and a is not out else None for a in args]
    core.check(core.lib().ldetr_bias_act_f32(core.ptr(args[0]), core.ptr(bd), core.ptr(args[1]), core.ptr(args[2]), core.ptr(args[3]), core.ptr(out), n,
                                             size_b, step_b, grad, S.ACT_INDEX[act], c['alpha'], c['gain'], -1.0 if c['clamp'] is None else c['clamp'],
                                             core.stream()), 'bias_act')
    torch.cuda.synchronize()
    for a, k in zip(args, keep):
        assert k is None or torch.equal(a, k), 'an input was written'
    return out.cpu()


@pytest.mark.parametrize('c', S.BIAS_ACT_CASES, ids=_ba_id)
def test_bias_act_paths(dev, c):
    x, b, dy, ddx = S.bias_act_inputs(c)
    grad = c['grad']
    y64, dx64, d_x64 = S.bias_act_ref(x, b, c['axis'], c['act'], c['alpha'], c['gain'], c['clamp'], dy=dy if grad >= 1 else None, ddx=ddx if grad == 2 else None)
    if c['via'] == 'wrapper':
        from layoutdetr_amd.torch_utils.ops import bias_act
        xg, bg = x.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        y = bias_act.bias_act(xg, bg, dim=c['axis'], act=c['act'], alpha=c['alpha'], gain=c['gain'], clamp=c['clamp'])
        y.backward(dy.to(dev))
        e_y, e_dx = S.rel_err(y, y64), S.rel_err(xg.grad, dx64)
        e_db = S.rel_err(bg.grad, dx64.sum([i for i in range(x.ndim) if i != c['axis']]))
        print(f'bias_act wrapper: y {e_y:.3e}, dx {e_dx:.3e}, db {e_db:.3e}')
        assert e_y <= S.TOL_BIAS_ACT['y'] and e_dx <= S.TOL_BIAS_ACT['dx'] and e_db <= 2e-5       # db: test_bias_act's bound
        return
    got = _ba_abi(dev, c, x, b, dy, ddx, y64)
    ref = (y64, dx64, d_x64)[grad].reshape(-1)
    e = S.rel_err(got, ref)
    print(f'bias_act grad {grad}: {e:.3e}')
    assert float(ref.abs().max()) > 0.1
    assert e <= (S.TOL_BIAS_ACT['y'] if grad == 0 else S.TOL_BIAS_ACT['dx'])


# ------------------------------------------------------------------------------------------------------------------------ toRGB
def _fwd_id(case):
    B, P, C, how = case
    return f'B{B}-P{P}-C{C}-{how}-{pid(S.torgb_fwd_case_path(case))}'


@pytest.mark.parametrize('case', S.TORGB_FWD_CASES, ids=_fwd_id)
def test_torgb_forward(dev, case):
    core = _core()
    B, P, C, how = case
    t = S.torgb_inputs(B, P, C)
    bias = None if how == 'abi_nobias' else t['bias']
    ref = S.torgb_fwd_ref(t['x'], t['w'], t['s'], bias)
    x, w, bd = t['x'].to(dev), t['w'].to(dev), (bias.to(dev) if bias is not None else None)
    s = t['s'].to(dev)
    path = S.torgb_fwd_case_path(case)
    if how.startswith('abi'):
        y = torch.full((B, P, 3), math.nan, device=dev)
        core.check(core.lib().ldetr_torgb_fwd_f32(core.ptr(x), core.ptr(w), core.ptr(s), core.ptr(bd), core.ptr(y), B, P, C, core.stream()), 'torgb_fwd')
    else:
        from layoutdetr_amd.hip import modconv
        if how == 'wrapper_strided':
            wide = torch.zeros(B, C + 4, device=dev)
            wide[:, :C] = s
            s = wide[:, :C]
            assert s.stride(0) != C
        from engine_launches import Launches
        with Launches() as L:
            y = modconv.torgb_fwd(x.reshape(B, 1, P, C), w, s, bd).reshape(B, P, 3)
        assert (len(L.seen) > 0) == (path == 'engine_fallback'), 'the wrapper took another path than the predicate says'
    e = S.rel_err(y, ref)
    print(f'torgb_fwd {path}: {e:.3e}')
    # streaming kernel: float32 torch on the CPU is 6.84e-7 from float64 -> 2.7e-6; engine fallback: the engine's own forward bound
    assert e <= (TOL_ENGINE_Y if path == 'engine_fallback' else S.fp32_bound('torgb_fwd'))


def _bwd_id(case):
    return 'B%d-P%d-C%d-' % case + pid(S.torgb_bwd_path(*case))


def _torgb_bwd_abi(dev, t, B, P, C, with_dbias=True):
    core = _core()
    c = {k: v.to(dev) for k, v in t.items()}
    dx = torch.full((B, P, C), math.nan, device=dev)
    dws = torch.zeros(B, 3, C, device=dev)
    dbias = torch.zeros(3, device=dev) if with_dbias else None
    core.check(core.lib().ldetr_torgb_bwd_f32(core.ptr(c['x']), core.ptr(c['dy']), core.ptr(c['w']), core.ptr(c['s']), core.ptr(dx), core.ptr(dws),
                                              core.ptr(dbias), B, P, C, core.stream()), 'torgb_bwd')
    torch.cuda.synchronize()
    return dx, dws, dbias


def _check_torgb_bwd(got, ref, what):
    (dx, dws, dbias), (dx64, dws64, db64) = got, ref
    e = [S.rel_err(dx, dx64), S.rel_err(dws, dws64), S.rel_err(dbias, db64) if dbias is not None else 0.0]
    print(f'torgb_bwd {what}: dx {e[0]:.3e}, dws {e[1]:.3e}, dbias {e[2]:.3e}')
    assert e[0] <= S.TOL_TORGB['dx'] and e[1] <= S.TOL_TORGB['dws'] and e[2] <= S.TOL_TORGB['dbias']


@pytest.mark.parametrize('case', S.TORGB_BWD_CASES, ids=_bwd_id)
def test_torgb_backward(dev, case):
    B, P, C = case
    t = S.torgb_inputs(B, P, C)
    _check_torgb_bwd(_torgb_bwd_abi(dev, t, B, P, C), S.torgb_bwd_ref(t['x'], t['dy'], t['w'], t['s']), S.torgb_bwd_path(*case))


def test_torgb_backward_without_bias_gradient(dev):
    B, P, C = 3, 37, 32
    t = S.torgb_inputs(B, P, C)
    _check_torgb_bwd(_torgb_bwd_abi(dev, t, B, P, C, with_dbias=False), S.torgb_bwd_ref(t['x'], t['dy'], t['w'], t['s']), 'dbias NULL')


@pytest.mark.parametrize('B,C', S.TORGB_FINISH_CASES, ids=lambda v: str(v))
def test_torgb_finish(dev, B, C):
    """dw accumulates onto a non-zero start; the 3C items of dw and the B C items of ds end in different blocks of one grid."""
    core = _core()
    t = S.finish_inputs(B, C)
    dw64, ds64 = S.torgb_finish_ref(t['dws'], t['s'], t['w'], t['dw0'])
    c = {k: v.to(dev) for k, v in t.items()}
    dw, ds = c['dw0'].clone(), torch.full((B, C), math.nan, device=dev)
    core.check(core.lib().ldetr_torgb_bwd_finish_f32(core.ptr(c['dws']), core.ptr(c['s']), core.ptr(c['w']), B, C, core.ptr(dw), core.ptr(ds), core.stream()),
               'torgb_bwd_finish')
    e_dw, e_ds = S.rel_err(dw, dw64), S.rel_err(ds, ds64)
    print(f'torgb_finish: dw {e_dw:.3e}, ds {e_ds:.3e}')
    assert e_dw <= S.fp32_bound('finish_dw')       # float32 torch on the CPU: 8.87e-8 -> 3.5e-7
    assert e_ds <= S.fp32_bound('finish_ds')       # 8.38e-8 -> 3.4e-7


@pytest.mark.parametrize('flat', [False, True], ids=['autograd_grads', 'flat_grad_views'])
@pytest.mark.parametrize('C', [512, 32], ids=['C512', 'C32'])
def test_torgb_autograd_end_to_end(dev, C, flat):
    """hip.modconv.torgb forward + backward against float64; flat: weight and bias gradients accumulate into .grad views that already hold values
    (training_loop.FlatModule), the Function returns None for them."""
    from layoutdetr_amd.hip import modconv
    B, P = 3, 37
    t = S.torgb_inputs(B, P, C)
    y64 = S.torgb_fwd_ref(t['x'], t['w'], t['s'], t['bias'])
    dx64, dws64, db64 = S.torgb_bwd_ref(t['x'], t['dy'], t['w'], t['s'])
    w0 = t['dw0'] if flat else torch.zeros(3, C)
    b0 = torch.tensor([0.5, -1.0, 2.0]) if flat else torch.zeros(3)
    dw64, ds64 = S.torgb_finish_ref(dws64, t['s'], t['w'], w0)
    x = t['x'].reshape(B, 1, P, C).to(dev).requires_grad_(True)
    s = t['s'].to(dev).requires_grad_(True)
    w = torch.nn.Parameter(t['w'].reshape(3, C, 1, 1).to(dev))
    b = torch.nn.Parameter(t['bias'].to(dev))
    if flat:
        w.grad, b.grad = w0.reshape(3, C, 1, 1).to(dev), b0.to(dev)
        w._ldetr_flat = b._ldetr_flat = True
        views = (w.grad.data_ptr(), b.grad.data_ptr())
    y = modconv.torgb(x, w, s, b)
    y.backward(t['dy'].reshape(B, 1, P, 3).to(dev))
    if flat:
        assert (w.grad.data_ptr(), b.grad.data_ptr()) == views, 'the gradients were accumulated in place'
    e = dict(y=S.rel_err(y.reshape(B, P, 3), y64), dx=S.rel_err(x.grad.reshape(B, P, C), dx64), dw=S.rel_err(w.grad.reshape(3, C), dw64),
             ds=S.rel_err(s.grad, ds64), db=S.rel_err(b.grad, b0.double() + db64))
    print('torgb autograd: ' + ', '.join(f'{k} {v:.3e}' for k, v in e.items()))
    assert e['y'] <= S.fp32_bound('torgb_fwd') and e['dx'] <= S.TOL_TORGB['dx'] and e['db'] <= S.TOL_TORGB['dbias']
    assert e['dw'] <= S.TOL_TORGB['dws'] and e['ds'] <= S.TOL_TORGB['dws']       # sums of the fp32-atomic dws: its bound


# ------------------------------------------------------------------------------------------------------------------------ max-pool
def _pool_id(case):
    N, H, W, C, kind = case
    return f'{H}x{W}x{C}-{kind}'


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


@pytest.mark.parametrize('case', S.POOL_CASES, ids=_pool_id)
def test_maxpool_is_exactly_torch(dev, case):
    """Outputs and routed gradients bit for bit F.max_pool2d's (the gradients are multiples of 1/8: their sums are exact), on signed inputs,
    ties, NaN / +-Inf elements and windows that hold nothing but -inf."""
    from layoutdetr_amd.hip import conv
    N, H, W, C, kind = case
    x, dy = S.pool_inputs(N, H, W, C, kind)
    y64, dx64 = S.maxpool_ref(x, dy)
    xg = _nhwc(x, dev).requires_grad_(True)
    y = conv.maxpool3x3s2_nhwc(xg)
    y.backward(_nhwc(dy, dev))
    assert S.equal_with_nan(y.permute(0, 3, 1, 2), y64), 'y'
    assert torch.equal(xg.grad.permute(0, 3, 1, 2).double().cpu(), dx64), 'dx'
    if kind == 'all_neg_inf':
        assert float(dx64[0].abs().sum()) > 0, 'torch routes the gradient of an all -inf window to its first in-image element'


def test_maxpool_forward_without_index(dev):
    core = _core()
    N, H, W, C = 2, 13, 12, 8
    x, _ = S.pool_inputs(N, H, W, C, 'signed')
    y = torch.full((N, S.pool_out(H), S.pool_out(W), C), math.nan, device=dev)
    core.check(core.lib().ldetr_maxpool3x3s2_fwd_f32(core.ptr(_nhwc(x, dev)), core.ptr(y), None, N, H, W, C, core.stream()), 'maxpool_fwd')
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), F.max_pool2d(x, 3, 2, 1))


def test_maxpool_backward_stride_loop_past_the_grid_cap(dev):
    from layoutdetr_amd.hip import conv
    N, H, W, C, kind = S.POOL_BIG_BWD
    assert S.maxpool_path(N, H, W, C, 'bwd') == 'bwd/stride_loop'
    x, dy = S.pool_inputs(N, H, W, C, kind)
    y64, dx64 = S.maxpool_ref(x, dy)
    xg = _nhwc(x, dev).requires_grad_(True)
    y = conv.maxpool3x3s2_nhwc(xg)
    y.backward(_nhwc(dy, dev))
    assert torch.equal(y.permute(0, 3, 1, 2).double().cpu(), y64) and torch.equal(xg.grad.permute(0, 3, 1, 2).double().cpu(), dx64)


def test_maxpool_forward_stride_loop_past_the_grid_cap(dev):
    from layoutdetr_amd.hip import conv
    N, H, W, C, kind = S.POOL_BIG_FWD
    assert S.maxpool_path(N, H, W, C, 'fwd') == 'fwd/stride_loop'
    x, _ = S.pool_inputs(N, H, W, C, kind)
    with torch.no_grad():
        y = conv.maxpool3x3s2_nhwc(_nhwc(x, dev))
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), F.max_pool2d(x, 3, 2, 1))
