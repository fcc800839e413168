"""The beta1 == 0 specialisation of the flat-buffer Adam step (csrc/optim.hip: adam_kernel<EMA, B1Z>; the training setting is betas = (0, 0.99)):
the first moment is not read, m_new is the sanitised gradient, the bias correction 1 - beta1^t is 1.  ldetr_adam_ema_step_f32 picks it when
beta1 == 0.0f; every other beta1 runs the general kernel.

Sizes 1 and 3 (scalar tail only), 4 (one quad), 4096 (exactly one 1024-quad chunk), 4100 (one quad into the second chunk) and 3 * 4096 + 5 (three
chunks, one more quad and a scalar tail element); with and without the fused EMA; the sanitiser on, with NaN, +Inf and -Inf in the gradient.  Two
steps, so that the second starts from running moments.  The float64 reference, the inputs and every bound are tests/streaming_common.py's, applied
as test_streaming_kernels_gpu.py applies them (p 1e-6 max-normalised and 4 x the float32 CPU error relative to the update, m and v 4 x the float32
CPU error per element, the EMA 1e-6).  Every case prints its figures before it asserts."""
import pytest
import torch

import streaming_common as S

pytestmark = pytest.mark.gpu

S.limit_threads()
SIZES = [1, 3, 4, 4096, 4100, 3 * 4096 + 5]
BETAS0 = (0.0, 0.99)
EMA_BETA = 0.999
STEPS = 2


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def _core():
    from layoutdetr_amd.hip import core
    return core


def poisoned(g):
    """NaN, +Inf and -Inf at the second element, in the last quad, in the scalar tail and at both ends, as far as the size has room."""
    g = g.clone()
    n = g.numel()
    pos = []
    for q in (1, (n // 4) * 4 - 2, n - 1, 0, n // 2):
        if 0 <= q < n and q not in pos:
            pos.append(q)
    for k, q in enumerate(pos):
        g[q] = [float('nan'), float('inf'), -float('inf')][k % 3]
    return g


def gradient(t, step):
    return poisoned(S.step_gradient(t['g'], step))


def run_gpu(dev, t, betas, ema, m0=None, steps=STEPS):
    """-> p, m, v, p_ema (or None) after `steps` fused-sanitise steps, and the sanitised float32 gradient of the last step."""
    core = _core()
    p, v = t['p'].to(dev), t['v'].to(dev)
    m = (t['m'] if m0 is None else m0).to(dev)
    pe = t['pe'].to(dev) if ema else None
    s, n = S.SANITIZE, t['p'].numel()
    for k in range(steps):
        gd = gradient(t, k + 1).to(dev)
        args = (core.ptr(p), core.ptr(gd), core.ptr(m), core.ptr(v), n, k + 1, S.OPT_LR, betas[0], betas[1], S.OPT_EPS, 1, s['gscale'], s['nan'], s['posinf'], s['neginf'])
        if ema:
            core.check(core.lib().ldetr_adam_ema_step_f32(*args, core.ptr(pe), EMA_BETA, core.stream()), 'adam_ema_step')
        else:
            core.check(core.lib().ldetr_adam_step_f32(*args, core.stream()), 'adam_step')
        assert torch.equal(gd.cpu().nan_to_num(7.0), gradient(t, k + 1).nan_to_num(7.0)), 'g is read only'
    torch.cuda.synchronize()
    return p, m, v, pe


def run_ref(t, betas, ema, steps=STEPS):
    p, m, v, pe = t['p'], t['m'], t['v'], (t['pe'] if ema else None)
    for k in range(steps):
        p, m, v, pe = S.adam_ref(p, gradient(t, k + 1), m, v, k + 1, S.OPT_LR, betas[0], betas[1], S.OPT_EPS, S.SANITIZE, pe=pe, ema_beta=EMA_BETA if ema else None)
    return p, m, v, pe


def check(tag, got, ref, p0):
    """test_streaming_kernels_gpu._check_adam's figures and bounds, and the EMA's."""
    p, m, v, pe = got
    p64, m64, v64, pe64 = ref
    rows = [('p (max-normalised)', S.rel_err(p, p64), S.TOL_OPT_P), ('p (of the update)', S.update_rel_err(p, p64, p0), S.fp32_bound('adam_p_update')),
            ('m (per element)', S.elem_rel_err(m, m64), S.fp32_bound('adam_m')), ('v (per element)', S.elem_rel_err(v, v64), S.fp32_bound('adam_v'))]
    if pe is not None:
        rows.append(('p_ema', S.rel_err(pe, pe64), S.TOL_OPT_P))
    for name, e, tol in rows:
        print(f'[adam beta1 = 0] {tag}: {name} err {e:.3e} (bound {tol:.2e})')
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
    bad = [f'{name}: {e:.3e} > {tol:.2e}' for name, e, tol in rows if not e <= tol]
    assert not bad, f'{tag}: ' + '; '.join(bad)


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('n', SIZES)
def test_beta1_zero_vs_fp64_m_is_the_gradient_old_m_is_dead(dev, n, ema):
    t = S.optim_inputs(n, seed=n)
    got = run_gpu(dev, t, BETAS0, ema)
    check(f'n {n} ema {int(ema)}', got, run_ref(t, BETAS0, ema), t['p'])
    s = S.SANITIZE
    g32 = S.sanitize_ref(gradient(t, STEPS), s['gscale'], s['nan'], s['posinf'], s['neginf'])      # float32: scaling by 0.5 and the replacements are exact
    assert torch.equal(got[1].cpu(), g32), 'm after the step must be the sanitised gradient, bit for bit'
    # the first moment a step starts from is never read: huge finite values in it change nothing
    huge = torch.full((n,), 3.0e38)
    huge[::2] = -1.0e30
    other = run_gpu(dev, t, BETAS0, ema, m0=huge)
    for name, a, b in zip(('p', 'm', 'v', 'p_ema'), got, other):
        if a is not None:
            assert torch.equal(a, b), f'{name} depends on the first moment the step started from'


def test_beta1_0_9_is_still_the_general_step(dev):
    """One case through the general kernel: beta1 = 0.9 at the same bounds, with the EMA, the chunk boundary and the non-finite gradients."""
    n = 4100
    t = S.optim_inputs(n, seed=n)
    betas = S.OPT_BETAS[0]
    assert betas[0] == 0.9
    for ema in (False, True):
        check(f'beta1 0.9 n {n} ema {int(ema)}', run_gpu(dev, t, betas, ema), run_ref(t, betas, ema), t['p'])
