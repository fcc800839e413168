"""The float64 references of tests/streaming_common.py against torch's own float64 evaluation (torch.optim.Adam, Tensor.lerp, torch.nan_to_num, autograd
of the toRGB einsum, F.gelu), the recorded float32 yardsticks re-measured, and the proof that every host-side path of every streaming-kernel family
is reached by at least one case of the tables that tests/test_streaming_kernels_gpu.py runs.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as F

import streaming_common as S

S.limit_threads()


# ------------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize('betas', S.OPT_BETAS)
def test_adam_ref_is_torch_adam(betas):
    t = S.optim_inputs(4103, seed=3)
    b1, b2 = S.as_f32(betas[0]), S.as_f32(betas[1])
    pr = t['p'].double().clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=S.as_f32(S.OPT_LR), betas=(b1, b2), eps=S.as_f32(S.OPT_EPS))
    for step in (1, 2, 3):
        pr.grad = S.step_gradient(t['g'], step).double()
        opt.step()
    p, m, v = S.adam_run(t, 3, betas, fuse=0)
    st = opt.state[pr]
    assert S.rel_err(p, pr) <= 1e-14 and S.elem_rel_err(m, st['exp_avg']) <= 1e-13 and S.elem_rel_err(v, st['exp_avg_sq']) <= 1e-13
    assert float((p - t['p'].double()).abs().max()) > 0.1, 'three steps at lr 0.05 move the parameters by about 0.15'


def test_adam_ref_sanitises_like_nan_to_num_and_lerps_like_torch():
    t = S.optim_inputs(4103, seed=4)
    g = S.poison(t['g'])
    assert int((~torch.isfinite(g)).sum()) == 3
    s = S.SANITIZE
    want = torch.nan_to_num(g.double() * s['gscale'], nan=s['nan'], posinf=s['posinf'], neginf=s['neginf'])
    assert torch.equal(S.sanitize_ref(g.double(), s['gscale'], s['nan'], s['posinf'], s['neginf']), want)
    assert torch.equal(S.sanitize_ref(g, s['gscale'], s['nan'], s['posinf'], s['neginf']), want.float()), 'exact in float32 as well'
    p, m, v, pe = S.adam_ref(t['p'], g, t['m'], t['v'], 1, S.OPT_LR, 0.9, 0.999, S.OPT_EPS, sanitize=s, pe=t['pe'], ema_beta=0.75)
    p2, m2, v2, _ = S.adam_ref(t['p'], want, t['m'], t['v'], 1, S.OPT_LR, 0.9, 0.999, S.OPT_EPS)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2) and bool(torch.isfinite(p).all())
    assert S.rel_err(pe, p.lerp(t['pe'].double(), 0.75)) <= 1e-15
    assert S.rel_err(S.ema_ref(t['pe'], t['p'], 0.75), t['p'].double().lerp(t['pe'].double(), 0.75)) <= 1e-15


def test_torgb_refs_are_the_autograd_of_the_einsum():
    t = {k: v.double() for k, v in S.torgb_inputs(3, 37, 96).items()}
    x, w, s, bias = [t[k].clone().requires_grad_(True) for k in ('x', 'w', 's', 'bias')]
    y = torch.einsum('bpc,oc,bc->bpo', x, w, s) + bias
    assert S.rel_err(S.torgb_fwd_ref(t['x'], t['w'], t['s'], t['bias']), y) <= 1e-15
    dx, dw, ds, db = torch.autograd.grad(y, (x, w, s, bias), t['dy'])
    rdx, rdws, rdb = S.torgb_bwd_ref(t['x'], t['dy'], t['w'], t['s'])
    rdw, rds = S.torgb_finish_ref(rdws, t['s'], t['w'], t['dw0'])
    assert S.rel_err(rdx, dx) <= 1e-14 and S.rel_err(rdb, db) <= 1e-14
    assert S.rel_err(rdw, t['dw0'] + dw) <= 1e-14 and S.rel_err(rds, ds) <= 1e-14


def test_bias_act_ref_gelu_and_gradient_orders():
    c = next(c for c in S.BIAS_ACT_CASES if c['name'] == 'gelu-grad1')
    x, b, dy, ddx = S.bias_act_inputs(c)
    y, dx, _ = S.bias_act_ref(x, b, c['axis'], 'gelu', c['alpha'], c['gain'], c['clamp'], dy=dy)
    xr = x.double().requires_grad_(True)
    yr = F.gelu(xr + b.double())
    assert S.rel_err(y, yr) <= 1e-14
    assert S.rel_err(dx, torch.autograd.grad(yr, xr, dy.double())[0]) <= 1e-14
    # second order against the closed form: y = gain tanh(x + b): d_x = ddx dy gain (-2 t (1 - t^2))
    y, dx, d_x = S.bias_act_ref(x, b, 1, 'tanh', 0.0, 1.3, None, dy=dy, ddx=ddx)
    tt = torch.tanh(x.double() + b.double())
    assert S.rel_err(dx, dy.double() * 1.3 * (1 - tt * tt)) <= 1e-13
    assert S.rel_err(d_x, ddx.double() * dy.double() * 1.3 * (-2 * tt * (1 - tt * tt))) <= 1e-13
    # the clamp removes the gradient where it binds
    y, dx, _ = S.bias_act_ref(x, b, 1, 'lrelu', 0.2, math.sqrt(2), 0.9, dy=dy)
    assert float(y.abs().max()) == 0.9 and bool((dx[y.abs() >= 0.9] == 0).all()) and bool((dx[y.abs() < 0.9] != 0).any())


def test_maxpool_ref_routes_all_neg_inf_windows_to_the_first_in_image_element():
    x = torch.full((1, 1, 4, 4), -math.inf)
    _, dx = S.maxpool_ref(x, torch.ones(1, 1, 2, 2))
    want = torch.zeros(4, 4, dtype=torch.float64)
    want[0, 0] = want[0, 1] = want[1, 0] = want[1, 1] = 1.0
    assert torch.equal(dx[0, 0], want)


# ------------------------------------------------------------------------------------------------------------------------ yardsticks
def test_recorded_float32_yardsticks():
    """FP32_BASELINE is what float32 torch on this kind of CPU gives against float64 (recorded with the past-the-cap case included).  Another CPU
    may sum in another order, so: the recorded figure is neither inflated (the re-measured one is no less than a quarter of it) nor so tight that
    float32 arithmetic itself would miss the bound derived from it."""
    got = S.measure_fp32_baselines(include_big=False)
    for k, rec in S.FP32_BASELINE.items():
        print(f'{k}: float32 CPU {got[k]:.3e}, recorded {rec:.3e}, bound {S.fp32_bound(k):.3e}')
        assert rec / S.FP32_FACTOR <= got[k] <= S.fp32_bound(k), k


# ------------------------------------------------------------------------------------------------------------------------ path coverage
def covered(paths):
    return sorted(set(paths))


def test_every_optimiser_path_has_a_case():
    got = covered(S.optim_path(n) for n in S.OPT_SIZES + [S.OPT_BIG])
    assert got == ['many_rounds', 'one_round']
    assert all(S.optim_path(n) == 'one_round' for n in S.OPT_SIZES), 'the parametrised sizes stay small; one case per entry point goes past the cap'
    n4 = S.OPT_BIG // 4
    assert S.OPT_BIG % 4 == 3 and n4 % S.STREAM_CHUNK4 == 37 and n4 // S.STREAM_CHUNK4 == S.STREAM_MAX_BLOCKS + 3
    pos = S.nonfinite_positions(S.OPT_BIG)
    assert any(S.STREAM_MAX_BLOCKS * S.STREAM_CHUNK4 * 4 <= q < (S.STREAM_MAX_BLOCKS + 1) * S.STREAM_CHUNK4 * 4 for q in pos), 'a second-round chunk'
    assert 0 < min(pos) < 4 and max(pos) == S.OPT_BIG - 1
    assert {n % 4 for n in S.OPT_SIZES} == {0, 1, 3} and 4096 in S.OPT_SIZES


def test_every_bias_act_path_has_a_case():
    got = covered(S.bias_act_path(c) for c in S.BIAS_ACT_CASES)
    assert got == sorted(S.BIAS_ACT_PATHS)
    cross = {(c['name'].split('-')[0], c['act'], c['grad']) for c in S.BIAS_ACT_CASES if c['name'].count('-') == 2 and c['name'].split('-')[0] in S.BIAS_FORMS}
    for form in S.BIAS_FORMS:
        for act in S.ACTS:
            for grad in (0, 1, 2):
                if grad < 2 or act in S.HAS_2ND:
                    assert (form, act, grad) in cross
    for form in S.BIAS_FORMS:      # the cross cases take the form their name says
        assert {S.bias_act_path(c) for c in S.BIAS_ACT_CASES if c['name'].startswith(form + '-')} == {form + '/single_round'}
    nt = [c for c in S.BIAS_ACT_CASES if S.bias_act_path(c).endswith('non_temporal')]
    assert len(nt) == 1 and math.prod(nt[0]['dims']) == 2 ** 25 and nt[0]['act'] == 'lrelu' and nt[0]['grad'] == 1
    assert {(c['grad'], c['inplace']) for c in S.BIAS_ACT_CASES if c['act'] == 'gelu'} >= {(0, True), (0, False), (1, False)}


def test_every_torgb_path_has_a_case():
    assert covered(S.torgb_fwd_case_path(c) for c in S.TORGB_FWD_CASES) == sorted(S.TORGB_FWD_PATHS)
    assert covered(S.torgb_bwd_path(*c) for c in S.TORGB_BWD_CASES) == sorted(S.TORGB_BWD_PATHS)
    assert S.torgb_bwd_path(3, 37, 96) == 'RL10/idle_threads/gz1' and S.torgb_bwd_path(1, 16 * 1025 + 3, 1028) == 'RL1/gz2/rows_doubled'
    ends = [S.finish_last_blocks(B, C) for B, C in S.TORGB_FINISH_CASES]
    assert any(dw > ds for dw, ds, _ in ends) and any(ds > dw for dw, ds, _ in ends), 'dw and ds end in different blocks, either way round'
    assert {B for B, _ in S.TORGB_FINISH_CASES} >= {1, 2, 5}


def test_every_maxpool_path_has_a_case():
    got = [S.maxpool_path(N, H, W, C, d) for (N, H, W, C, _) in S.POOL_CASES for d in ('fwd', 'bwd')]
    got += [S.maxpool_path(*S.POOL_BIG_FWD[:4], 'fwd'), S.maxpool_path(*S.POOL_BIG_BWD[:4], 'bwd')]
    assert covered(got) == sorted(S.POOL_PATHS)
    assert S.maxpool_path(*S.POOL_BIG_FWD[:4], 'fwd') == 'fwd/stride_loop' and S.maxpool_path(*S.POOL_BIG_BWD[:4], 'bwd') == 'bwd/stride_loop'
    assert {k for *_, k in S.POOL_CASES} == set(S.POOL_KINDS)
    x, _ = S.pool_inputs(2, 13, 12, 8, 'negative')
    assert float(x.max()) < 0
    x, _ = S.pool_inputs(2, 13, 12, 8, 'nonfinite')
    assert int(x.isnan().sum()) == 1 and int((x == math.inf).sum()) == 1 and int((x == -math.inf).sum()) == 1
