"""The float64 references of tests/token_rows_common.py against torch's own float64 evaluation (F.layer_norm with autograd on the explicitly formed
sum, F.cross_entropy with ignore_index and label_smoothing, nn.Embedding with padding_idx), the recorded float32 yardsticks re-measured, the proof
that every host-side path of every token-row kernel family is reached by at least one case of the tables that tests/test_token_rows_gpu.py runs,
and the proof that three plausible mistakes move a reference by more than 100 x the bound it is held to.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as F

import token_rows_common as R

R.limit_threads()
REF_TOL = 1e-13


def union(sets):
    out = set()
    for s in sets:
        out |= s
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize('D,fwd_slices,bias,p,use_dy2,bwd_slices', [(256, 0, False, 0.0, False, 0), (256, 17, True, 0.3, True, 16), (516, 9, True, 0.1, False, 9),
                                                                    (4, 1, True, 0.3, True, 1), (1024, 2, False, 0.0, True, 0)])
def test_layernorm_refs_are_torch_layer_norm_and_its_autograd(D, fwd_slices, bias, p, use_dy2, bwd_slices):
    rows = 18
    t = R.ln_inputs(rows, D, fwd_slices, bwd_slices)
    drop = R.drop_rows(0x1234, -77, p, rows, D)
    auto = R.ln_autograd_ref(t, fwd_slices, bias, drop, use_dy2, bwd_slices)
    fwd = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], fwd_slices, t['r_bias'] if bias else None, drop)
    bwd = R.ln_bwd_ref(fwd['z'], t['gamma'], t['dy'], t['dy2'] if use_dy2 else None, t['parts'], bwd_slices, drop)
    assert R.rel_err(fwd['z'], auto['z']) <= REF_TOL and R.rel_err(fwd['y'], auto['y']) <= REF_TOL
    z = auto['z']
    assert R.rel_err(fwd['mean'], z.mean(1)) <= REF_TOL and R.rel_err(fwd['rstd'], (z.var(1, unbiased=False) + R.as_f32(R.LN_EPS)).rsqrt()) <= REF_TOL
    for k in ('dx', 'dgamma', 'dbeta'):
        assert R.rel_err(bwd[k], auto[k]) <= REF_TOL, k
    for s in range(max(fwd_slices, 1)):       # every slice of the sum receives dx * drop
        assert R.rel_err(bwd['dr'], auto['dr'][s]) <= REF_TOL, s
    if p > 0:
        assert 0.5 * p < float((drop == 0).double().mean()) < 1.5 * p and float(drop.max()) == 1.0 / (1.0 - R.as_f32(p))


def test_layernorm_ref_ignores_the_bias_without_slices_and_adds_running_gradients():
    t = R.ln_inputs(5, 64, 0, 0)
    a = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], 0, t['r_bias'])
    b = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], 0, None)
    assert torch.equal(a['y'], b['y'])
    plain = R.ln_fwd_ref(t['x'], None, t['gamma'], t['beta'])
    assert R.rel_err(plain['y'], F.layer_norm(t['x'].double(), (64,), t['gamma'].double(), t['beta'].double(), R.as_f32(R.LN_EPS))) <= REF_TOL
    g0 = R.ln_bwd_ref(a['z'], t['gamma'], t['dy'])
    g1 = R.ln_bwd_ref(a['z'], t['gamma'], t['dy'], dg0=t['dg0'], db0=t['db0'])
    assert R.rel_err(g1['dgamma'], g0['dgamma'] + t['dg0'].double()) <= 1e-15 and R.rel_err(g1['dbeta'], g0['dbeta'] + t['db0'].double()) <= 1e-15


def test_layernorm_value_edges():
    D = R.LN_EDGE_D
    t = R.ln_inputs(R.LN_EDGE_ROWS, D)
    for dt in (R.F64, R.F32):
        c = R.ln_fwd_ref(torch.full((R.LN_EDGE_ROWS, D), 0.5), None, t['gamma'], t['beta'], dtype=dt)
        assert torch.equal(c['y'], t['beta'].to(dt).expand(R.LN_EDGE_ROWS, D)) and bool((c['mean'] == 0.5).all())
        assert R.rel_err(c['rstd'], torch.full((R.LN_EDGE_ROWS,), R.as_f32(R.LN_EPS) ** -0.5, dtype=R.F64)) <= 1e-6
    # rows offset by +100: E[z^2] - mean^2 in float32 loses the spread (10001 has an ulp of 1e-3), the two-pass form does not
    t = R.ln_inputs(R.LN_EDGE_ROWS, D, offset=R.LN_OFFSET)
    z = t['x']
    ref = R.ln_fwd_ref(z, None, t['gamma'], t['beta'])
    one_pass = ((z * z).mean(1) - z.mean(1) ** 2 + R.as_f32(R.LN_EPS)).rsqrt()
    two_pass = R.ln_fwd_ref(z, None, t['gamma'], t['beta'], dtype=R.F32)['rstd']
    e1, e2 = R.rel_err(one_pass, ref['rstd']), R.rel_err(two_pass, ref['rstd'])
    print(f'+100 rows, rstd in float32: one pass {e1:.3e}, two passes {e2:.3e}')
    assert e1 > 100 * e2 and e1 > 100 * R.fp32_bound('ln_rstd')


XENT_REF_CASES = [(37, 70, 0.0, 'mixed'), (37, 70, 0.1, 'mixed'), (5, 1, 0.1, 'mixed'), (5, 3, 0.0, 'mixed'), (9, 1028, 0.1, 'mixed'), (9, 1028, 0.0, 'neg_inf')]


@pytest.mark.parametrize('rows,V,eps,kind', XENT_REF_CASES)
def test_xent_ref_is_torch_cross_entropy(rows, V, eps, kind):
    x, t = R.xent_inputs(rows, V, kind)
    loss_sum, count, lse, d = R.xent_ref(x, t, R.XENT_IGNORE, eps, R.XENT_G)
    valid = (t >= 0) & (t < V)
    assert count == int(valid.sum()) and (kind != 'mixed' or rows < 8 or 0 < count < rows - 2)
    tt = torch.where(valid, t, torch.full_like(t, R.XENT_IGNORE))        # torch rejects out-of-range labels: the kernels treat them as ignored
    xr = x.double().requires_grad_(True)
    ref = F.cross_entropy(xr, tt, ignore_index=R.XENT_IGNORE, label_smoothing=R.as_f32(eps))
    (ref * R.XENT_G).backward()
    ref = ref.detach()
    assert bool(torch.isfinite(ref)) and abs(float(loss_sum) / count - float(ref)) <= REF_TOL * abs(float(ref))
    assert R.rel_err(d, xr.grad) <= REF_TOL
    assert R.rel_err(lse[valid], torch.logsumexp(x.double(), 1)[valid]) <= REF_TOL and bool((lse[~valid] == 0).all()) and bool((d[~valid] == 0).all())


def test_xent_ref_neg_inf_case_is_finite_and_all_ignored_is_zero():
    x, t = R.xent_inputs(9, 1028, 'neg_inf')
    assert bool((x[:, :8] == -math.inf).all()) and bool((x[1::2, 1024:] == -math.inf).all()) and bool(torch.isfinite(x[0::2, 1024:]).all())
    assert bool(torch.isfinite(x.gather(1, t[:, None])).all())
    for dt in (R.F64, R.F32):
        loss_sum, count, lse, d = R.xent_ref(x, t, R.XENT_IGNORE, 0.0, R.XENT_G, dt)
        assert count == 9 and bool(torch.isfinite(loss_sum)) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(d).all())
        assert bool((d[:, :8] == 0).all())
    x, t = R.xent_inputs(37, 70, 'all_ignored')
    loss_sum, count, lse, d = R.xent_ref(x, t, R.XENT_IGNORE, 0.1, R.XENT_G)
    assert float(loss_sum) == 0 and count == 0 and not bool(lse.any()) and not bool(d.any())


def test_golden_logits_are_exact_and_block0_targets_leave_one_block():
    x = R.golden_logits(R.GOLDEN_XENT['rows_sum'], R.GOLDEN_XENT['V'])
    assert torch.equal(x * 16, (x * 16).round()) and float(x.abs().max()) <= 8 and x.unique().numel() > 200
    t = R.golden_targets(R.GOLDEN_XENT['rows_sum'], R.GOLDEN_XENT['V'], only_block0=True)
    assert (t != R.XENT_IGNORE).nonzero()[:, 0].tolist() == [0, 1024, 2048]
    assert {int(r) % R.XENT_MAX_BLOCKS for r in (t != R.XENT_IGNORE).nonzero()[:, 0]} == {0}


@pytest.mark.parametrize('pad', [0, -1])
def test_embedding_ref_is_nn_embedding(pad):
    n, T, V, d = 21, 7, 50, 64
    t = R.emb_inputs(n, T, V, d, 'mixed')
    ids = t['ids']
    assert {-1, V, V + 5, 0, V - 1} <= set(ids.tolist())
    out, dw = R.embedding_ref(t['w'], ids, t['pos'], T, pad, t['dy'], t['dw0'])
    # torch: ids outside [0, V) go to an extra all-zero row V that is dropped afterwards; nn.Embedding's padding_idx None is the kernels' -1
    emb = torch.nn.Embedding(V + 1, d, padding_idx=0 if pad == 0 else None).double()
    emb.weight.data[:V] = t['w'].double()
    emb.weight.data[V] = 0
    ok = (ids >= 0) & (ids < V)
    ref = emb(torch.where(ok, ids, torch.full_like(ids, V))) + t['pos'].double()[torch.arange(n) % T]
    ref.backward(t['dy'].double())
    assert R.rel_err(out, ref) <= REF_TOL and torch.equal(out[~ok], t['pos'].double()[torch.arange(n) % T][~ok])
    assert R.rel_err(dw, t['dw0'].double() + emb.weight.grad[:V]) <= REF_TOL
    assert torch.equal(dw[0], t['dw0'][0].double()) == (pad == 0)
    out2, none = R.embedding_ref(t['w'], ids)
    assert none is None and torch.equal(out2[ok], t['w'].double()[ids[ok]]) and not bool(out2[~ok].any())


def test_sum_parts_ref_is_the_sum():
    base, parts = R.sum_parts_inputs(1028)
    assert R.rel_err(R.sum_parts_ref(base, parts, 9, 1028), base.double() + parts[:9, :1028].double().sum(0)) <= REF_TOL
    assert torch.equal(R.sum_parts_ref(None, parts, 0, 1028), torch.zeros(1028, dtype=R.F64))
    assert torch.equal(R.sum_parts_ref(None, parts, 1, 1028, R.F32), parts[0, :1028])


# ------------------------------------------------------------------------------------------------------------------------ yardsticks
def test_recorded_float32_yardsticks():
    """FP32_BASELINE is what float32 torch on this kind of CPU gives against float64.  Another CPU may sum in another order, so: the recorded
    figure is neither inflated (the re-measured one is no less than a quarter of it) nor so tight that float32 arithmetic itself would miss the
    bound derived from it."""
    got = R.measure_fp32_baselines()
    for k, rec in R.FP32_BASELINE.items():
        print(f'{k}: float32 CPU {got[k]:.3e}, recorded {rec:.3e}, bound {R.fp32_bound(k):.3e}')
    for k, rec in R.FP32_BASELINE.items():
        assert rec / R.FP32_FACTOR <= got[k] <= R.fp32_bound(k), k


# ------------------------------------------------------------------------------------------------------------------------ wrong references
@pytest.mark.parametrize('D,slices', [(256, 8), (512, 17), (256, 33)])
def test_layernorm_bound_rejects_a_missing_slice_and_a_doubled_bias(D, slices):
    rows = R.LN_SLICE_ROWS
    t = R.ln_inputs(rows, D, slices)
    good = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], slices, t['r_bias'])['y']
    short = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], slices - 1, t['r_bias'])['y']
    twice = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], slices, 2 * t['r_bias'])['y']
    e1, e2 = R.rel_err(short, good), R.rel_err(twice, good)
    print(f'D {D}, {slices} slices: one slice too few moves y by {e1:.3e}, the bias twice by {e2:.3e} (bound {R.TOL_LN["y"]:.1e})')
    assert e1 > 100 * R.TOL_LN['y'] and e2 > 100 * R.TOL_LN['y']


@pytest.mark.parametrize('pos_rows', [p for p in R.LN_POS_ROWS if p > 1])
def test_layernorm_bound_rejects_row_div_instead_of_row_mod(pos_rows):
    t = R.ln_inputs(R.LN_OPT_ROWS, R.LN_OPT_D, pos_rows=pos_rows)
    good = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], pos=t['pos'])['ypos']
    wrong = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], pos=t['pos'], pos_index='div')['ypos']
    e = R.rel_err(wrong, good)
    print(f'pos_rows {pos_rows}: row // ... moves y + pos by {e:.3e}')
    assert e > 100 * R.TOL_LN['y']


# ------------------------------------------------------------------------------------------------------------------------ path coverage
def test_every_layernorm_path_has_a_case():
    assert union(R.ln_shape_path(*c) for c in R.LN_SHAPE_CASES) == sorted(R.LN_SHAPE_PATHS)
    assert {D: R.ln_nv(D) for D in R.LN_DS} == {4: 1, 64: 1, 256: 1, 260: 2, 512: 2, 516: 3, 768: 3, 1024: 4}
    assert all('idle_lanes' in R.ln_shape_path(5, D) for D in (4, 64, 260, 516)) and all('all_lanes' in R.ln_shape_path(5, D) for D in (256, 512, 768, 1024))
    for D in (256, 1024):       # the second sweep of the backward ends in a ragged block
        assert R.ln_shape_path(2053, D) >= {'bwd_stride_loop', 'ragged_last_block'} and 2053 > R.LN_MAX_BWD_BLOCKS * R.LN_ROWS_PER_BLOCK
    got = union([R.ln_slices_path(D, s, 'fwd') for D, s in R.LN_FWD_SLICE_CASES] + [R.ln_slices_path(D, s, 'bwd') for D, s in R.LN_BWD_SLICE_CASES])
    assert got == sorted(R.LN_SLICE_PATHS)
    # exactly one full round (17 forward, 16 backward) and a round plus one
    assert R.ln_slices_path(256, 17, 'fwd') == {'fwd/PW16/one_round_full'} and R.ln_slices_path(256, 16, 'bwd') == {'bwd/PW16/one_round_full'}
    assert R.ln_slices_path(256, 18, 'fwd') == {'fwd/PW16/many_rounds_ragged'} and R.ln_slices_path(256, 17, 'bwd') == {'bwd/PW16/many_rounds_ragged'}
    assert R.ln_slices_path(512, 9, 'fwd') == {'fwd/PW8/one_round_full'} and R.ln_slices_path(768, 9, 'bwd') == {'bwd/PW8/many_rounds_ragged'}
    assert union(R.ln_group_path(*c) for c in R.LN_GROUP_CASES) == sorted(R.LN_GROUP_PATHS)
    a, b = R.LN_GROUP_MEMBERS
    assert a['fwd_slices'] != b['fwd_slices'] and a['bwd_slices'] != b['bwd_slices'] and a['p'] != b['p']
    assert R.LN_OPT_ROWS % R.LN_POS_ROWS[0] == 0 and R.LN_OPT_ROWS % R.LN_POS_ROWS[1] != 0 and R.LN_POS_ROWS[2] == 1


def test_every_sum_parts_path_has_a_case():
    assert union(R.sum_parts_path(n, s) for n in R.SUM_NS for s in R.SUM_SLICES) == sorted(R.SUM_PATHS)
    assert 'grid_stride' in R.sum_parts_path(R.SUM_NS[-1], 1) and all(n % 4 == 0 for n in R.SUM_NS)
    assert (R.SUM_NS[-1] // 4 - R.SUM_MAX_BLOCKS * 256) % 256 != 0, 'the second sweep ends inside a block'


def test_every_xent_path_has_a_case():
    assert union(R.xent_path(*c) for c in R.XENT_SHAPES) == sorted(R.XENT_PATHS)
    assert 'no_vector_part' in R.xent_path(5, 1, 3) and 'no_vector_part' in R.xent_path(5, 3, 1)
    assert R.xent_path(9, 1023, 1) >= {'vector_and_tail', 'idle_threads'} and R.xent_path(9, 1028, 64) >= {'second_quad_per_thread', 'pitch_beyond_padding'}
    assert 'second_row_per_block' in R.xent_path(1030, 70, 2) and 'third_row_per_block' in R.xent_path(2053, 258, 2)
    assert all((V + pad) % 4 == 0 for _, V, pad in R.XENT_SHAPES)
    x, t = R.xent_inputs(37, 70)
    assert {R.XENT_IGNORE, -3, 70, 75} <= set(t.tolist()) and int(((t >= 0) & (t < 70)).sum()) > 10


def test_every_embedding_path_has_a_case():
    assert union(R.emb_path(*c[:4]) for c in R.EMB_CASES) == sorted(R.EMB_PATHS)
    assert {c[4] for c in R.EMB_CASES} == {'mixed', 'one_id'} and any(c[0] % c[1] for c in R.EMB_CASES)
