"""Every path of the loss-tail kernels (csrc/layout_loss.hip) against float64: layout_losses_kernel's subgradient rules on boxes that tie, touch,
nest, coincide and have no area, its masks, layout_losses_bwd_kernel up to and past its block cap, loss_combine forward / backward over every
function, reduction, trip count and term count, masked_mse over its trip and block-cap boundaries; and ldetr_lsap_f64 (csrc/lsap.hip) over ragged
waves and infinite costs, index-exact against scipy.  Tables, references and the path predicates are in tests/loss_tail_common.py;
tests/test_loss_tail_ref_cpu.py proves that the tables reach every path and that the references are torch's own float64 results.

The layout kernels run through metrics.metric_layoutnet.layout_losses_per_sample (one forward, one backward per term with the other terms' upstream
rows zero) and, past the cap, through ldetr_layout_losses_bwd_f32 itself; combine and masked_mse through hip.losses.

Exact checks: a sample without a valid box is all zero (deviation 1 from the oracle, which gives NaN); the overlap row of a valid zero-area box is
exactly zero where the oracle's is NaN (deviation 2); gIoU is NaN exactly where the oracle's is; rows of invalid slots are exactly zero except the
alignment rows of slots the predicate names nearest neighbours; a block whose reference is all zero is exactly zero.  Bounded checks: the layout
measure of loss_tail_common (per term, per sample) at 4 x the float32 oracle's own error; combine and masked_mse at the project's 2e-6.  Every case
prints its figures before it asserts.

Largest measured errors (MI355X; bound): loss shares mse 8.8e-8 (2.0e-7), gIoU 7.4e-7 (3.0e-6), overlap 1.2e-7 (5.1e-7), alignment 2.1e-7 (2.9e-7);
gradients mse 9.5e-8 (3.8e-7), gIoU 1.8e-7 (2.1e-6), overlap 5.3e-6 (2.6e-5), alignment 1.8e-7 (4.0e-7); the backward kernel 1.9e-7 of the terms'
magnitudes (4 * 2^-24 = 2.4e-7); the wrapper at 1025 x 64 0.35 of its allowance; combine 1.8e-7, masked_mse 1.7e-7 (2e-6); softplus at its edges
2.1e-9.  169 cases in 4.6 s, the slowest (the first, which loads the library) 1.0 s.

Not pinned, because float32 cannot tell: softplus' threshold from below.  For x > 15, log1p(exp(x)) - x = exp(-x) < 3.1e-7 is under half an ulp of x
(4.8e-7), so a threshold of 15 returns the same float32 values as 20 does; the edge values pin it from above (without the branch exp(100) overflows)
and pin the derivative's own threshold."""
import ctypes

import pytest
import torch

import loss_tail_common as R

pytestmark = pytest.mark.gpu

R.limit_threads()
CANARY = -1234.5


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


class Figures(object):
    """Collects (name, error, tolerance) and exact conditions, prints each, asserts them together at the end of a case."""

    def __init__(self, case):
        self.case, self.rows, self.flags = case, [], []

    def add(self, name, a, b, tol):
        self.rows.append((name, R.rel_err(a, b), tol))

    def value(self, name, e, tol):
        self.rows.append((name, e, tol))

    def exact(self, name, ok):
        self.flags.append((name, bool(ok)))

    def check(self):
        for name, e, tol in self.rows:
            print(f'[loss tail] {self.case}: {name} err {e:.3e} (bound {tol:.2e})')
        for name, ok in self.flags:
            if not ok:
                print(f'[loss tail] {self.case}: {name} NOT exact')
        bad = [f'{name}: {e:.3e} > {tol:.2e}' for name, e, tol in self.rows if not e <= tol] + [f'{name}: not exact' for name, ok in self.flags if not ok]
        assert not bad, f'{self.case}: ' + '; '.join(bad)


# ------------------------------------------------------------------------------------------------------------------------ layout terms
def run_layout(dev, t, up):
    """-> (losses [4, B], grads [4, B, N, 4]) of the kernels: one forward, then one backward per term with g[term] = up and the other rows zero."""
    from layoutdetr_amd.metrics.metric_layoutnet import layout_losses_per_sample
    fg = t['fake'].to(dev).requires_grad_(True)
    out = layout_losses_per_sample(fg, t['real'].to(dev), t['valid'].to(dev))
    grads = []
    for k in range(4):
        g = torch.zeros_like(out)
        g[k] = up.to(dev)
        grads.append(torch.autograd.grad(out, fg, g, retain_graph=True)[0])
    return out.detach().cpu(), torch.stack(grads).cpu()


def check_layout(dev, t):
    B = t['fake'].shape[0]
    up = R.upstream(B)
    ref_l, ref_g = R.oracle_layout(t['fake'], t['real'], t['valid'], up)
    _, info = R.layout_paths(t['fake'], t['real'], t['valid'])
    got_l, got_g = run_layout(dev, t, up)
    errs, broken = R.layout_errors(got_l, got_g, ref_l, ref_g, t['fake'], t['real'], t['valid'], up)
    fig = Figures(t['name'])
    for k, e in errs.items():
        fig.value(k, e, R.fp32_bound(k))
    for b in broken:
        fig.exact(b, False)
    inv = ~t['valid']
    fig.exact('rows of invalid slots are zero (mse, gIoU, overlap)', not bool(got_g[:3][:, inv].any()))
    named = torch.zeros_like(inv)
    for b in range(B):
        named[b, list(info['nn_padded'][b])] = True
    fig.exact('alignment rows of invalid slots that are nobody\'s nearest neighbour are zero', not bool(got_g[3][inv & ~named].any()))
    return fig, got_l, got_g, ref_l, ref_g


@pytest.mark.parametrize('name', [r['name'] for r in R.RULE_ROWS])
def test_layout_rule_rows(dev, name):
    t = R.RULE[name]
    fig, got_l, got_g, ref_l, ref_g = check_layout(dev, t)
    empty, za = R.empty_samples(t['valid']), R.zero_area(t['fake'], t['valid'])
    if bool(empty.any()):          # deviation 1, asserted on both sides
        fig.exact('deviation 1: zeros from the kernel', not bool(got_l[:, empty].any()) and not bool(got_g[:, empty].any()))
        fig.exact('deviation 1: NaN overlap / alignment from the oracle', bool(ref_l[2:, empty].isnan().all()))
    if bool(za.any()):          # deviation 2, asserted on both sides
        fig.exact('deviation 2: a zero overlap row from the kernel', not bool(got_g[2][za & ~R.giou_nan_rows(t['fake'], t['real'], t['valid'])].any()))
        fig.exact('deviation 2: a NaN overlap row from the oracle', bool(ref_g[2][za].isnan().all()))
        fig.exact('deviation 2: the overlap loss is finite on both sides', bool(torch.isfinite(got_l[2, ~empty]).all()) and bool(torch.isfinite(ref_l[2, ~empty]).all()))
    if name == 'giou_zero_area_equal':
        # the saved per-term gradients from the forward entry point (the backward's weighted sum carries the NaN row into every term)
        from layoutdetr_amd.hip import core
        B, N, _ = t['fake'].shape
        x, r, v = t['fake'].to(dev), t['real'].to(dev), t['valid'].to(dev).to(torch.uint8)
        losses, saved = torch.empty(4, B, device=dev), torch.empty(4, B, N, 4, device=dev)
        core.check(core.lib().ldetr_layout_losses_f32(core.ptr(x), core.ptr(r), core.ptr(v), B, N, core.ptr(losses), core.ptr(saved), core.stream()), 'layout_losses')
        saved = saved.cpu().double() * R.upstream(B).double()[None, :, None, None]
        fig.exact('gIoU NaN on both sides', bool(got_l[1, 0].isnan()) and bool(ref_l[1, 0].isnan()) and bool(saved[1, 0, 0].isnan().all()) and bool(ref_g[1, 0, 0].isnan().all()))
        fig.exact('deviation 2 on the saved gradients: a zero overlap row', not bool(saved[2, 0, 0].any()))
        fig.exact('the saved gIoU row of the other box is finite', bool(torch.isfinite(saved[1, 0, 1]).all()))
        for k in (0, 3):
            fig.add(f'saved {R.TERMS[k]} gradient', saved[k], ref_g[k], R.fp32_bound('grad_' + R.TERMS[k]))
    if name in ('aln_exact', 'aln_single_box', 'aln_unit_distance'):
        fig.exact('alignment loss and gradient are zero', not bool(got_l[3].any()) and not bool(got_g[3].any()))
    if name in ('ovl_touching', 'ovl_covered_by_padded_only'):
        fig.exact('no overlap term, no gradient', not bool(got_l[2].any()) and not bool(got_g[2].any()))
    fig.check()


@pytest.mark.parametrize('grid,seed,B,N', R.RANDOM_TABLES)
def test_layout_random_tables(dev, grid, seed, B, N):
    check_layout(dev, R.random_table(grid, seed, B, N))[0].check()


def test_layout_losses_reject_65_boxes(dev):
    from layoutdetr_amd.metrics.metric_layoutnet import layout_losses_per_sample
    t = R.random_table('fine', 0, 2, R.MAX_N)
    pad = lambda x: torch.cat([x, x[:, :1]], 1).to(dev)
    with pytest.raises(RuntimeError, match='N <= 64'):
        layout_losses_per_sample(pad(t['fake']).requires_grad_(True), pad(t['real']), pad(t['valid']))


@pytest.mark.parametrize('B,N', R.BWD_CASES)
def test_layout_backward_kernel_up_to_and_past_its_block_cap(dev, B, N):
    """ldetr_layout_losses_bwd_f32 itself on random grads [4, B, N, 4] and g [4, B] against a float64 einsum.  Bound, per element: four products
    and three additions in float32, in any order and with or without fma, err <= 4 * 2^-24 * sum_t |g_t grads_t|."""
    from layoutdetr_amd.hip import core
    grads, g = R.bwd_inputs(B, N)
    gd, gg = grads.to(dev), g.to(dev)
    out = torch.full((B * N * 4 + 64,), CANARY, device=dev)
    core.check(core.lib().ldetr_layout_losses_bwd_f32(core.ptr(gd), core.ptr(gg), B, N, core.ptr(out), core.stream()), 'layout_losses_bwd')
    got = out[:B * N * 4].reshape(B, N, 4).cpu().double()
    ref = R.bwd_ref(grads, g)
    mag = torch.einsum('tb,tbnc->bnc', g.double().abs(), grads.double().abs())
    fig = Figures(f'bwd B{B} N{N} {sorted(R.bwd_path(B, N))}')
    fig.value('worst |err| / (sum_t |g_t grads_t|)', float(((got - ref).abs() / mag).max()), 4 * 2.0 ** -24)
    fig.add('dbox', got, ref, R.TOL_TAIL)
    fig.exact('nothing written past the end', bool((out[B * N * 4:] == CANARY).all()))
    fig.check()


@pytest.fixture(scope='module')
def big_reference():
    t = R.random_table('fine', 0, *R.BIG)
    up = R.upstream(R.BIG[0])
    return t, up, R.oracle_layout(t['fake'], t['real'], t['valid'], up, chunk=64)


def test_layout_wrapper_past_the_backward_cap(dev, big_reference):
    """One forward and ONE backward (all four upstream rows = up) at B = 1025, N = 64 against the chunked oracle.  The gradient is the sum of the
    four per-term gradients, so per sample its error is bounded by sum_t fp32_bound(grad_t) * max |reference block of term t| (each term's own
    bound in the measure of loss_tail_common) plus the float32 sum of four terms (4 * 2^-24 of their magnitudes)."""
    from layoutdetr_amd.metrics.metric_layoutnet import layout_losses_per_sample
    t, up, (ref_l, ref_g) = big_reference
    assert R.bwd_path(*R.BIG) == {'bwd/one_block_second_trip'}
    fg = t['fake'].to(dev).requires_grad_(True)
    out = layout_losses_per_sample(fg, t['real'].to(dev), t['valid'].to(dev))
    out.backward(up.to(dev)[None].expand(4, -1).contiguous())
    got_l, got_g = out.detach().cpu().double(), fg.grad.cpu().double()
    fig = Figures('wrapper B1025 N64')
    for k, term in enumerate(R.TERMS):
        fig.value('loss_' + term, float((got_l[k] - ref_l[k]).abs().max() / ref_l[k].abs().max()), R.fp32_bound('loss_' + term))
    block = ref_g.abs().amax((2, 3))          # [4, B]
    allowed = sum((R.fp32_bound('grad_' + term) + 4 * 2.0 ** -24) * block[k] for k, term in enumerate(R.TERMS))
    fig.value('worst per-sample |err| / allowed', float(((got_g - ref_g.sum(0)).abs().amax((1, 2)) / allowed).max()), 1.0)
    fig.exact('rows of invalid slots that are nobody\'s nearest neighbour are zero', not bool(got_g[(~t['valid']) & ~ref_g[3].ne(0).any(-1)].any()))
    fig.check()


# ------------------------------------------------------------------------------------------------------------------------ combine
def run_combine(dev, rows, xs, ws, gain):
    from layoutdetr_amd.hip import losses as hl
    leaves = [x.to(dev).requires_grad_(True) for x in xs]
    terms = [hl.Term(f't{k}', x, w, fn, red) for k, ((fn, n, red, _), x, w) in enumerate(zip(rows, leaves, ws))]
    total, rep = hl.combine(terms, gain)
    total.backward()
    return total.detach(), [rep[f't{k}'].detach() for k in range(len(rows))], [x.grad for x in leaves]


@pytest.mark.parametrize('gain', R.COMBINE_GAINS)
@pytest.mark.parametrize('name', list(R.COMBINE_CASES))
def test_combine_every_function_reduction_trip_and_term_count(dev, name, gain):
    rows = R.COMBINE_CASES[name]
    xs, ws = R.combine_inputs(rows)
    ref_total, ref_rep, ref_grads = R.combine_ref(rows, xs, ws, gain)
    total, rep, grads = run_combine(dev, rows, xs, ws, gain)
    fig = Figures(f'combine {name} gain {gain}')
    fig.add('total', total, ref_total, R.TOL_TAIL)
    for k in range(len(rows)):
        fig.add(f'value {k}', rep[k], ref_rep[k], R.TOL_TAIL)
        fig.add(f'gradient {k}', grads[k], ref_grads[k], R.TOL_TAIL)
        fig.exact(f'row {k} finite', bool(torch.isfinite(rep[k]).all()) and bool(torch.isfinite(grads[k]).all()))
        if rows[k][0] == R.RATIO:
            fig.exact(f'row {k}: no gradient to the count', float(grads[k][1]) == 0.0)
    fig.check()


def test_combine_softplus_edges_value_by_value(dev):
    """softplus(+-x) at and around its threshold, each value against float64 on its own scale (the batch-wide measure would hide 20 behind 100):
    values 2e-6 relative with the float32 denormal floor, derivatives 2e-6 absolute (they lie in [0, 1])."""
    rows = R.COMBINE_CASES['softplus-edges']
    xs, _ = R.combine_inputs(rows)
    ws = [1.0, 1.0]
    _, ref_rep, ref_grads = R.combine_ref([(R.SOFTPLUS, 8, False, ''), (R.SOFTPLUS_NEG, 8, False, '')], xs, ws, 1.0)
    _, rep, grads = run_combine(dev, [(R.SOFTPLUS, 8, False, ''), (R.SOFTPLUS_NEG, 8, False, '')], xs, ws, 1.0)
    fig = Figures('softplus edges')
    for k, sgn in ((0, 1.0), (1, -1.0)):
        for i, x in enumerate(R.SOFTPLUS_EDGES):
            v, r = float(rep[k][i]), float(ref_rep[k][i])
            fig.value(f'softplus({sgn * x:+.7g})', abs(v - r), R.TOL_TAIL * abs(r) + 2.0 ** -126)
            fig.value(f'd softplus({sgn * x:+.7g})', abs(float(grads[k][i]) * 8 - float(ref_grads[k][i]) * 8), R.TOL_TAIL)
    fig.check()


def test_combine_rejects_17_rows(dev):
    from layoutdetr_amd.hip import losses as hl
    x = torch.ones(3, device=dev)
    with pytest.raises(ValueError, match='at most 16'):
        hl.combine([hl.Term(f't{k}', x) for k in range(17)])
    with pytest.raises(ValueError, match='at most 16'):
        hl.combine([hl.Term(['a', 'b', 'c', 'd'], torch.ones(4, 3, device=dev), [1.0] * 4, hl.IDENT, [False] * 4)] * 4 + [hl.Term('e', x)])


# ------------------------------------------------------------------------------------------------------------------------ masked mse
@pytest.mark.parametrize('rows,D,N', R.MSE_SHAPES)
def test_masked_mse_trip_and_block_cap_boundaries(dev, rows, D, N):
    from layoutdetr_amd.hip import losses as hl
    fig = Figures(f'masked mse rows {rows} D {D}')
    for bdiv in sorted({1, N}):
        for mask in R.MSE_MASKS:
            a, b, valid = R.mse_inputs(rows, D, bdiv, mask)
            ref_loss, count, ref_da = R.mse_ref(a, b, valid, bdiv, R.MSE_UP)
            ag = a.to(dev).requires_grad_(True)
            loss = hl.masked_mse(ag, b.to(dev), valid.to(dev).to(torch.uint8), bdiv=bdiv)
            (loss * R.MSE_UP).backward()
            tag = f'bdiv {bdiv} {mask} {sorted(R.mse_path(rows, D, bdiv, mask))}'
            da = ag.grad.cpu()
            if count == 0:
                fig.exact(f'{tag}: loss and gradient are zero', float(loss.detach()) == 0.0 and not bool(da.any()))
                continue
            fig.add(f'{tag}: loss', loss, ref_loss, R.TOL_TAIL)
            fig.add(f'{tag}: d a', da, ref_da, R.TOL_TAIL)
            fig.exact(f'{tag}: rows that are not valid get a zero gradient', not bool(da[~valid].any()))
    fig.check()


def test_masked_mse_without_rows(dev):
    """rows == 0 through the entry points (an empty tensor has no address to hand over): the forward writes 0 and count 0, the backward launches
    nothing and leaves its output alone."""
    from layoutdetr_amd.hip import core
    buf = torch.full((8,), CANARY, device=dev)
    valid = torch.ones(8, dtype=torch.uint8, device=dev)
    out, g = torch.full((2,), CANARY, device=dev), torch.ones(1, device=dev)
    da = torch.full((8,), CANARY, device=dev)
    core.check(core.lib().ldetr_masked_mse_fwd_f32(core.ptr(buf), core.ptr(buf), core.ptr(valid), ctypes.c_int64(0), 4, 1, core.ptr(out), core.stream()), 'masked_mse_fwd')
    core.check(core.lib().ldetr_masked_mse_bwd_f32(core.ptr(buf), core.ptr(buf), core.ptr(valid), ctypes.c_int64(0), 4, 1, core.ptr(out), core.ptr(g), core.ptr(da), core.stream()),
               'masked_mse_bwd')
    assert out.tolist() == [0.0, 0.0] and bool((da == CANARY).all())


# ------------------------------------------------------------------------------------------------------------------------ LSAP
def run_lsap(dev, cost, maximize):
    from layoutdetr_amd.hip import core
    batch, n, _ = cost.shape
    c = torch.from_numpy(cost).to(dev)
    ri = torch.full((batch + 1, n), -7, dtype=torch.int32, device=dev)
    ci = torch.full_like(ri, -7)
    core.check(core.lib().ldetr_lsap_f64(core.ptr(c), batch, n, int(maximize), core.ptr(ri), core.ptr(ci), core.stream()), 'lsap')
    assert bool((ri[batch] == -7).all()) and bool((ci[batch] == -7).all()), 'written past the last problem'
    return ri[:batch].cpu().numpy(), ci[:batch].cpu().numpy()


@pytest.mark.parametrize('n', R.LSAP_NS)
@pytest.mark.parametrize('batch', R.LSAP_BATCHES)
def test_lsap_ragged_waves_match_scipy(dev, batch, n):
    from scipy.optimize import linear_sum_assignment
    cost = R.lsap_costs(batch, n)
    for maximize in (False, True):
        ri, ci = run_lsap(dev, cost, maximize)
        for b in range(batch):
            r, c = linear_sum_assignment(cost[b], maximize=maximize)
            assert ri[b].tolist() == r.tolist() and ci[b].tolist() == c.tolist(), (b, maximize)


@pytest.mark.parametrize('n', R.LSAP_NS)
def test_lsap_infinite_costs_and_one_infeasible_problem(dev, n):
    from scipy.optimize import linear_sum_assignment
    cost = R.lsap_inf_costs(n)
    for maximize in (False, True):
        c = -cost if maximize else cost
        ri, ci = run_lsap(dev, c, maximize)
        for b in (0, 2):
            r, cc = linear_sum_assignment(c[b], maximize=maximize)
            assert ri[b].tolist() == r.tolist() and ci[b].tolist() == cc.tolist(), (b, maximize)
        with pytest.raises(ValueError):
            linear_sum_assignment(c[1], maximize=maximize)
        assert ri[1].tolist() == [-1] * n and ci[1].tolist() == [-1] * n
