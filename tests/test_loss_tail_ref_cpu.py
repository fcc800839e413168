"""The tables and float64 references of tests/loss_tail_common.py, checked without a GPU: every layout table is on the grid that makes float32 and
float64 branch alike; the per-sample shares and per-term gradients of the reference are oracle/losses_ref.py's scalar terms and their autograd;
every rule row has the property it is named after and every path name of every predicate is reached by a case that tests/test_loss_tail_gpu.py
runs; the tables are finite where they claim to be and not finite exactly where the two documented deviations say; the recorded float32 yardsticks
are re-measured; one plausible mistake per kernel family moves its reference by far more than the bound it is held to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_tail_common as R
from oracle import losses_ref as L

R.limit_threads()
REF_TOL = 1e-13


def union(sets):
    out = set()
    for s in sets:
        out |= s
    return sorted(out)


@pytest.fixture(scope='module')
def tables():
    """Every layout table with its float64 reference and predicate, computed once."""
    out = []
    for t in R.all_layout_tables():
        up = R.upstream(t['fake'].shape[0])
        losses, grads = R.oracle_layout(t['fake'], t['real'], t['valid'], up)
        paths, info = R.layout_paths(t['fake'], t['real'], t['valid'])
        out.append(dict(t, up=up, losses=losses, grads=grads, paths=paths, info=info))
    return out


# ------------------------------------------------------------------------------------------------------------------------ torch's conventions
def test_torch_subgradient_conventions_the_kernel_header_names():
    a = torch.tensor([1.0, 2.0], dtype=R.F64, requires_grad=True)
    b = torch.tensor([1.0, 3.0], dtype=R.F64, requires_grad=True)
    (torch.maximum(a, b).sum() + 10 * torch.minimum(a, b).sum()).backward()
    assert a.grad.tolist() == [5.5, 10.0] and b.grad.tolist() == [5.5, 1.0]          # ties half-half
    x = torch.tensor([[3.0, 1.0, 1.0, 2.0]], dtype=R.F64, requires_grad=True)
    x.min(-1).values.sum().backward()
    assert x.grad.tolist() == [[0.0, 1.0, 0.0, 0.0]]          # the first arg-min
    z = torch.zeros(2, dtype=R.F64, requires_grad=True)
    z.abs().sum().backward()
    assert z.grad.tolist() == [0.0, 0.0]          # sign(0) = 0
    q = torch.tensor([0.0, 2.0], dtype=R.F64, requires_grad=True)
    torch.nan_to_num(q / torch.tensor([0.0, 4.0], dtype=R.F64)).sum().backward()
    assert q.grad[0].isnan() and q.grad[1] == 0.25          # nan_to_num blocks the gradient of what it replaced; 0 / 0 behind it is still NaN


# ------------------------------------------------------------------------------------------------------------------------ tables
def test_every_layout_table_is_on_the_grid_and_inside_the_unit_square(tables):
    assert len(tables) == len(R.RULE_ROWS) + 2 * 2 * len(R.RANDOM_SHAPES)
    for t in tables:
        assert R.on_grid(t['fake']) and R.on_grid(t['real']), t['name']
        l, tp, r, b = L.xywh_to_ltrb(t['fake'].permute(2, 0, 1))
        assert float(min(l.min(), tp.min())) >= 0 and float(max(r.max(), b.max())) <= 1, t['name']          # no distance beyond 1
        assert t['fake'].shape[1] <= R.MAX_N
    assert not R.on_grid(torch.tensor([[[0.5, 0.5, 3 / 1024, 0.25]]])) and not R.on_grid(torch.tensor([[[0.3, 0.5, 0.25, 0.25]]]))
    coarse = [t for t in tables if t['name'].startswith('coarse')]
    share = sum(float(((t['fake'] == t['real']).all(-1)).sum()) for t in coarse) / sum(t['fake'].shape[0] * t['fake'].shape[1] for t in coarse)
    assert 0.25 < share < 0.4          # EQUAL_SHARE, plus the boxes that are equal by chance
    for t in coarse + [t for t in tables if t['name'].startswith('fine')]:          # padded slots hold ordinary boxes
        assert bool((t['fake'][~t['valid']][:, 2:] > 0).all())


def test_every_rule_row_has_its_property_and_every_layout_path_has_a_case(tables):
    for t in tables[:len(R.RULE_ROWS)]:
        assert t['claims'] and set(t['claims']) <= t['paths'], (t['name'], sorted(t['paths']))
    assert union(t['paths'] for t in tables) == sorted(R.LAYOUT_PATHS)
    by = {t['name']: t for t in tables}
    f = lambda n: by[n]['fake'][0].double()
    ltrb = lambda x: torch.stack(L.xywh_to_ltrb(x.T), -1)
    # gIoU rows, in the kernel's names
    A, Rr = ltrb(f('giou_touching')), ltrb(by['giou_touching']['real'][0].double())
    assert float(torch.maximum(A[0, 0], Rr[0, 0])) == float(torch.minimum(A[0, 2], Rr[0, 2]))          # l_max == r_min: cond false on an equal edge
    assert torch.equal(by['giou_equal']['fake'], by['giou_equal']['real']) and torch.equal(by['giou_equal_fine']['fake'], by['giou_equal_fine']['real'])
    assert by['giou_zero_area_equal']['losses'][1, 0].isnan() and by['giou_zero_area_equal']['grads'][1, 0, 0].isnan().all() and \
        torch.isfinite(by['giou_zero_area_equal']['grads'][1, 0, 1]).all()
    # overlap rows
    t = by['ovl_identical_pair_and_third']
    assert torch.equal(t['fake'][0, 0], t['fake'][0, 1]) and float(t['losses'][2, 0]) > 0 and bool(t['grads'][2, 0].any())
    for n in ('ovl_touching', 'ovl_covered_by_padded_only'):
        assert float(by[n]['losses'][2, 0]) == 0 and not bool(by[n]['grads'][2, 0].any()), n
    # alignment rows: who is whose first arg-min
    assert by['aln_two_neighbours_same_distance']['info']['nn'][0][0] == (1, 1)          # neighbours 1 and 2 at the same distance on xc: the first
    A = f('aln_two_neighbours_same_distance')
    assert float((A[0, 0] - A[1, 0]).abs()) == float((A[0, 0] - A[2, 0]).abs())
    assert by['aln_two_coordinates_same_distance']['info']['nn'][0] == {0: (1, 1), 1: (0, 1)}          # xc and yc at the same distance: xc
    A = f('aln_two_coordinates_same_distance')
    assert float((A[0, 0] - A[1, 0]).abs()) == float((A[0, 1] - A[1, 1]).abs())
    t = by['aln_nearest_is_padded']
    assert t['info']['nn_padded'][0] == {1} and sorted(j for j, _ in t['info']['nn'][0].values()) == [0, 1]
    s0 = float(t['up'][0]) * -1.0 / (1.0 - 6.0 / R.GRID) / 2          # box 0: xc 300 against the padded 306, two valid boxes
    assert (t['grads'][3, 0, 1] - torch.tensor([-s0, 0.0, 0.0, 0.0], dtype=R.F64)).abs().max() <= 1e-14          # the opposite gradient and nothing else
    t = by['aln_invalid_row_nearest_to_valid']
    assert t['info']['nn_padded'][0] == set() and not bool(t['grads'][3, 0, 1].any())
    t = by['aln_one_neighbour_of_several']
    assert [j for j, _ in t['info']['nn'][0].values()].count(0) >= 2
    for n in ('aln_exact', 'aln_single_box', 'aln_unit_distance'):
        assert float(by[n]['losses'][3, 0]) == 0 and by[n]['info']['nn'][0] == {}, n
    assert not bool(by['aln_exact']['grads'][3].any()) and not bool(by['aln_single_box']['grads'][3].any())
    X = f('aln_unit_distance')
    assert X.tolist() == [[0, 0, 0, 0], [1, 1, 0, 0]]
    # masks
    assert by['mask_empty_sample_in_batch']['valid'].any(1).tolist() == [True, False, True] and not bool(by['mask_nothing_valid']['valid'].any())


def test_tables_are_finite_except_where_the_two_deviations_say(tables):
    for t in tables:
        fin = bool(torch.isfinite(t['losses']).all()) and bool(torch.isfinite(t['grads']).all())
        assert fin == (t['name'] not in R.NONFINITE_RULE_ROWS), t['name']
        empty, za = R.empty_samples(t['valid']), R.zero_area(t['fake'], t['valid'])
        # deviation 1: the oracle's overlap and alignment of a sample without a valid box are NaN (mse / gIoU shares: empty sums)
        assert bool(t['losses'][2:, empty].isnan().all()) and not bool(t['losses'][:2, empty].any())
        # deviation 2: the oracle's overlap row of a valid zero-area box is NaN, every other row of the sample is finite; the loss is finite
        g = t['grads'][2]
        assert torch.equal(g.isnan().all(-1)[~empty], za[~empty]) and torch.equal(g.isnan().any(-1)[~empty], za[~empty]), t['name']
        assert bool(torch.isfinite(t['losses'][2, ~empty]).all())
        if t['name'] != 'giou_zero_area_equal':
            assert bool(torch.isfinite(t['grads'][[0, 1, 3]][:, ~empty]).all()) and bool(torch.isfinite(t['losses'][[0, 1, 3]][:, ~empty]).all()), t['name']


def test_predicate_names_the_zero_blocks_and_the_padded_neighbours(tables):
    """What the GPU file holds to exact zeros: a sample's block of a term is all zero in the reference exactly where the predicate finds no
    contribution (or, for overlap, only identical pairs, whose contributions cancel); rows of invalid slots are zero except the alignment rows
    the predicate names nearest neighbours."""
    for t in tables:
        B = t['fake'].shape[0]
        recon, cscale = R.reconstructed(t['fake'], t['real'], t['valid']), R.cancel_scale(t['fake'], t['valid'], t['up'])
        for b in range(B):
            if not bool(t['valid'][b].any()):
                continue
            for k, term in enumerate(R.TERMS):
                blk = t['grads'][k, b]
                zero = not bool(blk[torch.isfinite(blk)].any())          # (the NaN rows of deviation 2 aside)
                contrib = bool(t['info']['contrib'][k, b])
                if k == 1:
                    assert contrib != bool(recon[b])
                    if not contrib:          # exactly zero by cancellation: the float64 evaluation leaves residue
                        assert float(blk.abs().max()) <= 1e-13 * float(cscale[b]), (t['name'], b)
                    else:
                        assert not zero, (t['name'], b)
                elif k == 2:
                    assert zero == (not contrib or bool(t['info']['ovl_cancels'][b])), (t['name'], term, b)
                else:
                    assert zero == (not contrib), (t['name'], term, b)
            inv = ~t['valid'][b]
            assert not bool(t['grads'][:3, b][:, inv].any())
            named = torch.zeros_like(inv)
            named[list(t['info']['nn_padded'][b])] = True
            # (a named slot between two boxes at the same distance can still end with a zero row)
            assert not bool((t['grads'][3, b].ne(0).any(-1) & inv & ~named).any()), (t['name'], b)


# ------------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize('case', [('coarse', 0, 16, 9), ('fine', 1, 3, 9), ('fine', 0, 2, 17), ('coarse', 1, 70, 3)])
def test_layout_reference_is_the_oracle_scalar_terms_and_their_autograd(case):
    t = R.random_table(*case)
    fake, real, valid = t['fake'], t['real'], t['valid']
    up = R.upstream(fake.shape[0])
    losses, grads = R.oracle_layout(fake, real, valid, up)
    loop_l, loop_g = R.oracle_layout(fake, real, valid, up, per_box=False, chunk=5)          # the literal per-sample call, other chunking
    assert R.rel_err(losses, loop_l) <= REF_TOL and R.rel_err(grads, loop_g) <= REF_TOL
    f = fake.double().requires_grad_(True)
    r = real.double()
    terms = [F.mse_loss(f[valid], r[valid]), L.generalized_iou_loss(f[valid], r[valid]), L.compute_overlap(f, valid), L.compute_alignment(f, valid)]
    assert abs(float(losses[0].sum() - terms[0].detach())) <= REF_TOL * float(terms[0].detach()) and abs(float(losses[1].sum() - terms[1].detach())) <= REF_TOL * float(terms[1].detach())
    assert R.rel_err(losses[2], terms[2]) <= REF_TOL and R.rel_err(losses[3], terms[3]) <= REF_TOL
    # test_fused_layout_losses_match_reference_formulation's total: the four per-term gradients add up to its gradient
    u = up.double()
    w = [100.0, 4.0, 7.0, 17.0]
    (terms[0] * w[0] + terms[1] * w[1] + (terms[2] * u).sum() * w[2] + (terms[3] * u).sum() * w[3]).backward()
    unit_l, unit_g = R.oracle_layout(fake, real, valid, torch.ones_like(up))
    total = unit_g[0] * w[0] + unit_g[1] * w[1] + grads[2] * w[2] + grads[3] * w[3]
    assert R.rel_err(total, f.grad) <= 1e-12


def test_backward_reference_is_the_weighted_sum():
    grads, g = R.bwd_inputs(3, 9)
    ref = R.bwd_ref(grads, g)
    loop = sum(g[t].double()[:, None, None] * grads[t].double() for t in range(4))
    assert R.rel_err(ref, loop) <= REF_TOL and ref.shape == (3, 9, 4)


def test_combine_reference_is_the_existing_tests_chain():
    """tests/test_kernels_gpu.py::test_loss_combine_and_masked_mse_vs_torch_autograd's terms through combine_ref."""
    B, gain = 16, 0.5
    g = torch.Generator().manual_seed(716)
    mk = lambda *s: torch.randn(*s, generator=g)
    a, b, lay, sc, ce = mk(B) * 3, mk(B) * 30, mk(4, B).abs(), mk(1), torch.tensor([7.5, 3.0])
    W = [1.0, 1.0, 100.0, 4.0, 7.0, 17.0, 5.0, 50.0]
    rows = [(R.SOFTPLUS_NEG, B, False, ''), (R.SOFTPLUS, B, False, ''), (R.IDENT, B, True, ''), (R.IDENT, B, True, ''), (R.IDENT, B, False, ''), (R.IDENT, B, False, ''),
            (R.IDENT, 1, False, ''), (R.RATIO, 2, False, '')]
    xs = [a, b, lay[0], lay[1], lay[2], lay[3], sc, ce]
    total, rep, grads = R.combine_ref(rows, xs, W, gain)
    lv = [x.double().clone().requires_grad_(True) for x in xs]
    ref = [F.softplus(-lv[0]) * W[0], F.softplus(lv[1]) * W[1], lv[2].sum() * W[2], lv[3].sum() * W[3], lv[4] * W[4], lv[5] * W[5], lv[6][0] * W[6], lv[7][0] / lv[7][1] * W[7]]
    tot = sum(ref).mean() * gain
    tot.backward()
    assert abs(float(total - tot.detach())) <= REF_TOL * abs(float(tot.detach()))
    for k in range(8):
        assert R.rel_err(rep[k], ref[k]) <= REF_TOL, k
    for k in range(7):
        assert R.rel_err(grads[k], lv[k].grad) <= REF_TOL, k
    assert abs(float(grads[7][0] - lv[7].grad[0] * ce[1].double())) <= 1e-12 and float(grads[7][1]) == 0
    # softplus' branch in float64 torch: linear strictly above the threshold
    e = torch.tensor(R.SOFTPLUS_EDGES, dtype=R.F64)
    assert torch.equal(F.softplus(e)[e > 20], e[e > 20]) and float(F.softplus(e)[4]) > 20 and R.SOFTPLUS_EDGES[5] > 20 and np.float32(R.SOFTPLUS_EDGES[5]) == R.SOFTPLUS_EDGES[5]


def test_masked_mse_reference_counts_and_repeats_rows():
    a, b, valid = R.mse_inputs(18, 36, 9, 'ragged')
    loss, count, da = R.mse_ref(a, b, valid, 9, R.MSE_UP)
    full = b.double()[torch.arange(18) // 9]
    assert count == int(valid.sum()) and 0 < count < 18
    assert abs(float(loss) - float(((a.double() - full)[valid] ** 2).sum() / (count * 36))) <= REF_TOL
    assert R.rel_err(da[valid], R.MSE_UP * 2 * (a.double() - full)[valid] / (count * 36)) <= REF_TOL and not bool(da[~valid].any())
    loss, count, da = R.mse_ref(a, b, torch.zeros(18, dtype=torch.bool), 9)
    assert float(loss) == 0 and count == 0 and not bool(da.any())


def test_lsap_tables_are_what_they_claim():
    from scipy.optimize import linear_sum_assignment
    for n in R.LSAP_NS:
        c = R.lsap_inf_costs(n)
        assert np.isinf(c[0]).sum() > n and not np.isnan(c).any() and np.isfinite(c[2]).all()
        r, cc = linear_sum_assignment(c[0])
        assert np.isfinite(c[0][r, cc]).all()
        r2, cc2 = linear_sum_assignment(-c[0], maximize=True)
        assert cc2.tolist() == cc.tolist()
        with pytest.raises(ValueError):
            linear_sum_assignment(c[1])
    assert [b % R.LSAP_WAVE for b in R.LSAP_BATCHES] == [1, 1, 2] and [b // R.LSAP_WAVE for b in R.LSAP_BATCHES] == [0, 1, 2]
    assert R.LSAP_NS[0] <= 16 < R.LSAP_NS[1] <= 64


# ------------------------------------------------------------------------------------------------------------------------ yardsticks
def test_recorded_float32_yardsticks():
    """FP32_BASELINE is what the float32 oracle on this kind of CPU gives against float64.  Another CPU may sum in another order, so: the recorded
    figure is neither inflated (the re-measured one is no less than a quarter of it) nor so tight that float32 arithmetic itself would miss the
    bound derived from it."""
    got = R.measure_fp32_baselines()
    for k, rec in R.FP32_BASELINE.items():
        print(f'{k}: float32 CPU {got[k]:.3e}, recorded {rec:.3e}, bound {R.fp32_bound(k):.3e}')
    for k, rec in R.FP32_BASELINE.items():
        assert rec / R.FP32_FACTOR <= got[k] <= R.fp32_bound(k), k


# ------------------------------------------------------------------------------------------------------------------------ wrong references
def _swap(t, i, j):
    p = list(range(t.shape[1]))
    p[i], p[j] = p[j], p[i]
    return t[:, p]


def test_layout_bounds_reject_the_last_arg_min_a_one_sided_tie_and_a_skipped_padded_neighbour():
    # the last arg-min instead of the first: evaluate with neighbours 1 and 2 exchanged, then exchange the rows back
    t = R.RULE['aln_two_neighbours_same_distance']
    up = R.upstream(1)
    good_l, good_g = R.oracle_layout(t['fake'], t['real'], t['valid'], up)
    l2, g2 = R.oracle_layout(_swap(t['fake'], 1, 2), _swap(t['real'], 1, 2), t['valid'], up)
    e, _ = R.layout_errors(l2, _swap(g2.transpose(1, 2), 1, 2).transpose(1, 2), good_l, good_g, t['fake'], t['real'], t['valid'], up, kernel=False)
    print(f'last arg-min: alignment gradient moves by {e["grad_alignment"]:.3e} (bound {R.fp32_bound("grad_alignment"):.2e})')
    assert e['grad_alignment'] > 100 * R.fp32_bound('grad_alignment') and e['loss_alignment'] <= R.fp32_bound('loss_alignment')
    # a tie that sends the whole gradient to one side: the generated box moved off the tie by one grid step
    t = R.RULE['ovl_shared_left_edge']
    good_l, good_g = R.oracle_layout(t['fake'], t['real'], t['valid'], up)
    moved = t['fake'].clone()
    moved[0, 1, 0] += 2.0 / R.GRID
    l2, g2 = R.oracle_layout(moved, t['real'], t['valid'], up)
    e, _ = R.layout_errors(l2, g2, good_l, good_g, t['fake'], t['real'], t['valid'], up, kernel=False)
    print(f'one-sided tie: overlap gradient moves by {e["grad_overlap"]:.3e} (bound {R.fp32_bound("grad_overlap"):.2e})')
    assert e['grad_overlap'] > 100 * R.fp32_bound('grad_overlap')
    # a padded nearest neighbour that receives nothing
    t = R.RULE['aln_nearest_is_padded']
    good_l, good_g = R.oracle_layout(t['fake'], t['real'], t['valid'], up)
    wrong = good_g.clone()
    wrong[3, 0, 1] = 0
    e, broken = R.layout_errors(good_l, wrong, good_l, good_g, t['fake'], t['real'], t['valid'], up)
    assert e['grad_alignment'] > 100 * R.fp32_bound('grad_alignment') and not broken
    # the kernel's conventions are conditions of their own: a NaN where deviation 2 promises a zero
    t = R.RULE['ovl_zero_w_inside']
    good_l, good_g = R.oracle_layout(t['fake'], t['real'], t['valid'], up)
    kern = good_g.clone()
    kern[2, 0, 1] = 0
    assert R.layout_errors(good_l, kern, good_l, good_g, t['fake'], t['real'], t['valid'], up)[1] == []
    assert R.layout_errors(good_l, good_g, good_l, good_g, t['fake'], t['real'], t['valid'], up)[1] != []


def test_backward_bound_rejects_a_missing_second_trip():
    B, N = 1025, 64
    grads, g = R.bwd_inputs(B, N)
    ref = R.bwd_ref(grads, g)
    wrong = ref.clone().reshape(-1)
    wrong[R.BWD_THREADS * R.BWD_MAX_BLOCKS:] = 0
    assert B * N * 4 - R.BWD_THREADS * R.BWD_MAX_BLOCKS == 256 and R.rel_err(wrong.reshape(ref.shape), ref) > 100 * R.TOL_TAIL


def test_combine_bound_rejects_a_mean_for_a_sum_and_a_missing_threshold():
    rows = R.COMBINE_CASES['softplus-sum-n257']
    xs, ws = R.combine_inputs(rows)
    total, rep, grads = R.combine_ref(rows, xs, ws, 0.5)
    t2, _, g2 = R.combine_ref([(rows[0][0], rows[0][1], False, '')], xs, ws, 0.5)
    assert abs(float(t2 - total)) > 100 * R.TOL_TAIL * abs(float(total)) and R.rel_err(g2[0], grads[0]) > 100 * R.TOL_TAIL
    # softplus without its linear branch overflows float32 at x = 100: log1p(exp(100)) = inf
    x = torch.tensor(R.SOFTPLUS_EDGES, dtype=R.F32)
    assert bool(torch.isinf(torch.log1p(torch.exp(x))[-1])) and bool(torch.isfinite(F.softplus(x)).all())


def test_masked_mse_bound_rejects_the_row_count_for_the_valid_count():
    a, b, valid = R.mse_inputs(255, 1, 5, 'ragged')
    loss, count, da = R.mse_ref(a, b, valid, 5)
    assert abs(float(loss) * count / 255 - float(loss)) > 100 * R.TOL_TAIL * float(loss)


# ------------------------------------------------------------------------------------------------------------------------ path coverage
def test_every_backward_combine_and_masked_mse_path_has_a_case():
    assert union(R.bwd_path(*c) for c in R.BWD_CASES + [R.BIG]) == sorted(R.BWD_PATHS)
    assert R.bwd_path(1024, 64) == {'bwd/exact_cap'} and R.bwd_path(*R.BIG) == {'bwd/one_block_second_trip'} and R.bwd_path(2100, 64) == {'bwd/every_block_second_trip'}
    got = set()
    for name, rows in R.COMBINE_CASES.items():
        xs, _ = R.combine_inputs(rows)
        assert len(xs) == len(rows) and all(x.numel() == n for x, (_, n, _, _) in zip(xs, rows)), name
        got |= R.combine_path(rows, xs)
    assert sorted(got) == sorted(R.COMBINE_PATHS)
    mixed = R.COMBINE_CASES['K16-mixed-ratio-first-middle-last']
    assert len(mixed) == R.COMBINE_MAX_K and {r[0] for r in mixed} == {R.IDENT, R.SOFTPLUS, R.SOFTPLUS_NEG, R.RATIO}
    assert R.combine_path(mixed) >= {'K16', 'ratio_first', 'ratio_between', 'ratio_last'}
    assert all(f'{f}-{r}-n{n}' in R.COMBINE_CASES for f in ('ident', 'softplus', 'softplus_neg') for r in ('mean', 'sum') for n in (1, 2, 255, 256, 257, 1000))
    assert R.combine_path(R.COMBINE_CASES['softplus-edges'], R.combine_inputs(R.COMBINE_CASES['softplus-edges'])[0]) >= \
        {'softplus_above_threshold', 'softplus_at_threshold', 'softplus_below_threshold'}
    assert union(R.mse_path(rows, D, bdiv, m) for rows, D, N in R.MSE_SHAPES for bdiv in (1, N) for m in R.MSE_MASKS) == sorted(R.MSE_PATHS)
    assert {rows * D for rows, D, _ in R.MSE_SHAPES} >= {1, 255, 256, 257, 65536, 65537, 3 * 65536 + 5} and {D for _, D, _ in R.MSE_SHAPES} == {1, 4, 36}
    assert all(rows % N == 0 for rows, _, N in R.MSE_SHAPES)
