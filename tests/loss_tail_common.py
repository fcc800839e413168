"""What tests/test_loss_tail_ref_cpu.py and tests/test_loss_tail_gpu.py share for the loss-tail kernels (csrc/layout_loss.hip: layout_losses /
layout_losses_bwd, loss_combine fwd / bwd, masked_mse fwd / bwd) and for the device Hungarian solve behind the same loss path (csrc/lsap.hip):
the case tables, float64 references and one predicate per kernel family that restates the kernel's branch selection and names the paths a case
takes.  The CPU file asserts that every path name is reached by a table case and that every rule row has the property it is named after; the GPU
file runs the tables.  Nothing here touches the GPU or the kernel library.

Layout boxes live on a grid: centres are integers / 1024, widths and heights even integers / 1024, so x +- w / 2, every coordinate difference and
every area (20-bit numerators) is exact in float32: float32 and float64 take the same branch at every comparison, ties included.  Padded slots hold
ordinary boxes.

The layout reference is oracle/losses_ref.py (pinned by tests/test_oracle_golden.py) in float64 through autograd.  The kernel differs from it in
two places, both kept on purpose (a NaN would zero the whole step behind the gradient sanitiser) and both asserted by the GPU file:
  1. a sample without a valid box: the kernel writes 0 for its four shares and a zero gradient, the oracle's overlap / alignment are 0 / 0 = NaN;
  2. a valid box of zero area: the kernel gives that box a zero overlap gradient, the oracle's row for it is NaN (0 * inf behind nan_to_num).

Measure of the layout checks: a loss share against the largest |reference| of its term over the batch; a gradient per term and per sample against
the largest |reference| of that sample's [N, 4] block, a block whose reference is all zero being exactly zero.  That measure has no project bound:
FP32_BASELINE records what the oracle itself gives in float32 on the CPU against float64 over the tables, the GPU file allows FP32_FACTOR x that
(other summation order, fma contraction, logf / expf), the CPU file re-measures."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses_ref as L

F64, F32 = torch.float64, torch.float32
GRID = 1024
U = GRID // 8          # the coarse grid: centres and sizes in eighths
TERMS = ('mse', 'giou', 'overlap', 'alignment')


def limit_threads():
    """CPU references: more threads than this are slower on many-core hosts."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel_err(a, b):
    """max |a - b| / max |b|, the suite's measure."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


# Bounds the project already has, in rel_err's measure (tests/test_kernels_gpu.py).
TOL_TAIL = 2e-6           # test_loss_combine_and_masked_mse_vs_torch_autograd

# float32 oracle on the CPU against the float64 oracle, worst case over RULE_ROWS and RANDOM_TABLES in the measure above (measure_fp32_baselines;
# the CPU file re-measures them); the GPU file allows FP32_FACTOR x these.  -log(1 - m) carries an absolute error of about one float32 ulp of 1
# per box whatever m is, against alignment terms that are small where boxes nearly align: the alignment loss figure is that, not slack.
# The overlap gradient figure comes from small boxes nested in large ones (fine grid): ai / a1 is constant there, its two partial derivatives of size
# 1 / w cancel, and the float32 residue of that is measured against what is left of the sample's block.
FP32_BASELINE = dict(loss_mse=5.04e-8, loss_giou=7.38e-7, loss_overlap=1.28e-7, loss_alignment=7.32e-8,
                     grad_mse=9.54e-8, grad_giou=5.17e-7, grad_overlap=6.41e-6, grad_alignment=1.01e-7)
FP32_FACTOR = 4.0      # -> bounds 2.0e-7, 3.0e-6, 5.1e-7, 2.9e-7, 3.8e-7, 2.1e-6, 2.6e-5, 4.0e-7


def fp32_bound(key):
    return FP32_FACTOR * FP32_BASELINE[key]


# ------------------------------------------------------------------------------------------------------------------------ layout tables
def boxes(rows):
    """[..., 4] grid integers (xc, yc, w, h) -> float32 boxes."""
    return torch.tensor(rows, dtype=torch.int64).to(F32) / GRID


def shifted(fake):
    """The default reference boxes of a rule row that pins a term of the generated boxes alone: no edge in common with them."""
    return fake + torch.tensor([2.0, -4.0, 8.0, 2.0]) / GRID          # edges move by -2, -5, +6, -3 grid steps


def _row(name, fake, valid=None, real=None, claims=()):
    fake = boxes(fake)
    if fake.dim() == 2:
        fake = fake[None]
    B, N, _ = fake.shape
    valid = torch.ones(B, N, dtype=torch.bool) if valid is None else torch.tensor(valid, dtype=torch.bool).reshape(B, N)
    real = shifted(fake) if real is None else boxes(real).reshape(B, N, 4)
    return dict(name=name, fake=fake, real=real, valid=valid, claims=tuple(claims))


A0 = [4 * U, 4 * U, 2 * U, 2 * U]          # edges 3/8 .. 5/8 both ways
# name -> the rule it pins; claims: path names (layout_paths) the CPU file requires of the row
RULE_ROWS = [
    # ---- gIoU
    _row('giou_equal', [A0, [2 * U, 5 * U, U, 3 * U]], real=[A0, [2 * U, 5 * U, U, 3 * U]], claims=['giou/all_eight_ties']),
    _row('giou_equal_fine', [[401, 387, 222, 146], [640, 555, 98, 310]], real=[[401, 387, 222, 146], [640, 555, 98, 310]], claims=['giou/all_eight_ties']),
    _row('giou_touching', [[3 * U, 4 * U, 2 * U, 2 * U]], real=[[5 * U, 4 * U, 2 * U, 2 * U]], claims=['giou/touching']),
    _row('giou_fake_in_real', [[3 * U, 4 * U, 2 * U, 2 * U]], real=[[4 * U, 4 * U, 4 * U, 4 * U]], claims=['giou/fake_in_real', 'giou/nested_one_shared_edge']),
    _row('giou_real_in_fake', [[4 * U, 4 * U, 4 * U, 4 * U]], real=[[3 * U, 4 * U, 2 * U, 2 * U]], claims=['giou/real_in_fake', 'giou/nested_one_shared_edge']),
    _row('giou_disjoint', [[2 * U, 2 * U, 2 * U, 2 * U]], real=[[6 * U, 6 * U, 2 * U, 2 * U]], claims=['giou/disjoint']),
    _row('giou_zero_area_equal', [[4 * U, 4 * U, 0, 2 * U], [2 * U, 2 * U, 2 * U, U]], real=[[4 * U, 4 * U, 0, 2 * U], [2 * U + 6, 2 * U, 2 * U, U + 4]],
         claims=['giou/nan_zero_area_equal', 'ovl/zero_area_row']),
    # ---- overlap
    _row('ovl_identical_pair_and_third', [A0, A0, [5 * U, 5 * U, 2 * U, 2 * U]], claims=['ovl/identical_pair', 'ovl/pair']),
    _row('ovl_shared_left_edge', [[4 * U, 4 * U, 4 * U, 4 * U], [3 * U, 4 * U, 2 * U, 2 * U]], claims=['ovl/pair_edge_tie']),
    _row('ovl_touching', [[3 * U, 4 * U, 2 * U, 2 * U], [5 * U, 4 * U, 2 * U, 2 * U]], claims=['ovl/touching', 'ovl/no_term']),
    _row('ovl_covered_by_padded_only', [A0, [4 * U, 4 * U, 4 * U, 4 * U]], valid=[1, 0], claims=['ovl/padded_overlap_skipped', 'ovl/no_term']),
    _row('ovl_three_mutual', [[400, 400, 300, 300], [500, 450, 260, 280], [450, 520, 320, 200]], claims=['ovl/pair']),
    _row('ovl_zero_w_inside', [[4 * U, 4 * U, 4 * U, 4 * U], [3 * U, 5 * U, 0, 2 * U], [5 * U, 5 * U, 2 * U, 2 * U]], claims=['ovl/zero_area_row', 'ovl/pair_edge_tie']),
    _row('ovl_zero_h_inside', [[4 * U, 4 * U, 4 * U, 4 * U], [3 * U, 5 * U, 2 * U, 0], [5 * U, 5 * U, 2 * U, 2 * U]], claims=['ovl/zero_area_row', 'ovl/pair_edge_tie']),
    _row('ovl_zero_both_inside', [[4 * U, 4 * U, 4 * U, 4 * U], [3 * U, 5 * U, 0, 0], [5 * U, 5 * U, 2 * U, 2 * U]], claims=['ovl/zero_area_row', 'ovl/pair_edge_tie']),
    # ---- alignment
    _row('aln_exact', [[3 * U, 2 * U, 2 * U, 2 * U], [4 * U, 6 * U, 4 * U, 2 * U]], claims=['aln/exact_m0']),
    _row('aln_two_neighbours_same_distance', [[512, 200, 100, 50], [502, 500, 40, 60], [522, 800, 44, 70]], claims=['aln/tie_over_j']),
    _row('aln_two_coordinates_same_distance', [[512, 200, 100, 50], [522, 210, 160, 110]], claims=['aln/tie_over_c']),
    _row('aln_nearest_is_padded', [[300, 300, 100, 100], [306, 320, 60, 40], [100, 100, 40, 40]], valid=[1, 0, 1], claims=['aln/nn_padded']),
    _row('aln_invalid_row_nearest_to_valid', [[300, 300, 100, 100], [306, 320, 60, 40], [302, 700, 60, 40]], valid=[1, 0, 1], claims=['aln/invalid_row_masked']),
    _row('aln_one_neighbour_of_several', [[512, 512, 100, 100], [516, 200, 40, 40], [300, 518, 60, 60], [700, 800, 98, 40]], claims=['aln/nn_shared']),
    _row('aln_single_box', [[4 * U, 4 * U, 2 * U, 2 * U]], claims=['aln/n1', 'aln/masked_m1']),
    _row('aln_unit_distance', [[0, 0, 0, 0], [GRID, GRID, 0, 0]], claims=['aln/masked_m1', 'ovl/zero_area_row']),
    # ---- masks
    _row('mask_empty_sample_in_batch', [[A0, [2 * U, 5 * U, U, 3 * U]], [[400, 400, 300, 300], [500, 450, 260, 280]], [[450, 520, 320, 200], [300, 300, 100, 100]]],
         valid=[[1, 1], [0, 0], [1, 0]], claims=['mask/empty_sample']),
    _row('mask_nothing_valid', [[400, 400, 300, 300], [500, 450, 260, 280]], valid=[0, 0], claims=['mask/empty_sample', 'mask/cnt_zero']),
    _row('mask_first_slot_invalid', [[400, 400, 300, 300], [500, 450, 260, 280], [450, 520, 320, 200], [300, 300, 100, 100]], valid=[0, 1, 1, 1],
         claims=['mask/first_slot_invalid']),
]
RULE = {r['name']: r for r in RULE_ROWS}
# rows whose oracle values are not all finite, and why
NONFINITE_RULE_ROWS = {'giou_zero_area_equal': 'gIoU 0 / 0 on both sides; overlap row of the zero-area box (deviation 2)',
                       'ovl_zero_w_inside': 'deviation 2', 'ovl_zero_h_inside': 'deviation 2', 'ovl_zero_both_inside': 'deviation 2',
                       'aln_unit_distance': 'deviation 2 (both boxes have zero area)',
                       'mask_empty_sample_in_batch': 'deviation 1', 'mask_nothing_valid': 'deviation 1'}

RANDOM_SHAPES = [(1, 1), (2, 2), (3, 9), (16, 9), (2, 16), (2, 17), (1, 63), (2, 64), (70, 3)]
RANDOM_TABLES = [(grid, seed, B, N) for grid in ('coarse', 'fine') for seed in (0, 1) for B, N in RANDOM_SHAPES]
MAX_N = 64
EQUAL_SHARE = 0.3         # coarse grid: share of the reference boxes set equal to the generated ones
BIG = (1025, 64)          # one forward + backward through the wrapper, past the backward's block cap


def _random_boxes(g, grid, B, N):
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (B, N), generator=g)
    if grid == 'coarse':
        return torch.stack([ri(1, 7) * U, ri(1, 7) * U, ri(1, 2) * U, ri(1, 2) * U], -1).to(F32) / GRID
    return torch.stack([ri(256, 768), ri(256, 768), 2 * ri(1, 255), 2 * ri(1, 255)], -1).to(F32) / GRID


def random_table(grid, seed, B, N):
    """-> dict(fake, real, valid): non-zero areas, every coordinate in [0, 1], ragged masks with at least one valid box per sample."""
    g = torch.Generator().manual_seed(8100 + 1000 * seed + 31 * B + N + (0 if grid == 'coarse' else 500))
    fake, real = _random_boxes(g, grid, B, N), _random_boxes(g, grid, B, N)
    if grid == 'coarse':
        same = torch.rand(B, N, generator=g) < EQUAL_SHARE
        real = torch.where(same[..., None], fake, real)
    valid = torch.rand(B, N, generator=g) < 0.75
    valid[0] = True
    valid[torch.arange(B), torch.randint(0, N, (B,), generator=g)] = True
    return dict(name=f'{grid}-s{seed}-B{B}-N{N}', fake=fake, real=real, valid=valid)


def upstream(B, seed=0):
    """The per-sample upstream gradient of one term, in [0.5, 1.5]."""
    return torch.rand(B, generator=torch.Generator().manual_seed(8900 + B + seed)) + 0.5


def on_grid(t):
    """The property every layout table has: grid coordinates, and the same edges in float32 as in float64."""
    x = t.double() * GRID
    ok = bool((x == x.round()).all()) and bool((x[..., 2:] % 2 == 0).all()) and bool((x[..., 2:] >= 0).all())
    e32 = torch.stack(L.xywh_to_ltrb(t.to(F32).permute(2, 0, 1)))
    e64 = torch.stack(L.xywh_to_ltrb(t.to(F64).permute(2, 0, 1)))
    return ok and torch.equal(e32.double(), e64)


# ------------------------------------------------------------------------------------------------------------------------ layout reference
def oracle_layout(fake, real, valid, up, dtype=F64, chunk=128, per_box=True):
    """oracle/losses_ref.py in `dtype` through autograd -> (losses [4, B], grads [4, B, N, 4]):  with cnt = max(valid.sum(), 1) over the batch and
    nb the valid boxes of sample b,
        losses[0, b] = ((f[b][v] - r[b][v]) ** 2).sum() / (4 cnt),      losses[1, b] = generalized_iou_loss(f[b][v], r[b][v]) * nb / cnt
    (both 0 for a sample without a valid box: an empty sum), losses[2] = compute_overlap, losses[3] = compute_alignment;
    grads[t] = d (losses[t] * up).sum() / d fake, one backward per term.  Samples are evaluated `chunk` at a time (overlap and alignment are per
    sample, the two scalar terms are per sample given cnt).  per_box: generalized_iou_loss is evaluated box by box under vmap and the boxes of a
    sample added (the CPU file checks this against the literal per-sample call, per_box=False)."""
    B, N, _ = fake.shape
    cnt = max(int(valid.sum()), 1)
    losses, grads = [], []
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        f = fake[s:e].to(dtype).clone().requires_grad_(True)
        r, v, u = real[s:e].to(dtype), valid[s:e], up[s:e].to(dtype)
        nb = v.sum(1)
        d2 = ((f - r) ** 2).sum(-1)
        mse = torch.where(v, d2, torch.zeros_like(d2)).sum(1) / (4 * cnt)
        if per_box:
            pb = torch.func.vmap(lambda a, b: L.generalized_iou_loss(a[None], b[None]))(f[v], r[v])
            giou = torch.zeros(e - s, dtype=dtype).index_add(0, torch.nonzero(v)[:, 0], pb) / cnt
        else:
            giou = torch.stack([L.generalized_iou_loss(f[b][v[b]], r[b][v[b]]) * int(nb[b]) / cnt if int(nb[b]) else f[b].sum() * 0 for b in range(e - s)])
        out = [mse, giou, L.compute_overlap(f, v), L.compute_alignment(f, v)]
        losses.append(torch.stack(out).detach())
        # one backward per term, each through that term's graph alone (a zero cotangent sent into another term's graph would meet its 0 * inf)
        grads.append(torch.stack([torch.autograd.grad((o * u).sum(), f)[0] for o in out]))
    return torch.cat(losses, 1), torch.cat(grads, 1)


def zero_area(fake, valid):
    """[B, N]: valid boxes with w == 0 or h == 0 (deviation 2)."""
    return valid & ((fake[..., 2] == 0) | (fake[..., 3] == 0))


def giou_nan_rows(fake, real, valid):
    """[B, N]: valid zero-area boxes equal to their reference: gIoU is 0 / 0 there, on both sides."""
    return zero_area(fake, valid) & (fake == real).all(-1)


def empty_samples(valid):
    """[B]: samples without a valid box (deviation 1)."""
    return ~valid.any(1)


def reconstructed(fake, real, valid):
    """[B]: samples whose valid boxes all equal their reference boxes and have an area.  There the gIoU gradient is exactly zero by cancellation
    (with half-half ties d ai = d au / ... = 1 / 2 of d a1, so d (ai / au) = d (au / ah) = 0), and what any evaluation returns is the rounding
    residue of terms of size 1 / w and 1 / h."""
    same = ((fake == real).all(-1) & (fake[..., 2] != 0) & (fake[..., 3] != 0)) | ~valid
    return same.all(1) & valid.any(1)


def cancel_scale(fake, valid, up):
    """[B]: the size of the gIoU partial derivatives that cancel in a reconstructed sample: up / cnt * max over its valid boxes of 1 / w, 1 / h."""
    cnt = max(int(valid.sum()), 1)
    inv = torch.where(valid[..., None] & (fake[..., 2:] != 0), 1.0 / fake[..., 2:].double().clamp_min(1e-30), torch.zeros(fake.shape[:2] + (2,), dtype=F64))
    return up.double() / cnt * inv.amax((1, 2))


def layout_errors(got_l, got_g, ref_l, ref_g, fake, real, valid, up, kernel=True):
    """The measure of the module docstring -> (errs {loss_<term> / grad_<term>: worst error}, broken: list of violated exact conditions).
    kernel=True applies the kernel's conventions to `got`: zeros for a sample without a valid box (the oracle's overlap / alignment are not
    compared there), an exactly zero overlap row for a valid zero-area box where the oracle's row is NaN, NaN exactly where the oracle's gIoU is
    NaN, exact zeros where a sample's reference block is all zero.  The kernel's backward is the weighted sum of the four saved gradients, so the
    NaN gIoU row of a box (giou_nan_rows) is NaN in every term's backward (0 * NaN, as a sum of cotangents in autograd would be): required, and the
    row left out of the comparison (the GPU file reads the saved gradients of such a row from the forward entry point).  kernel=False (the float32 oracle): only entries finite on both sides."""
    got_l, got_g, ref_l, ref_g = [x.detach().double().cpu() for x in (got_l, got_g, ref_l, ref_g)]
    B = valid.shape[0]
    empty, za = empty_samples(valid), zero_area(fake, valid)
    recon, cscale = reconstructed(fake, real, valid), cancel_scale(fake, valid, up)
    nanrows = giou_nan_rows(fake, real, valid)
    errs, broken = {}, []
    if kernel and bool(nanrows.any()):
        if not bool(got_g[:, nanrows].isnan().all()):
            broken.append('the row of a box with NaN gIoU is not NaN in every backward')
        got_g = torch.where(nanrows[None, :, :, None], ref_g, got_g)
    for t, term in enumerate(TERMS):
        gl, rl = got_l[t], ref_l[t]
        skip = empty if t >= 2 else torch.zeros(B, dtype=torch.bool)
        if kernel:
            if bool((gl[empty] != 0).any()) or bool((got_g[:, empty] != 0).any()):
                broken.append(f'{term}: a sample without a valid box is not all zero')
            if not torch.equal(torch.isnan(gl[~skip]), torch.isnan(rl[~skip])):
                broken.append(f'{term}: NaN pattern of the loss shares')
        fin = torch.isfinite(rl) & torch.isfinite(gl) & ~skip
        scale = rl[fin].abs().max().item() if bool(fin.any()) else 0.0
        d = (gl[fin] - rl[fin]).abs().max().item() if bool(fin.any()) else 0.0
        if scale == 0.0:
            if kernel and d != 0.0:
                broken.append(f'{term}: loss shares not exactly zero where the reference is')
            errs['loss_' + term] = 0.0
        else:
            errs['loss_' + term] = d / scale
        worst = 0.0
        for b in range(B):
            if bool(skip[b]):
                continue
            g, r = got_g[t, b], ref_g[t, b]
            if t == 1 and bool(recon[b]):
                worst = max(worst, g.abs().max().item() / cscale[b].item())
                continue
            if kernel and t == 2:
                if not torch.equal(torch.isnan(r).all(-1), za[b]) or not torch.equal(torch.isnan(r).any(-1), za[b]):
                    broken.append(f'overlap: sample {b}: the oracle is NaN elsewhere than on the rows of zero-area boxes')
                if bool((g[za[b] & ~nanrows[b]] != 0).any()):
                    broken.append(f'overlap: sample {b}: the row of a zero-area box is not exactly zero')
                g = torch.where(za[b][:, None], r, g)
            if kernel and not torch.equal(torch.isnan(g), torch.isnan(r)):
                broken.append(f'{term}: sample {b}: NaN pattern of the gradient')
            fin = torch.isfinite(r) & torch.isfinite(g)
            if not bool(fin.any()):
                continue
            scale, d = r[fin].abs().max().item(), (g[fin] - r[fin]).abs().max().item()
            if scale == 0.0:
                if kernel and d != 0.0:
                    broken.append(f'{term}: sample {b}: gradient not exactly zero where the reference block is')
            else:
                worst = max(worst, d / scale)
        errs['grad_' + term] = worst
    return errs, broken


# ------------------------------------------------------------------------------------------------------------------------ layout predicate
LAYOUT_PATHS = ['mask/all_valid', 'mask/ragged', 'mask/empty_sample', 'mask/cnt_zero', 'mask/first_slot_invalid',
                'giou/all_eight_ties', 'giou/edge_tie', 'giou/no_tie', 'giou/partial', 'giou/fake_in_real', 'giou/real_in_fake', 'giou/nested_one_shared_edge',
                'giou/touching', 'giou/disjoint', 'giou/nan_zero_area_equal',
                'ovl/pair', 'ovl/pair_edge_tie', 'ovl/identical_pair', 'ovl/touching', 'ovl/disjoint', 'ovl/padded_overlap_skipped', 'ovl/zero_area_row', 'ovl/no_term',
                'aln/nonzero', 'aln/exact_m0', 'aln/masked_m1', 'aln/n1', 'aln/tie_over_j', 'aln/tie_over_c', 'aln/nn_padded', 'aln/nn_shared', 'aln/invalid_row_masked']


def _ltrb(x):
    return x[..., 0] - x[..., 2] / 2, x[..., 1] - x[..., 3] / 2, x[..., 0] + x[..., 2] / 2, x[..., 1] + x[..., 3] / 2


def _meet(a, b):
    """Two (l, t, r, b) boxes -> 'overlap' (the kernel's cond), 'touching' (cond false with an equal edge and no gap) or 'disjoint'."""
    lm, tm, rm, bm = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    if lm < rm and tm < bm:
        return 'overlap'
    return 'touching' if lm <= rm and tm <= bm else 'disjoint'


def layout_paths(fake, real, valid):
    """The branches layout_losses_kernel takes on one batch, restated in float64 (csrc/layout_loss.hip) -> (paths, info) with
    info['contrib'] [4, B] bool: the sample's gradient block of that term can be non-zero (mse: a valid box differs from its reference; gIoU: a
    valid box is not its reference, or has zero area; overlap: a valid pair overlaps; alignment: a valid box has 0 < m < 1),
    info['nn_padded'][b]: the invalid slots of sample b that a valid box names as its nearest neighbour (they receive an alignment gradient),
    info['nn'][b]: {k: (j, c)} the first arg-min of every valid box with 0 < m < 1,
    info['ovl_cancels'] [B] bool: every overlapping valid pair of the sample is a pair of identical boxes that overlap nothing else (the tie
    halves and the quotient term of such a pair cancel: contributions, but a zero gradient)."""
    f, r, v = fake.double().numpy(), real.double().numpy(), valid.numpy().astype(bool)
    B, N, _ = f.shape
    paths = set()
    contrib, ovl_cancels = np.zeros((4, B), dtype=bool), np.zeros(B, dtype=bool)
    nn_padded, nn = [set() for _ in range(B)], [dict() for _ in range(B)]
    if not v.any():
        paths.add('mask/cnt_zero')
    for b in range(B):
        nb = int(v[b].sum())
        if nb == 0:
            paths.add('mask/empty_sample')
            continue
        paths.add('mask/all_valid' if nb == N else 'mask/ragged')
        if not v[b, 0]:
            paths.add('mask/first_slot_invalid')
        A = np.stack(_ltrb(f[b]), -1)           # [N, 4] l, t, r, b
        R = np.stack(_ltrb(r[b]), -1)
        X = np.stack([A[:, 0], f[b, :, 0], A[:, 2], A[:, 1], f[b, :, 1], A[:, 3]])       # [6, N]
        any_pair, only_identical = False, True
        for k in range(N):
            D = np.abs(X[:, k:k + 1] - X)
            D[:, k] = 1.0
            mc, jc = D.min(1), D.argmin(1)         # numpy's argmin is the first one, as the kernel's `v < m`
            best, bc = mc.min(), int(mc.argmin())
            if not v[b, k]:
                if best < 1.0:
                    paths.add('aln/invalid_row_masked')
                continue
            # ---- mse / gIoU
            same = A[k] == R[k]
            if (f[b, k] != r[b, k]).any():
                contrib[0, b] = True
            a1, a2 = (A[k, 2] - A[k, 0]) * (A[k, 3] - A[k, 1]), (R[k, 2] - R[k, 0]) * (R[k, 3] - R[k, 1])
            paths.add('giou/all_eight_ties' if same.all() else ('giou/edge_tie' if same.any() else 'giou/no_tie'))
            if same.all() and a1 == 0:
                paths.add('giou/nan_zero_area_equal')
                contrib[1, b] = True
            else:
                if not same.all():
                    contrib[1, b] = True
                meet = _meet(A[k], R[k])
                if meet == 'overlap':
                    inner = A[k, 0] >= R[k, 0] and A[k, 1] >= R[k, 1] and A[k, 2] <= R[k, 2] and A[k, 3] <= R[k, 3]
                    outer = A[k, 0] <= R[k, 0] and A[k, 1] <= R[k, 1] and A[k, 2] >= R[k, 2] and A[k, 3] >= R[k, 3]
                    if not same.all():
                        paths.add('giou/fake_in_real' if inner else ('giou/real_in_fake' if outer else 'giou/partial'))
                        if (inner or outer) and int(same.sum()) == 1:
                            paths.add('giou/nested_one_shared_edge')
                else:
                    paths.add('giou/' + meet)
            # ---- overlap
            if a1 == 0:
                paths.add('ovl/zero_area_row')
            for j in range(N):
                if j == k:
                    continue
                meet = _meet(A[k], A[j])
                if not v[b, j]:
                    if meet == 'overlap':
                        paths.add('ovl/padded_overlap_skipped')
                    continue
                if meet == 'overlap':
                    any_pair = True
                    eq = A[k] == A[j]
                    paths.add('ovl/identical_pair' if eq.all() else ('ovl/pair_edge_tie' if eq.any() else 'ovl/pair'))
                    only_identical = only_identical and bool(eq.all())
                else:
                    paths.add('ovl/' + meet)
            # ---- alignment
            if best == 1.0:
                paths.add('aln/masked_m1')
                if N == 1:
                    paths.add('aln/n1')
            elif best == 0.0:
                paths.add('aln/exact_m0')
            else:
                paths.add('aln/nonzero')
                contrib[3, b] = True
                j = int(jc[bc])
                nn[b][k] = (j, bc)
                if int((D[bc] == best).sum()) > 1:
                    paths.add('aln/tie_over_j')
                if int((mc == best).sum()) > 1:
                    paths.add('aln/tie_over_c')
                if not v[b, j]:
                    paths.add('aln/nn_padded')
                    nn_padded[b].add(j)
        targets = [j for j, _ in nn[b].values()]
        if len(targets) != len(set(targets)):
            paths.add('aln/nn_shared')
        contrib[2, b] = any_pair
        ovl_cancels[b] = any_pair and only_identical
        if not any_pair:
            paths.add('ovl/no_term')
    return paths, dict(contrib=contrib, nn_padded=nn_padded, nn=nn, ovl_cancels=ovl_cancels)


# ------------------------------------------------------------------------------------------------------------------------ layout backward
BWD_THREADS, BWD_MAX_BLOCKS = 256, 1024          # csrc/layout_loss.hip: layout_losses_bwd_kernel, ldetr_layout_losses_bwd_f32
BWD_CASES = [(3, 9), (1024, 64), (1025, 64), (2100, 64)]
BWD_PATHS = ['bwd/under_cap', 'bwd/exact_cap', 'bwd/one_block_second_trip', 'bwd/every_block_second_trip']


def bwd_path(B, N):
    blocks = (B * N * 4 + BWD_THREADS - 1) // BWD_THREADS
    if blocks < BWD_MAX_BLOCKS:
        return {'bwd/under_cap'}
    if blocks == BWD_MAX_BLOCKS:
        return {'bwd/exact_cap'}
    return {'bwd/one_block_second_trip' if blocks == BWD_MAX_BLOCKS + 1 else 'bwd/every_block_second_trip'}


def bwd_inputs(B, N):
    g = torch.Generator().manual_seed(8300 + B + N)
    return torch.randn(4, B, N, 4, generator=g), torch.randn(4, B, generator=g)


def bwd_ref(grads, g):
    """dbox[b, n, c] = sum_t g[t, b] grads[t, b, n, c]."""
    return torch.einsum('tb,tbnc->bnc', g.double(), grads.double())


# ------------------------------------------------------------------------------------------------------------------------ combine
IDENT, SOFTPLUS, SOFTPLUS_NEG, RATIO = 0, 1, 2, 3          # hip/losses.py
COMBINE_THREADS, COMBINE_MAX_K = 256, 16
COMBINE_NS = [1, 2, 255, 256, 257, 1000]
COMBINE_GAINS = [1.0, 0.5]
SOFTPLUS_EDGES = [-100.0, -20.5, -20.0, 0.0, 20.0, float(np.nextafter(np.float32(20.0), np.float32(np.inf))), 20.5, 100.0]
# name -> list of (fn, n, sum_reduce, kind of input)
COMBINE_CASES = {}
for _fn, _fname in ((IDENT, 'ident'), (SOFTPLUS, 'softplus'), (SOFTPLUS_NEG, 'softplus_neg')):
    for _red in (False, True):
        for _n in COMBINE_NS:
            COMBINE_CASES[f'{_fname}-{"sum" if _red else "mean"}-n{_n}'] = [(_fn, _n, _red, 'randn')]
COMBINE_CASES['ratio'] = [(RATIO, 2, False, 'ratio')]
COMBINE_CASES['softplus-edges'] = [(SOFTPLUS, len(SOFTPLUS_EDGES), False, 'edges'), (SOFTPLUS_NEG, len(SOFTPLUS_EDGES), True, 'edges')]
COMBINE_CASES['K16-one-function'] = [(IDENT, 5, False, 'randn')] * 16
COMBINE_CASES['K16-mixed-ratio-first-middle-last'] = [(RATIO, 2, False, 'ratio'), (SOFTPLUS, 257, False, 'randn'), (IDENT, 1, False, 'randn'), (SOFTPLUS_NEG, 256, True, 'randn'),
                                                      (IDENT, 300, True, 'randn'), (SOFTPLUS, 2, True, 'randn'), (IDENT, 255, False, 'randn'), (RATIO, 2, False, 'ratio'),
                                                      (SOFTPLUS_NEG, 1000, False, 'randn'), (SOFTPLUS, 64, False, 'randn'), (IDENT, 2, True, 'randn'), (SOFTPLUS_NEG, 3, False, 'randn'),
                                                      (IDENT, 513, False, 'randn'), (SOFTPLUS, 1, True, 'randn'), (SOFTPLUS_NEG, 100, True, 'randn'), (RATIO, 2, False, 'ratio')]
COMBINE_PATHS = ['K1', 'K16', 'K_between', 'ratio', 'ratio_first', 'ratio_last', 'ratio_between', 'ident', 'softplus', 'softplus_neg', 'sum_reduce', 'batch_mean',
                 'one_trip_idle_threads', 'one_trip_full', 'second_trip', 'fourth_trip', 'softplus_above_threshold', 'softplus_at_threshold', 'softplus_below_threshold']


def combine_path(rows, xs=None):
    """loss_combine_fwd / bwd_kernel: one block of 256 threads walks the K rows; a RATIO row leaves the loop body early (`continue` before the block
    reduction); the other rows take ceil(n / 256) trips; softplus takes its linear branch above 20."""
    K = len(rows)
    out = {'K1' if K == 1 else ('K16' if K == COMBINE_MAX_K else 'K_between')}
    for k, (fn, n, red, _) in enumerate(rows):
        if fn == RATIO:
            out.add('ratio')
            if K > 1:
                out.add('ratio_first' if k == 0 else ('ratio_last' if k == K - 1 else 'ratio_between'))
            continue
        out.add({IDENT: 'ident', SOFTPLUS: 'softplus', SOFTPLUS_NEG: 'softplus_neg'}[fn])
        out.add('sum_reduce' if red else 'batch_mean')
        trips = (n + COMBINE_THREADS - 1) // COMBINE_THREADS
        out.add('one_trip_full' if n == COMBINE_THREADS else ('one_trip_idle_threads' if trips == 1 else ('second_trip' if trips == 2 else 'fourth_trip')))
        if xs is not None and fn != IDENT:
            a = xs[k].double() * (1.0 if fn == SOFTPLUS else -1.0)
            if bool((a > 20).any()):
                out.add('softplus_above_threshold')
            if bool((a == 20).any()):
                out.add('softplus_at_threshold')
            if bool((a < 20).any()):
                out.add('softplus_below_threshold')
    return out


def combine_inputs(rows, seed=0):
    """float32 inputs and weights of one case.  'randn': 3 * randn, every fourth element x 10 (beyond softplus' threshold on either side), an
    IDENT row offset by + 2 (the project's bound is relative to the result: a sum that cancels to nothing has no scale); 'ratio': the (sum, count)
    pair of a cross entropy; 'edges': SOFTPLUS_EDGES."""
    g = torch.Generator().manual_seed(8500 + len(rows) + 7 * seed + sum(n for _, n, _, _ in rows))
    xs, ws = [], []
    for k, (fn, n, red, kind) in enumerate(rows):
        if kind == 'ratio':
            xs.append(torch.tensor([7.5 + k, 3.0 + (k % 5)]))
        elif kind == 'edges':
            xs.append(torch.tensor(SOFTPLUS_EDGES, dtype=F32))
        else:
            x = torch.randn(n, generator=g) * 3.0
            x[3::4] *= 10.0
            xs.append(x.abs() + 2.0 if fn == IDENT else x)
        ws.append(float(torch.rand((), generator=g)) * 4 + 0.5)
    return xs, ws


def combine_ref(rows, xs, ws, gain, softplus_threshold=20.0):
    """training/loss.py's op chain in float64 autograd: value_k = w_k f_k(x_k) (a RATIO row: w x[0] / x[1]); a sum_reduce row enters the total as
    its sum, a per-sample row as its mean (`sum(terms).mean()` with scalars broadcast); total = gain * sum.  Reported: the sum of a sum_reduce /
    RATIO / single-element row, the weighted vector otherwise.  The RATIO gradient is reported as the kernel leaves it: d total / d (x0 / x1) on
    x0 (the cross-entropy backward divides by its count itself), 0 on x1.  -> (total, reports, grads)"""
    leaves = [x.double().clone().requires_grad_(True) for x in xs]
    total, rep, ratios = 0.0, [], []
    for (fn, n, red, _), x, w in zip(rows, leaves, ws):
        w = float(torch.tensor(w, dtype=F32))
        if fn == RATIO:
            q = x[0] / x[1]
            q.retain_grad()
            ratios.append(q)
            v = q * w
            total = total + v
            rep.append(v.detach())
            continue
        fx = x if fn == IDENT else F.softplus(x if fn == SOFTPLUS else -x, threshold=softplus_threshold)
        v = fx * w
        total = total + (v.sum() if red else v.mean())
        rep.append(v.sum().detach() if (red or n == 1) else v.detach())
    total = total * gain
    total.backward()
    grads, qi = [], 0
    for (fn, _, _, _), x in zip(rows, leaves):
        if fn == RATIO:
            grads.append(torch.stack([ratios[qi].grad, torch.zeros((), dtype=F64)]))
            qi += 1
        else:
            grads.append(x.grad)
    return total.detach(), rep, grads


# ------------------------------------------------------------------------------------------------------------------------ masked mse
MSE_THREADS, MSE_BWD_MAX_BLOCKS = 256, 256          # csrc/layout_loss.hip: masked_mse_*_kernel, ldetr_masked_mse_bwd_f32
MSE_CAP = MSE_THREADS * MSE_BWD_MAX_BLOCKS          # 65536 elements per sweep of the backward
# (rows, D, N): rows x D walks the trip boundary of the forward's single block and the backward's block cap; bdiv is 1 or N (N divides rows)
MSE_SHAPES = [(1, 1, 1), (255, 1, 5), (64, 4, 8), (256, 1, 16), (257, 1, 257), (18, 36, 9), (16384, 4, 64), (65537, 1, 65537), (1821, 36, 3), (196613, 1, 196613)]
MSE_MASKS = ['all', 'none', 'ragged']
MSE_UP = 3.0          # the upstream gradient
MSE_PATHS = ['D1', 'D>1', 'bdiv1', 'bdivN', 'fwd/one_trip_idle_threads', 'fwd/one_trip_full', 'fwd/many_trips',
             'bwd/under_cap', 'bwd/exact_cap', 'bwd/second_sweep_one_thread', 'bwd/second_sweep', 'bwd/fourth_sweep', 'count_zero', 'count_all', 'count_some']


def mse_path(rows, D, bdiv, mask):
    n = rows * D
    out = {'D1' if D == 1 else 'D>1', 'bdiv1' if bdiv == 1 else 'bdivN'}
    out.add('fwd/one_trip_full' if n == MSE_THREADS else ('fwd/one_trip_idle_threads' if n < MSE_THREADS else 'fwd/many_trips'))
    if n < MSE_CAP:
        out.add('bwd/under_cap')
    elif n == MSE_CAP:
        out.add('bwd/exact_cap')
    elif n == MSE_CAP + 1:
        out.add('bwd/second_sweep_one_thread')
    else:
        out.add('bwd/second_sweep' if n <= 2 * MSE_CAP else 'bwd/fourth_sweep')
    out.add({'all': 'count_all', 'none': 'count_zero', 'ragged': 'count_some'}[mask])
    return out


def mse_inputs(rows, D, bdiv, mask):
    g = torch.Generator().manual_seed(8700 + rows % 1000 + D + bdiv % 100)
    a, b = torch.randn(rows, D, generator=g), torch.randn(rows // bdiv, D, generator=g)
    valid = dict(all=torch.ones(rows, dtype=torch.bool), none=torch.zeros(rows, dtype=torch.bool), ragged=torch.rand(rows, generator=g) > 0.3)[mask]
    if mask == 'ragged' and rows > 1:
        valid[0], valid[-1] = False, True
    return a, b, valid


def mse_ref(a, b, valid, bdiv, up=1.0):
    """F.mse_loss(a[valid], b[valid]) with one reference row per bdiv rows, in float64 autograd; no valid row: 0 and a zero gradient (the kernel's
    0 / max(count, 1)).  -> (loss, count, d (up * loss) / d a)"""
    x = a.double().clone().requires_grad_(True)
    full = b.double().repeat_interleave(bdiv, 0)
    if not bool(valid.any()):
        return torch.zeros((), dtype=F64), 0, torch.zeros_like(x)
    loss = F.mse_loss(x[valid], full[valid])
    (loss * up).backward()
    return loss.detach(), int(valid.sum()), x.grad


# ------------------------------------------------------------------------------------------------------------------------ LSAP
LSAP_WAVE = 64          # csrc/lsap.hip: one problem per lane, 64 lanes per block
LSAP_NS = [9, 17]          # the two instantiations (n <= 16, n <= 64)
LSAP_BATCHES = [1, 65, 130]          # a single lane; a full wave and one lane; two full waves and two lanes


def lsap_costs(batch, n, seed=0):
    """float64 costs as test_lsap_matches_scipy_bit_exact draws them: every third problem heavy with ties, problem 1 constant."""
    rng = np.random.RandomState(9100 + batch + n + seed)
    cost = rng.rand(batch, n, n)
    cost[::3] = np.round(cost[::3] * 3) / 3
    if batch > 1:
        cost[1] = 0.5
    return cost


def lsap_inf_costs(n, seed=0):
    """[3, n, n]: feasible with +inf entries (the diagonal and one more entry per row stay finite), infeasible (row 2 all +inf), feasible."""
    rng = np.random.RandomState(9200 + n + seed)
    cost = rng.rand(3, n, n)
    blocked = rng.rand(n, n) < 0.5
    blocked[np.arange(n), np.arange(n)] = False
    blocked[np.arange(n), (np.arange(n) + 3) % n] = False
    cost[0][blocked] = np.inf
    cost[1][min(2, n - 1), :] = np.inf
    return cost


# ------------------------------------------------------------------------------------------------------------------------ float32 yardstick
def all_layout_tables():
    return RULE_ROWS + [random_table(*c) for c in RANDOM_TABLES]


def measure_fp32_baselines():
    """The oracle in float32 on the CPU against the oracle in float64 over every layout table, in layout_errors' measure -> dict like
    FP32_BASELINE."""
    out = dict.fromkeys(FP32_BASELINE, 0.0)
    for t in all_layout_tables():
        up = upstream(t['fake'].shape[0])
        l64, g64 = oracle_layout(t['fake'], t['real'], t['valid'], up, F64)
        l32, g32 = oracle_layout(t['fake'], t['real'], t['valid'], up, F32)
        errs, _ = layout_errors(l32, g32, l64, g64, t['fake'], t['real'], t['valid'], up, kernel=False)
        for k, e in errs.items():
            out[k] = max(out[k], e)
    return out
