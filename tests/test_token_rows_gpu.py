"""Every host-side path of the token-row kernels against float64: the grouped LayerNorm forward / backward with its in-launch partial-sum reduction,
ldetr_sum_parts_f32 (csrc/layernorm.hip), the label-smoothed softmax cross entropy and the token embedding gather / scatter (csrc/xent.hip).
References, case tables and the path predicates are in tests/token_rows_common.py; tests/test_token_rows_ref_cpu.py proves that the tables reach every
path and that the references are torch's own float64 results.

LayerNorm is driven through hip.blocks.ln_fwd / ln_bwd / launch, the other families through core.lib() as hip/stacks.py, training/med.py and
training/networks_detr.py call them.  Dropout seeds are pinned per case (as test_dropout_parity_gpu.fresh_device_word does) and the masks rebuilt on
the host by oracle/dropout_ref.py.

Exact checks: pure additions (the pre-norm sum without dropout, y + pos, sum_parts, the embedding gather) are bit-equal to the float32 CPU sum in
the documented order; ignored / out-of-range / padding rows get exact zeros; the valid-row count is exact; a zero-row problem and a NULL output
leave everything else as it was.  Bounded checks keep the project's bounds (LayerNorm y 3e-6, gradients 1e-5; cross-entropy loss 2e-6 relative +
1e-6, dlogits 2e-5; embedding scatter 2e-5); what has no project bound is held to 4 x the float32 CPU error (token_rows_common.FP32_BASELINE).
Every case prints its figures before it asserts.

Largest measured errors (MI355X; bound): LayerNorm y 2.3e-7, z with dropout 2.4e-7 (3e-6), dx 2.9e-7, dr 2.7e-7, dgamma / dbeta 2.1e-7 (1e-5); mean
2.4e-6 (5.3e-6), rstd 1.4e-7 (6.2e-7); 2053 rows dgamma 1.0e-6 (7.0e-6), dbeta 6.7e-7 (4.6e-6); +100 rows y 2.0e-6 (1.1e-5), gradients 4.4e-6
(1.1e-5).  Cross entropy: mean loss 5.0e-6 absolute (2e-6 |loss| + 1e-6 = 2.0e-5 there), row_lse 5.1e-8 (2e-6), dlogits 6.2e-7 (2e-5); loss sum
over 2053 rows 5.2e-7 (3.3e-6); logits x 30 loss 4.8e-8 (3.2e-7), dlogits 7.0e-6 (2.8e-5).  Embedding scatter 2.0e-6 (2e-5)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import token_rows_common as R

pytestmark = pytest.mark.gpu

R.limit_threads()
CANARY = -1234.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'xent_guard.npz')


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(dev):
    """A device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def _hip():
    from layoutdetr_amd.hip import blocks, core
    return core, blocks


def pin_seeds(core, dev, case):
    """Both halves of the dropout seeds pinned to the case (test_dropout_parity_gpu.fresh_device_word) -> the device word."""
    torch.manual_seed(0x70C + case)
    core._seed_counter[0] = 0x5EED + 64 * case
    core.reseed(dev)
    word = core.iter_seed().item()
    assert word != 0
    return word


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
            print(f'[token rows] {self.case}: {name} err {e:.3e} (bound {tol:.2e})')
        for name, ok in self.flags:
            print(f'[token rows] {self.case}: {name} {"exact" if ok else "NOT exact"}')
        bad = [f'{name}: {e:.3e} > {tol:.2e}' for name, e, tol in self.rows if not e <= tol] + [f'{name}: not exact' for name, ok in self.flags if not ok]
        assert not bad, f'{self.case}: ' + '; '.join(bad)


def canary(dev, *shape):
    return torch.full(shape, CANARY, device=dev, dtype=torch.float32)


def untouched(t):
    return bool((t == CANARY).all())


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm drivers
def ln_fwd_problem(dev, t, r_parts=0, bias=False, p=0.0, seed=0, pos=None, null=(), zero_rows=False, plain=False):
    """-> (argument block, dict of the device tensors it points to).  Outputs are pre-filled with CANARY.  null: outputs passed as NULL.
    zero_rows: the block describes 0 rows of the (non-empty) buffers.  plain: r = NULL."""
    core, blocks = _hip()
    rows, D = t['x'].shape
    d = dict(x=t['x'].to(dev), r=None if plain else t['r'][:max(r_parts, 1)].contiguous().to(dev), gamma=t['gamma'].to(dev), beta=t['beta'].to(dev),
             r_bias=t['r_bias'].to(dev) if bias else None, pos=pos.to(dev) if pos is not None else None,
             y=canary(dev, rows, D), z=canary(dev, rows, D), mean=canary(dev, rows), rstd=canary(dev, rows), ypos=canary(dev, rows, D) if pos is not None else None)
    a = blocks.ln_fwd(d['x'], d['r'], d['gamma'], d['beta'], R.LN_EPS, p, seed, d['y'], d['z'], d['mean'], d['rstd'], r_parts=r_parts, r_bias=d['r_bias'],
                      pos=d['pos'], ypos=d['ypos'])
    for k in null:
        setattr(a, k, None)
    if zero_rows:
        a.rows = 0
    return a, d


def ln_bwd_problem(dev, t, z, mean, rstd, n_parts=0, use_dy2=False, p=0.0, seed=0, null=(), running=False, zero_rows=False, want_dr=True):
    """z / mean / rstd: device tensors (the forward's own) or float32 CPU tensors."""
    core, blocks = _hip()
    rows, D = t['dy'].shape
    d = dict(dy=t['dy'].to(dev), dy2=t['dy2'].to(dev) if use_dy2 else None, parts=t['parts'][:n_parts].contiguous().to(dev) if n_parts else None,
             z=z.to(dev), mean=mean.to(dev), rstd=rstd.to(dev), gamma=t['gamma'].to(dev), dx=canary(dev, rows, D), dr=canary(dev, rows, D) if want_dr else None,
             dgamma=t['dg0'].to(dev) if running else torch.zeros(D, device=dev), dbeta=t['db0'].to(dev) if running else torch.zeros(D, device=dev))
    if zero_rows:
        d['dgamma'], d['dbeta'] = canary(dev, D), canary(dev, D)
    a = blocks.ln_bwd(d['dy'], d['z'], d['mean'], d['rstd'], d['gamma'], d['dx'], d['dr'], d['dgamma'], d['dbeta'], p, seed, dy2=d['dy2'], parts=d['parts'],
                      n_parts=n_parts)
    for k in null:
        setattr(a, k, None)
    if zero_rows:
        a.rows = 0
    return a, d


def launch(what, args):
    core, blocks = _hip()
    blocks.launch(what, args)
    torch.cuda.synchronize()


def check_ln_fwd(f, tag, d, t, r_parts, bias, p, drop, pos=None, null=(), stats_bounded=True, plain=False):
    """One forward problem's outputs against the float64 reference (and the exact checks of the module docstring)."""
    kw = dict(r_parts=r_parts, r_bias=t['r_bias'] if bias else None, drop=drop, pos=pos)
    r = None if plain else t['r']
    ref = R.ln_fwd_ref(t['x'], r, t['gamma'], t['beta'], **kw)
    f.add(tag + 'y', d['y'], ref['y'], R.TOL_LN['y'])
    if 'z' not in null:
        if p > 0:
            f.add(tag + 'z', d['z'], ref['z'], R.TOL_LN['y'])
        else:
            f.exact(tag + 'z == float32 sum in slice order', torch.equal(d['z'].cpu(), R.ln_fwd_ref(t['x'], r, t['gamma'], t['beta'], dtype=R.F32, **kw)['z']))
    for k in ('mean', 'rstd'):
        if k not in null and stats_bounded:
            f.add(tag + k, d[k], ref[k], R.fp32_bound('ln_' + k))
    if pos is not None:
        rows = t['x'].shape[0]
        f.add(tag + 'y + pos', d['ypos'], ref['ypos'], R.TOL_LN['y'])
        f.exact(tag + 'ypos == y + pos[row % pos_rows]', torch.equal(d['ypos'].cpu(), d['y'].cpu() + pos[torch.arange(rows) % pos.shape[0]]))
    return ref


def check_ln_bwd(f, tag, d, t, z64, n_parts, use_dy2, drop, null=(), running=False, big=False):
    ref = R.ln_bwd_ref(z64, t['gamma'], t['dy'], t['dy2'] if use_dy2 else None, t['parts'], n_parts, drop, t['dg0'] if running else None, t['db0'] if running else None)
    if 'dx' not in null:
        f.add(tag + 'dx', d['dx'], ref['dx'], R.TOL_LN['grad'])
    if 'dr' not in null and d['dr'] is not None:
        f.add(tag + 'dr', d['dr'], ref['dr'], R.TOL_LN['grad'])
        if drop is not None:
            f.exact(tag + 'dr == 0 where dropped', not bool(d['dr'].cpu()[drop == 0].any()))
    if 'dgamma' not in null:
        f.add(tag + 'dgamma', d['dgamma'], ref['dgamma'], R.fp32_bound('ln_big_dgamma') if big else R.TOL_LN['grad'])
        f.add(tag + 'dbeta', d['dbeta'], ref['dbeta'], R.fp32_bound('ln_big_dbeta') if big else R.TOL_LN['grad'])
    return ref


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm: D and rows
def _shape_id(c):
    return f'rows{c[0]}-D{c[1]}-' + '.'.join(sorted(R.ln_shape_path(*c)))


@pytest.mark.parametrize('case', R.LN_SHAPE_CASES, ids=_shape_id)
def test_layernorm_every_instantiation_and_grid(dev, case):
    """LayerNorm(x + dropout(r)) with p = 0.1 and its backward at every NV, with idle lanes in the last vector, D = 4 and 1024, ragged last
    blocks and (2053 rows) a second sweep of the backward's capped grid; plus the same rows without dropout (z bit-equal) and without a residual."""
    core, blocks = _hip()
    rows, D = case
    t = R.ln_inputs(rows, D)
    word = pin_seeds(core, dev, 100 + R.LN_SHAPE_CASES.index(case))
    seed = core.next_seed()
    drop = R.drop_rows(seed, word, R.LN_SHAPE_P, rows, D)
    big = rows > R.LN_MAX_BWD_BLOCKS * R.LN_ROWS_PER_BLOCK
    f = Figures(f'layernorm {case}')
    a, d = ln_fwd_problem(dev, t, p=R.LN_SHAPE_P, seed=seed)
    launch('layernorm_fwd', [a])
    ref = check_ln_fwd(f, '', d, t, 0, False, R.LN_SHAPE_P, drop)
    b, e = ln_bwd_problem(dev, t, d['z'], d['mean'], d['rstd'], p=R.LN_SHAPE_P, seed=seed)
    launch('layernorm_bwd', [b])
    check_ln_bwd(f, '', e, t, ref['z'], 0, False, drop, big=big)
    a, d = ln_fwd_problem(dev, t)
    launch('layernorm_fwd', [a])
    check_ln_fwd(f, 'p = 0: ', d, t, 0, False, 0.0, None)
    a, d = ln_fwd_problem(dev, t, plain=True)
    launch('layernorm_fwd', [a])
    check_ln_fwd(f, 'no residual: ', d, t, 0, False, 0.0, None, plain=True)
    f.exact('no residual: z == x', torch.equal(d['z'].cpu(), t['x']))
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm: slices
def _slice_id(direction):
    return lambda c: f'D{c[0]}-slices{c[1]}-' + '.'.join(sorted(R.ln_slices_path(c[0], c[1], direction))).replace('/', '.')


@pytest.mark.parametrize('case', R.LN_FWD_SLICE_CASES, ids=_slice_id('fwd'))
def test_layernorm_forward_slice_reduction(dev, case):
    """r = (r[0] + r_bias) + r[1] + ... formed inside the launch, every round shape of the slice loop, with and without r_bias and dropout.
    Without dropout z is bit-equal to the float32 sum in that order."""
    core, blocks = _hip()
    D, slices = case
    rows = R.LN_SLICE_ROWS
    t = R.ln_inputs(rows, D, fwd_slices=slices)
    f = Figures(f'layernorm forward {slices} slices at D {D}')
    for bias in (False, True):
        for p in (0.0, R.LN_SLICE_P):
            word = pin_seeds(core, dev, 200 + slices)
            seed = core.next_seed()
            a, d = ln_fwd_problem(dev, t, r_parts=slices, bias=bias, p=p, seed=seed)
            launch('layernorm_fwd', [a])
            check_ln_fwd(f, f'bias {int(bias)} p {p}: ', d, t, slices, bias, p, R.drop_rows(seed, word, p, rows, D), stats_bounded=False)
    f.check()


@pytest.mark.parametrize('case', R.LN_BWD_SLICE_CASES, ids=_slice_id('bwd'))
def test_layernorm_backward_slice_reduction(dev, case):
    """Incoming gradient dy (+ dy2) + sum of the slices, every round shape, with and without dy2 and dropout.  z, mean and rstd are handed in as the
    float32 roundings of the float64 reference's, so the backward is tested on its own."""
    core, blocks = _hip()
    D, slices = case
    rows = R.LN_SLICE_ROWS
    t = R.ln_inputs(rows, D, bwd_slices=slices)
    fw = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'])
    z32 = fw['z'].float()
    f = Figures(f'layernorm backward {slices} slices at D {D}')
    for use_dy2 in (False, True):
        for p in (0.0, R.LN_SLICE_P):
            word = pin_seeds(core, dev, 300 + slices)
            seed = core.next_seed()
            b, e = ln_bwd_problem(dev, t, z32, fw['mean'].float(), fw['rstd'].float(), n_parts=slices, use_dy2=use_dy2, p=p, seed=seed)
            launch('layernorm_bwd', [b])
            check_ln_bwd(f, f'dy2 {int(use_dy2)} p {p}: ', e, t, z32, slices, use_dy2, R.drop_rows(seed, word, p, rows, D))
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm: groups
@pytest.mark.parametrize('case', R.LN_GROUP_CASES, ids=lambda c: f'rows{c[0]}+{c[1]}-' + '.'.join(sorted(R.ln_group_path(*c))))
def test_layernorm_group_of_two_vs_fp64(dev, case):
    """Two problems with different row counts, slice counts and dropout probabilities as one launch, each against its own reference; a problem
    with zero rows leaves its (canary-filled) outputs untouched and does not disturb the other."""
    core, blocks = _hip()
    D = R.LN_GROUP_D
    word = pin_seeds(core, dev, 400 + R.LN_GROUP_CASES.index(case))
    f = Figures(f'layernorm group {case}')
    fwd, bwd, meta = [], [], []
    for i, (rows, m) in enumerate(zip(case, R.LN_GROUP_MEMBERS)):
        empty = rows == 0
        t = R.ln_inputs(4 if empty else rows, D, fwd_slices=m['fwd_slices'], bwd_slices=m['bwd_slices'], seed=i + 1)
        seed = core.next_seed()
        fwd.append(ln_fwd_problem(dev, t, r_parts=m['fwd_slices'], bias=True, p=m['p'], seed=seed, zero_rows=empty))
        meta.append((t, seed, empty, m))
    launch('layernorm_fwd', [a for a, _ in fwd])
    refs = []
    for i, ((a, d), (t, seed, empty, m)) in enumerate(zip(fwd, meta)):
        if empty:
            f.exact(f'problem {i} (0 rows): forward outputs untouched', all(untouched(d[k]) for k in ('y', 'z', 'mean', 'rstd')))
            refs.append(None)
            fw = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'])
            z, mean, rstd = fw['z'].float(), fw['mean'].float(), fw['rstd'].float()
        else:
            drop = R.drop_rows(seed, word, m['p'], t['x'].shape[0], D)
            refs.append((check_ln_fwd(f, f'problem {i}: ', d, t, m['fwd_slices'], True, m['p'], drop, stats_bounded=False), drop))
            z, mean, rstd = d['z'], d['mean'], d['rstd']
        bwd.append(ln_bwd_problem(dev, t, z, mean, rstd, n_parts=m['bwd_slices'], use_dy2=True, p=m['p'], seed=seed, zero_rows=empty))
    launch('layernorm_bwd', [b for b, _ in bwd])
    for i, ((b, e), (t, seed, empty, m)) in enumerate(zip(bwd, meta)):
        if empty:
            f.exact(f'problem {i} (0 rows): backward outputs untouched', all(untouched(e[k]) for k in ('dx', 'dr', 'dgamma', 'dbeta')))
        else:
            ref, drop = refs[i]
            check_ln_bwd(f, f'problem {i}: ', e, t, ref['z'], m['bwd_slices'], True, drop, big=t['x'].shape[0] > R.LN_MAX_BWD_BLOCKS * R.LN_ROWS_PER_BLOCK)
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm: optional pointers
@pytest.mark.parametrize('pos_rows', R.LN_POS_ROWS)
def test_layernorm_second_output_pos_rows(dev, pos_rows):
    """ypos = y + pos[row % pos_rows] where pos_rows divides the row count, does not divide it, and is 1."""
    rows, D = R.LN_OPT_ROWS, R.LN_OPT_D
    t = R.ln_inputs(rows, D, pos_rows=pos_rows)
    a, d = ln_fwd_problem(dev, t, pos=t['pos'])
    launch('layernorm_fwd', [a])
    f = Figures(f'layernorm pos_rows {pos_rows}')
    check_ln_fwd(f, '', d, t, 0, False, 0.0, None, pos=t['pos'])
    f.check()


def _opt_full(dev, t, seed, p):
    a, d = ln_fwd_problem(dev, t, r_parts=2, bias=True, p=p, seed=seed)
    launch('layernorm_fwd', [a])
    b, e = ln_bwd_problem(dev, t, d['z'], d['mean'], d['rstd'], n_parts=2, use_dy2=True, p=p, seed=seed)
    launch('layernorm_bwd', [b])
    return d, e


@pytest.mark.parametrize('which', R.LN_OPTIONAL_NULL)
def test_layernorm_null_outputs_leave_the_others_unchanged(dev, which):
    """Each optional output NULL once: the remaining outputs equal the full case's bit for bit (dgamma / dbeta, summed by atomics in no fixed
    order, within the gradient bound of the reference)."""
    core, blocks = _hip()
    rows, D, p = R.LN_OPT_ROWS, R.LN_OPT_D, 0.2
    t = R.ln_inputs(rows, D, fwd_slices=2, bwd_slices=2)
    word = pin_seeds(core, dev, 500)
    seed = core.next_seed()
    drop = R.drop_rows(seed, word, p, rows, D)
    full_f, full_b = _opt_full(dev, t, seed, p)
    f = Figures(f'layernorm NULL {which}')
    if which in ('z', 'mean', 'rstd'):
        a, d = ln_fwd_problem(dev, t, r_parts=2, bias=True, p=p, seed=seed, null=(which,))
        launch('layernorm_fwd', [a])
        f.exact(f'{which} buffer untouched', untouched(d[which]))
        for k in ('y', 'z', 'mean', 'rstd'):
            if k != which:
                f.exact(f'{k} == full case', torch.equal(d[k], full_f[k]))
        check_ln_fwd(f, '', d, t, 2, True, p, drop, null=(which,), stats_bounded=False)
    else:
        null = ('dx',) if which == 'dx' else ('dgamma', 'dbeta')
        b, e = ln_bwd_problem(dev, t, full_f['z'], full_f['mean'], full_f['rstd'], n_parts=2, use_dy2=True, p=p, seed=seed, null=null)
        launch('layernorm_bwd', [b])
        for k in null:
            f.exact(f'{k} buffer untouched', untouched(e[k]) if k == 'dx' else not bool(e[k].any()))
        for k in ('dx', 'dr'):
            if k not in null:
                f.exact(f'{k} == full case', torch.equal(e[k], full_b[k]))
        z64 = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], 2, t['r_bias'], drop)['z']
        check_ln_bwd(f, '', e, t, z64, 2, True, drop, null=null)
    f.check()


def test_layernorm_running_dgamma_dbeta(dev):
    """dgamma / dbeta handed in as running gradients: the launch adds to them."""
    rows, D = R.LN_OPT_ROWS, R.LN_OPT_D
    t = R.ln_inputs(rows, D, bwd_slices=3)
    fw = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'])
    z32 = fw['z'].float()
    b, e = ln_bwd_problem(dev, t, z32, fw['mean'].float(), fw['rstd'].float(), n_parts=3, running=True, want_dr=False)
    launch('layernorm_bwd', [b])
    f = Figures('layernorm running gradients')
    check_ln_bwd(f, '', e, t, z32, 3, False, None, running=True)
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm: value edges
def test_layernorm_constant_rows_give_beta_exactly(dev):
    rows, D = R.LN_EDGE_ROWS, R.LN_EDGE_D
    t = R.ln_inputs(rows, D)
    t['x'] = torch.full((rows, D), 0.5)
    a, d = ln_fwd_problem(dev, t, plain=True)
    launch('layernorm_fwd', [a])
    f = Figures('layernorm constant rows')
    f.exact('y == beta', torch.equal(d['y'].cpu(), t['beta'].expand(rows, D)))
    f.exact('mean == 0.5', bool((d['mean'] == 0.5).all()))
    f.add('rstd vs eps^-1/2', d['rstd'], torch.full((rows,), R.as_f32(R.LN_EPS) ** -0.5, dtype=R.F64), R.fp32_bound('ln_rstd'))
    f.check()


def test_layernorm_rows_offset_by_100(dev):
    """Unit spread around +100: a one-pass variance E[z^2] - mean^2 would be off by orders of magnitude (test_token_rows_ref_cpu.py shows it)."""
    rows, D = R.LN_EDGE_ROWS, R.LN_EDGE_D
    t = R.ln_inputs(rows, D, offset=R.LN_OFFSET)
    a, d = ln_fwd_problem(dev, t, plain=True)
    launch('layernorm_fwd', [a])
    b, e = ln_bwd_problem(dev, t, d['z'], d['mean'], d['rstd'], want_dr=False)
    launch('layernorm_bwd', [b])
    ref = R.ln_fwd_ref(t['x'], None, t['gamma'], t['beta'])
    rb = R.ln_bwd_ref(ref['z'], t['gamma'], t['dy'])
    f = Figures('layernorm +100 rows')
    f.add('y', d['y'], ref['y'], R.fp32_bound('ln_offset_y'))
    f.add('mean', d['mean'], ref['mean'], R.fp32_bound('ln_mean'))
    f.add('rstd', d['rstd'], ref['rstd'], R.fp32_bound('ln_rstd'))
    for k in ('dx', 'dgamma', 'dbeta'):
        f.add(k, e[k], rb[k], R.fp32_bound('ln_offset_grad'))
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ sum_parts
@pytest.mark.parametrize('n', R.SUM_NS, ids=lambda n: f'n{n}-' + '.'.join(sorted(R.sum_parts_path(n, 1) - {'one_round_ragged'})))
def test_sum_parts_bit_equal_to_sequential_float32_sum(dev, n):
    """out = base (or 0) + parts[0] + parts[1] + ...: every slice count of SUM_SLICES, with and without base, slices n and n + 64 floats apart."""
    core, blocks = _hip()
    base, parts = R.sum_parts_inputs(n)
    base_d, parts_d = base.to(dev), parts.to(dev)
    f = Figures(f'sum_parts n {n}')
    for pad in R.SUM_STRIDE_PAD:
        stride = n + pad
        pd = parts_d if pad == max(R.SUM_STRIDE_PAD) else parts_d[:, :n].contiguous()
        assert pd.stride(0) == stride
        for slices in R.SUM_SLICES:
            for use_base in (False, True):
                out = canary(dev, n + 4)
                core.check(core.lib().ldetr_sum_parts_f32(core.ptr(base_d) if use_base else None, core.ptr(pd) if slices else None, slices, stride, core.ptr(out), n,
                                                          core.stream()), 'sum_parts')
                torch.cuda.synchronize()
                want = R.sum_parts_ref(base if use_base else None, parts, slices, n, R.F32)
                f.exact(f'stride n + {pad}, {slices} slices, base {int(use_base)}', torch.equal(out[:n].cpu(), want) and untouched(out[n:]))
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ cross entropy
def run_xent(dev, x, t, pad, eps, g=R.XENT_G, inplace=False, backward=True):
    """Forward and backward as training/med.py calls them.  The logits lie in a [rows, V + pad] buffer whose padding columns hold NaN (a read of
    them would poison the result); the gradient buffer is pre-filled with CANARY.  -> dict(loss_sum, count, lse, d, d_pad)"""
    core, blocks = _hip()
    rows, V = x.shape
    ld = V + pad
    buf = torch.full((rows, ld), float('nan'))
    buf[:, :V] = x
    xd, td = buf.to(dev), t.to(dev)
    lse, acc = canary(dev, rows), torch.zeros(2, device=dev)
    core.check(core.lib().ldetr_softmax_xent_fwd_f32(core.ptr(xd), ld, core.ptr(td), core.ptr(lse), ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(acc.data_ptr() + 4),
                                                     rows, V, R.XENT_IGNORE, eps, core.stream()), 'softmax_xent_fwd')
    out = dict(lse=lse)
    if backward:
        gd = torch.tensor([g], device=dev, dtype=torch.float32)
        dx = xd if inplace else canary(dev, rows, ld)
        core.check(core.lib().ldetr_softmax_xent_bwd_f32(core.ptr(xd), ld, core.ptr(td), core.ptr(lse), ctypes.c_void_p(acc.data_ptr() + 4), core.ptr(gd), core.ptr(dx), ld,
                                                         rows, V, R.XENT_IGNORE, eps, core.stream()), 'softmax_xent_bwd')
        out.update(d=dx[:, :V], d_pad=dx[:, V:])
    torch.cuda.synchronize()
    out.update(loss_sum=float(acc[0]), count=float(acc[1]), acc=acc)
    return out


def check_xent(f, got, x, t, eps, inplace=False, loss_key=None, d_key=None, sum_key=None):
    """Project bounds on the mean loss and dlogits unless a float32-yardstick key is given."""
    V = x.shape[1]
    loss_sum, count, lse, d = R.xent_ref(x, t, R.XENT_IGNORE, eps, R.XENT_G)
    valid = (t != R.XENT_IGNORE) & (t >= 0) & (t < V)
    f.exact('count', got['count'] == count)
    f.exact('finite', bool(torch.isfinite(got['d']).all()) and bool(torch.isfinite(got['lse']).all()) and np.isfinite(got['loss_sum']))
    f.exact('zero gradient and row_lse at ignored and out-of-range rows', not bool(got['d'][~valid.to(got['d'].device)].any()) and not bool(got['lse'].cpu()[~valid].any()))
    f.exact('padding columns untouched', bool(got['d_pad'].isnan().all()) if inplace else untouched(got['d_pad']))
    if count:
        mean, ref = got['loss_sum'] / got['count'], float(loss_sum) / count
        if loss_key:
            f.value('mean loss (relative)', abs(mean - ref) / abs(ref), R.fp32_bound(loss_key))
        else:
            f.value('mean loss', abs(mean - ref), R.TOL_XENT['loss_rel'] * abs(ref) + R.TOL_XENT['loss_abs'])
        if sum_key:
            f.value('loss sum (relative)', abs(got['loss_sum'] - float(loss_sum)) / abs(float(loss_sum)), R.fp32_bound(sum_key))
        f.add('row_lse', got['lse'], lse, R.TOL_XENT['loss_rel'])        # the loss's leading term, held to the loss's relative bound
        f.add('dlogits', got['d'], d, R.fp32_bound(d_key) if d_key else R.TOL_XENT['dlogits'])
    else:
        f.exact('loss_sum == 0', got['loss_sum'] == 0.0)
        f.exact('dlogits == 0', not bool(got['d'].any()))


@pytest.mark.parametrize('eps', R.XENT_EPS, ids=lambda e: f'eps{e}')
@pytest.mark.parametrize('shape', R.XENT_SHAPES, ids=lambda s: f'rows{s[0]}-V{s[1]}-pad{s[2]}-' + '.'.join(sorted(R.xent_path(*s))))
def test_xent_every_path_with_ignored_and_out_of_range_targets(dev, shape, eps):
    rows, V, pad = shape
    x, t = R.xent_inputs(rows, V)
    got = run_xent(dev, x, t, pad, eps)
    f = Figures(f'xent {shape} eps {eps}')
    check_xent(f, got, x, t, eps, sum_key='xent_big_loss_sum' if rows == R.XENT_BIG_ROWS else None)
    f.check()


def test_xent_all_targets_ignored(dev):
    x, t = R.xent_inputs(37, 70, 'all_ignored')
    got = run_xent(dev, x, t, 2, 0.1)
    f = Figures('xent all ignored')
    check_xent(f, got, x, t, 0.1)
    f.exact('loss_sum == count == 0', got['loss_sum'] == 0.0 and got['count'] == 0.0)
    f.check()


@pytest.mark.parametrize('eps', R.XENT_EPS, ids=lambda e: f'eps{e}')
def test_xent_logits_times_30(dev, eps):
    rows, V, scale = R.XENT_X30
    x, t = R.xent_inputs(rows, V, scale=scale)
    got = run_xent(dev, x, t, 2, eps)
    f = Figures(f'xent logits x 30 eps {eps}')
    check_xent(f, got, x, t, eps, loss_key='xent_x30_loss', d_key='xent_x30_dlogits')
    f.check()


def test_xent_rows_with_neg_inf_logits(dev):
    """eps 0, V = 1028: columns 0..7 are -inf in every row (threads 0 and 1 start on four -inf logits) and 1024..1027 in the odd rows (thread 0's
    second quad as well), targets on finite columns: F.cross_entropy is finite there, and so must the kernel be."""
    x, t = R.xent_inputs(9, 1028, 'neg_inf')
    got = run_xent(dev, x, t, 64, 0.0)
    f = Figures('xent -inf logits')
    check_xent(f, got, x, t, 0.0)
    f.exact('zero gradient at -inf logits', not bool(got['d'][:, :8].any()))
    f.check()


def test_xent_backward_in_place(dev):
    """dlogits == logits, which include/ldetr_hip.h allows."""
    x, t = R.xent_inputs(37, 70)
    got = run_xent(dev, x, t, 2, 0.1, inplace=True)
    f = Figures('xent in place')
    check_xent(f, got, x, t, 0.1, inplace=True)
    f.exact('same bits as out of place', torch.equal(got['d'], run_xent(dev, x, t, 2, 0.1)['d']))
    f.check()


def golden_xent_run(dev):
    """What tests/golden/xent_guard.npz records: row_lse of 1030 all-valid rows (blocks 0..5 take a second row), and row_lse / loss_sum / count of
    2049 rows of which only block 0's three are valid (one atomic, so the sum is reproducible)."""
    c = R.GOLDEN_XENT
    x = R.golden_logits(c['rows_lse'], c['V'])
    a = run_xent(dev, x, R.golden_targets(c['rows_lse'], c['V']), c['pad'], c['eps'], backward=False)
    x = R.golden_logits(c['rows_sum'], c['V'])
    b = run_xent(dev, x, R.golden_targets(c['rows_sum'], c['V'], only_block0=True), c['pad'], c['eps'], backward=False)
    return dict(lse_1030=a['lse'].cpu().numpy(), lse_2049=b['lse'].cpu().numpy(), acc_2049=b['acc'].cpu().numpy())


def test_xent_finite_rows_bit_identical_to_the_kernel_before_the_neg_inf_guard(dev):
    """row_lse and loss_sum of all-finite rows equal, bit for bit, what the kernel gave before its per-thread updates were guarded against
    -inf - (-inf) (recorded from that build on an MI355X)."""
    want = np.load(GOLDEN)
    got = golden_xent_run(dev)
    f = Figures('xent golden')
    for k in ('lse_1030', 'lse_2049', 'acc_2049'):
        diff = got[k].view(np.int32).astype(np.int64) - want[k].view(np.int32).astype(np.int64)
        print(f'[token rows] xent golden: {k}: {int((diff != 0).sum())} of {diff.size} values differ, by at most {int(np.abs(diff).max())} ulp')
        f.exact(k, np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)))
    f.exact('three valid rows', float(got['acc_2049'][1]) == 3.0)
    f.check()


# ------------------------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize('case', R.EMB_CASES, ids=lambda c: f'n{c[0]}-T{c[1]}-V{c[2]}-d{c[3]}-{c[4]}-' + '.'.join(sorted(R.emb_path(*c[:4]))))
def test_embedding_gather_and_scatter(dev, case):
    """Gather with and without position rows (bit-equal; ids outside [0, V) give pos alone or zeros), scatter with padding_idx 0 and -1 into a
    zeroed and into a running dweight."""
    core, blocks = _hip()
    n, T, V, d, kind = case
    t = R.emb_inputs(n, T, V, d, kind)
    ids = t['ids']
    ids_d, w_d, pos_d, dy_d = ids.to(dev), t['w'].to(dev), t['pos'].to(dev), t['dy'].to(dev)
    oor = (ids < 0) | (ids >= V)
    f = Figures(f'embedding {case}')
    for use_pos in (False, True):
        out = canary(dev, n + 1, d)
        if use_pos:        # training/med.py
            core.check(core.lib().ldetr_embedding_fwd_f32(core.ptr(w_d), core.ptr(pos_d), core.ptr(ids_d), core.ptr(out), n, d, V, T, core.stream()), 'embedding_fwd')
        else:              # training/networks_detr.py
            core.check(core.lib().ldetr_embedding_fwd_f32(core.ptr(w_d), None, core.ptr(ids_d), core.ptr(out), n, d, V, 1, core.stream()), 'embedding_fwd')
        torch.cuda.synchronize()
        want, _ = R.embedding_ref(t['w'], ids, t['pos'] if use_pos else None, T, dtype=R.F32)
        o = out[:n].cpu()
        f.exact(f'gather pos {int(use_pos)}', torch.equal(o, want) and untouched(out[n:]))
        f.exact(f'out-of-range rows pos {int(use_pos)}', torch.equal(o[oor], t['pos'][torch.arange(n) % T][oor]) if use_pos else not bool(o[oor].any()))
    for pad in (0, -1):
        for running in (False, True):
            dw = t['dw0'].to(dev) if running else torch.zeros(V, d, device=dev)
            core.check(core.lib().ldetr_embedding_bwd_f32(core.ptr(dy_d), core.ptr(ids_d), core.ptr(dw), n, d, V, pad, core.stream()), 'embedding_bwd')
            torch.cuda.synchronize()
            _, want = R.embedding_ref(t['w'], ids, None, T, pad, t['dy'], t['dw0'] if running else None)
            f.add(f'scatter padding_idx {pad} running {int(running)}', dw, want, R.TOL_EMB)
            hit = torch.zeros(V, dtype=torch.bool)
            hit[ids[~oor & (ids != pad)]] = True
            start = t['dw0'] if running else torch.zeros(V, d)
            f.exact(f'rows without a token (padding row included) unchanged, padding_idx {pad} running {int(running)}', torch.equal(dw.cpu()[~hit], start[~hit]))
    f.check()
