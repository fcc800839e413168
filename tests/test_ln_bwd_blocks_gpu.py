"""The backward of the grouped LayerNorm at both block shapes of ln_bwd_kernel (csrc/layernorm.hip): blocks of 4 rows, and blocks of 16 rows from 256
rows on (D <= 256), which put a quarter of the dgamma / dbeta atomics behind the same row loop.

Rows 1, 3, 4, 5 (one ragged block), 255 / 256 / 257 (either side of the switch; 257 with a ragged 16-row block), 1024 (many blocks in one sweep) and
2051 (beyond the 2048-row sweep of the capped grid: blocks loop over rows, ragged last block); D 64 (idle lanes), 256 (the step's case) and 512
(NV = 2: four-wave blocks at every row count).  One problem, and two problems of different row counts in one launch (the larger one decides the
block shape of both); 0 and 8 gradient slices; dropout off and on; dgamma / dbeta always start from non-zero running values.  Inputs, float64
references and bounds are tests/token_rows_common.py's (TOL_LN['grad'] = 1e-5 for dx / dr / dgamma / dbeta; the float32-baseline bounds for dgamma /
dbeta summed over more than 2048 rows, as test_token_rows_gpu.py applies them).  z, mean and rstd are handed in as the float32 roundings of the
float64 forward, so the backward is tested on its own.  dx and dr do not depend on the block shape or on the order of the atomics: they are
bit-equal between two runs, and between an eager launch and a captured graph's replays.  Every case prints its figures before it asserts."""
import pytest
import torch

import token_rows_common as R

pytestmark = pytest.mark.gpu

R.limit_threads()
ROWS = [1, 3, 4, 5, 255, 256, 257, 1024, 2051]
DS = [64, 256, 512]
SLICES = [0, 8]
P_DROP = 0.3
PAIRS = [(5, 1024, 256), (2051, 3, 256), (1024, 2051, 256), (5, 255, 256), (5, 2051, 64), (2051, 4, 512)]      # (rows of problem 0, of problem 1, D)


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
    torch.manual_seed(0x1B0 + case)
    core._seed_counter[0] = 0x7EED + 64 * case
    core.reseed(dev)
    word = core.iter_seed().item()
    assert word != 0
    return word


_INPUTS = {}


def inputs(rows, D, seed=0):
    """ln_inputs with 8 gradient slices and the float32 forward quantities, built once per shape and never written."""
    key = (rows, D, seed)
    if key not in _INPUTS:
        t = R.ln_inputs(rows, D, bwd_slices=max(SLICES), seed=seed)
        fw = R.ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'])
        t.update(z32=fw['z'].float(), mean32=fw['mean'].float(), rstd32=fw['rstd'].float())
        _INPUTS[key] = t
    return _INPUTS[key]


def problem(dev, t, n_parts, p, seed, dy_scale=1.0):
    """-> (argument block, device tensors); dgamma / dbeta preloaded with the running values dg0 / db0."""
    core, blocks = _hip()
    rows, D = t['dy'].shape
    d = dict(dy=(t['dy'] * dy_scale).to(dev), parts=t['parts'][:n_parts].contiguous().to(dev) if n_parts else None, z=t['z32'].to(dev), mean=t['mean32'].to(dev),
             rstd=t['rstd32'].to(dev), gamma=t['gamma'].to(dev), dx=torch.empty(rows, D, device=dev), dr=torch.empty(rows, D, device=dev),
             dgamma=t['dg0'].to(dev), dbeta=t['db0'].to(dev))
    a = blocks.ln_bwd(d['dy'], d['z'], d['mean'], d['rstd'], d['gamma'], d['dx'], d['dr'], d['dgamma'], d['dbeta'], p, seed, parts=d['parts'], n_parts=n_parts)
    return a, d


def launch(args):
    core, blocks = _hip()
    blocks.launch('layernorm_bwd', args)
    torch.cuda.synchronize()


def bounds(rows):
    """test_token_rows_gpu.check_ln_bwd's: the project's gradient bound, and the float32-baseline bounds where the sums run over more than one sweep."""
    big = rows > R.LN_MAX_BWD_BLOCKS * R.LN_ROWS_PER_BLOCK
    return dict(dx=R.TOL_LN['grad'], dr=R.TOL_LN['grad'], dgamma=R.fp32_bound('ln_big_dgamma') if big else R.TOL_LN['grad'],
                dbeta=R.fp32_bound('ln_big_dbeta') if big else R.TOL_LN['grad'])


def check(tag, d, t, n_parts, drop, dy_scale=1.0, times=1):
    """The four outputs against float64; `times` launches on the same buffers add `times` sums to the running values."""
    rows = t['dy'].shape[0]
    ref = R.ln_bwd_ref(t['z32'], t['gamma'], t['dy'] * dy_scale, None, t['parts'], n_parts, drop)
    want = dict(dx=ref['dx'], dr=ref['dr'], dgamma=t['dg0'].double() + times * ref['dgamma'], dbeta=t['db0'].double() + times * ref['dbeta'])
    tol = bounds(rows)
    bad = []
    for k in ('dx', 'dr', 'dgamma', 'dbeta'):
        e = R.rel_err(d[k], want[k])
        print(f'[ln bwd blocks] {tag}: {k} err {e:.3e} (bound {tol[k]:.2e})')
        if not e <= tol[k]:
            bad.append(f'{k}: {e:.3e} > {tol[k]:.2e}')
    if drop is not None and bool(d['dr'].cpu()[drop == 0].any()):
        bad.append('dr != 0 where dropped')
    return bad


def same_bits(tag, d, e, bad):
    for k in ('dx', 'dr'):
        if not torch.equal(d[k], e[k]):
            bad.append(f'{tag}: {k} differs between two runs')


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('rows', ROWS)
def test_one_problem_vs_fp64(dev, rows, D):
    """With 0 and 8 gradient slices, dropout off and on; a second run from the same inputs gives the same dx / dr."""
    core, blocks = _hip()
    t = inputs(rows, D)
    bad = []
    for n_parts in SLICES:
        for p in (0.0, P_DROP):
            word = pin_seeds(core, dev, 10 * ROWS.index(rows) + DS.index(D))
            seed = core.next_seed() if p > 0 else 0
            drop = R.drop_rows(seed, word, p, rows, D)
            tag = f'rows {rows} D {D} slices {n_parts} p {p}'
            a, d = problem(dev, t, n_parts, p, seed)
            launch([a])
            bad += [f'{tag}: {b}' for b in check(tag, d, t, n_parts, drop)]
            a2, d2 = problem(dev, t, n_parts, p, seed)
            launch([a2])
            same_bits(tag, d, d2, bad)
    assert not bad, '; '.join(bad)


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('rows', ROWS)
def test_three_launches_accumulate_like_one_of_threefold_dy(dev, rows, D):
    """dgamma / dbeta are running sums: three launches on the same buffers leave running + 3 x sum, which is what one launch of 3 x dy leaves
    (both within the bound of the float64 value)."""
    t = inputs(rows, D)
    tag = f'rows {rows} D {D}'
    a, d = problem(dev, t, 0, 0.0, 0)
    for _ in range(3):
        launch([a])
    bad = check(tag + ' three launches', d, t, 0, None, times=3)
    a3, d3 = problem(dev, t, 0, 0.0, 0, dy_scale=3.0)
    launch([a3])
    bad += check(tag + ' one launch of 3 dy', d3, t, 0, None, dy_scale=3.0)
    for k in ('dgamma', 'dbeta'):
        e = R.rel_err(d[k], d3[k])
        print(f'[ln bwd blocks] {tag}: {k} three launches vs one of 3 dy {e:.3e}')
        if not e <= 2 * bounds(rows)[k]:      # each side is within the bound of the same float64 value
            bad.append(f'{k}: three launches differ from one of 3 dy by {e:.3e}')
    assert not bad, '; '.join(bad)


def pair(dev, core, case, index):
    rows0, rows1, D = case
    word = pin_seeds(core, dev, 200 + index)
    out = []
    for i, (rows, n_parts, p) in enumerate(((rows0, 8, P_DROP), (rows1, 0, 0.0))):
        t = inputs(rows, D, seed=i + 1)
        seed = core.next_seed() if p > 0 else 0
        out.append((t, n_parts, R.drop_rows(seed, word, p, rows, D), problem(dev, t, n_parts, p, seed)))
    return out


@pytest.mark.parametrize('case', PAIRS, ids=lambda c: f'rows{c[0]}+{c[1]}-D{c[2]}')
def test_two_problems_in_one_launch(dev, case):
    """Two problems of different row counts in one launch, each against its own reference."""
    core, blocks = _hip()
    first = pair(dev, core, case, PAIRS.index(case))
    launch([a for _, _, _, (a, _) in first])
    second = pair(dev, core, case, PAIRS.index(case))
    launch([a for _, _, _, (a, _) in second])
    bad = []
    for i, ((t, n_parts, drop, (_, d)), (_, _, _, (_, d2))) in enumerate(zip(first, second)):
        tag = f'pair {case} problem {i}'
        bad += [f'{tag}: {b}' for b in check(tag, d, t, n_parts, drop)]
        same_bits(tag, d, d2, bad)
    assert not bad, '; '.join(bad)


@pytest.mark.parametrize('case', [PAIRS[2], PAIRS[5]], ids=lambda c: f'rows{c[0]}+{c[1]}-D{c[2]}')
def test_captured_graph_replayed_twice(dev, case):
    """The launch captured in a graph (running values restored inside the capture) and replayed twice: both replays within the bounds, dx / dr
    the eager launch's bits."""
    core, blocks = _hip()
    eager = pair(dev, core, case, 300)
    launch([a for _, _, _, (a, _) in eager])
    cap = pair(dev, core, case, 300)
    args = [a for _, _, _, (a, _) in cap]
    run0 = [(d['dgamma'].clone(), d['dbeta'].clone()) for _, _, _, (_, d) in cap]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for (g0, b0), (_, _, _, (_, d)) in zip(run0, cap):
            d['dgamma'].copy_(g0); d['dbeta'].copy_(b0)
        blocks.launch('layernorm_bwd', args)
    bad = []
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for i, ((t, n_parts, drop, (_, d)), (_, _, _, (_, e))) in enumerate(zip(cap, eager)):
            tag = f'graph {case} replay {replay} problem {i}'
            bad += [f'{tag}: {b}' for b in check(tag, d, t, n_parts, drop)]
            same_bits(tag + ' (against the eager launch)', d, e, bad)
    assert not bad, '; '.join(bad)
