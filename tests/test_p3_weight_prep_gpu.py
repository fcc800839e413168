"""ldetr_p3_weight_prep (csrc/p3_engine.hip: p3_weight_prep_kernel) writes the data-gradient image [I][T][O] tile by tile through an LDS transpose
(one tap x 8 out-channel groups x 32 in channels per tile, a run of contiguous bytes per (i, tap)); the images must stay what the single-tensor
entry points write, byte for byte: the forward image ldetr_p3_split_f32 of the weight as stored, the data-gradient image ldetr_p3_weight_bwd's.

Shapes (O, I, T): (8, 8, 1) one unit; (64, 64, 1) and (64, 64, 9) whole tiles; (256, 64, 1) and (64, 256, 1) several group / channel tiles;
(128, 128, 9) the trunk's 3x3 form; (24, 40, 9) ragged in both directions, where a conv has more tiles than blocks and its blocks walk them.
Tables of one to three convs, with and without the folded scale, forward image only, data-gradient image only, and both; a guard band on either
side of both destination buffers stays untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 1), (64, 64, 1), (256, 64, 1), (64, 256, 1), (64, 64, 9), (128, 128, 9), (24, 40, 9)]      # (O, I, T)
TABLES = [[s] for s in SHAPES] + [[(24, 40, 9), (64, 64, 1)], [(8, 8, 1), (24, 40, 9), (256, 64, 1)], [(128, 128, 9), (64, 256, 1), (24, 40, 9)]]
GUARD = 4096
FILL = 0xA5


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


def split_image(core, w):
    x = w.reshape(w.shape[0], -1)
    out = torch.empty(x.numel() * 6, dtype=torch.uint8, device=w.device)
    core.check(core.lib().ldetr_p3_split_f32(core.ptr(x), x.stride(0), core.ptr(out), x.shape[0], x.shape[1], core.stream()), 'split')
    return out


def bwd_image(core, w, scale):
    O, T, _, I = w.shape
    out = torch.empty(w.numel() * 6, dtype=torch.uint8, device=w.device)
    core.check(core.lib().ldetr_p3_weight_bwd(core.ptr(w), core.ptr(scale), core.ptr(out), O, T, 1, I, core.stream()), 'weight_bwd')
    return out


_WEIGHTS = {}


def weights(dev, table):
    """[(w [O][T][1][I], scale [O])] of a table, built once; the first element of every weight is made non-finite in turn (stored as (x, 0, 0))."""
    key = tuple(table)
    if key not in _WEIGHTS:
        gen = torch.Generator().manual_seed(31 + 7 * len(table) + table[0][0])
        out = []
        for k, (O, I, T) in enumerate(table):
            w = torch.randn(O, T, 1, I, generator=gen)
            w.view(-1)[k] = [float('inf'), float('nan'), 3.3e38][k % 3]
            out.append((w.to(dev), (torch.rand(O, generator=gen) + 0.5).to(dev)))
        _WEIGHTS[key] = out
    return _WEIGHTS[key]


@pytest.mark.parametrize('which', ['fwd', 'bwd', 'both'])
@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
@pytest.mark.parametrize('table', TABLES, ids=lambda t: '+'.join(f'{o}x{i}x{k}' for o, i, k in t))
def test_weight_prep_images_byte_for_byte(dev, table, scaled, which):
    core = _core()
    ws = weights(dev, table)
    total = sum(w.numel() * 6 for w, _ in ws)
    fwd = torch.full((total + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    bwd = torch.full((total + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    rows, off, blk = [], GUARD, 0
    for k, (w, sc) in enumerate(ws):
        O, T, _, I = w.shape
        use_sc = scaled and k % 2 == 0           # (in a table of several convs: some with, some without)
        rows.append([w.data_ptr(), sc.data_ptr() if use_sc else 0, fwd.data_ptr() + off if which != 'bwd' else 0, bwd.data_ptr() + off if which != 'fwd' else 0,
                     O, T, I, blk])
        off += w.numel() * 6
        blk += (w.numel() // 8 + 255) // 256
    tab = torch.tensor(rows, dtype=torch.int64, device=dev)
    core.check(core.lib().ldetr_p3_weight_prep(core.ptr(tab), len(ws), blk, core.stream()), 'prep')
    torch.cuda.synchronize()
    for name, buf in (('forward', fwd), ('data-gradient', bwd)):
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + total:] == FILL).all()), f'{name} image: guard band written'
    off = GUARD
    for k, (w, sc) in enumerate(ws):
        n = w.numel() * 6
        if which != 'bwd':
            assert torch.equal(fwd[off:off + n], split_image(core, w)), f'conv {k} {tuple(w.shape)}: forward image differs from ldetr_p3_split_f32'
        else:
            assert bool((fwd[off:off + n] == FILL).all()), f'conv {k}: forward image written without a destination'
        if which != 'fwd':
            assert torch.equal(bwd[off:off + n], bwd_image(core, w, sc if scaled and k % 2 == 0 else None)), \
                f'conv {k} {tuple(w.shape)}: data-gradient image differs from ldetr_p3_weight_bwd'
        else:
            assert bool((bwd[off:off + n] == FILL).all()), f'conv {k}: data-gradient image written without a destination'
        off += n
