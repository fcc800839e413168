"""CPU tests (no GPU) of layout generation (layoutdetr_amd/generate.py): the host-side draws against the reference's own (fixture
tests/golden/generate.npz, written by tools/gen_generate_golden.py), the argument checks of ldetr_layout_finish_f32, which fire before any
launch, the prefix-mask check and the command line's option parsing."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'generate.npz')


@pytest.fixture(scope='module')
def gold():
    d = np.load(GOLDEN, allow_pickle=False)
    return {k: d[k] for k in d.files}


def test_latents_and_jitter_factors_equal_the_reference_draws_bit_for_bit(gold):
    from layoutdetr_amd import generate
    seeds = gold['draw_seeds'].tolist()
    z = generate.latents(seeds, 4)
    assert z.dtype == torch.float32 and tuple(z.shape) == (len(seeds), 9, 4)
    assert np.array_equal(z.numpy(), gold['latents'])
    f = generate.jitter_factors(seeds)            # default strength 0.2: generate_util.py's log(0.8) .. log(1.2)
    assert f.dtype == torch.float32 and tuple(f.shape) == (len(seeds), 9, 4)
    assert np.array_equal(f.numpy(), gold['jitter_factors'])
    assert np.array_equal(generate.jitter_factors(seeds, strength=0.2).numpy(), gold['jitter_factors'])
    assert not np.array_equal(generate.jitter_factors(seeds, strength=0.1).numpy(), gold['jitter_factors'])


def test_reference_plan_draws_in_the_reference_order(gold):
    from layoutdetr_amd import generate
    seeds = gold['plan_seeds'].tolist()
    pp = {'jitter': float(gold['plan_probs'][0]), 'horizontal_center_aligned': float(gold['plan_probs'][1])}
    want = [(bool(j), generate.CENTER if c else generate.LEFT) for j, c in zip(gold['plan_jitter'], gold['plan_center'])]
    assert generate.reference_plan(seeds, pp, np.random.RandomState(0)) == want
    np.random.seed(0)                             # the reference's own source
    assert generate.reference_plan(seeds, pp) == want
    assert seeds[0] == 1 and want[0][0] is False  # seed 1 is never jittered ...
    # ... and draws no number for it: with seed 1 first, the stream is one draw shorter than with another seed first
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    generate.reference_plan([1], pp, a); generate.reference_plan([2], pp, b)
    assert a.rand() != b.rand()
    c = np.random.RandomState(3); c.rand()
    assert generate.reference_plan([5], {}, c) == [(False, generate.LEFT)] and c.rand() == np.random.RandomState(3).rand(2)[1]    # no key, no draw


def test_layout_finish_argument_checks_fire_before_any_launch():
    from layoutdetr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    nine = [P(64)] * 9
    rc = lib.ldetr_layout_finish_f32(*nine, 1, 4, 17, None)
    assert rc != 0 and b'1 <= N <= 16' in lib.ldetr_last_error() and b'got 17' in lib.ldetr_last_error()
    assert lib.ldetr_layout_finish_f32(*nine, 2, 0, 9, None) == 0                       # K = 0: nothing to do, nothing touched
    assert lib.ldetr_layout_finish_f32(*([None] * 9), 0, 5, 9, None) == 0               # C = 0 likewise
    rc = lib.ldetr_layout_finish_f32(None, *nine[1:], 1, 4, 9, None)
    assert rc != 0 and b'bbox_in is null' in lib.ldetr_last_error()
    rc = lib.ldetr_layout_finish_f32(*nine, 1, 1025, 9, None)
    assert rc != 0 and b'K <= 1024' in lib.ldetr_last_error()
    rc = lib.ldetr_layout_finish_f32(*nine[:8], None, 1, 4, 9, None)
    assert rc != 0 and b'null output' in lib.ldetr_last_error()


class _TinyG(torch.nn.Linear):
    z_dim = 4


def test_sampler_refuses_a_padding_mask_that_is_not_a_prefix():
    from layoutdetr_amd import generate
    from layoutdetr_amd.training.shared_decode import check_prefix_mask
    s = generate.Sampler(_TinyG(2, 2))
    pm = torch.zeros(1, 9, dtype=torch.bool)
    pm[0, 3] = True                               # a hole: slot 3 padded, slots 4.. valid
    with pytest.raises(ValueError, match='prefix mask'):
        s.encode(torch.zeros(1, 3, 32, 32), None, torch.zeros(1, 9, dtype=torch.int64), padding_mask=pm)
    ok = torch.arange(9)[None, :] >= torch.tensor([[4], [9], [1]])
    assert torch.equal(check_prefix_mask(ok), ok)


def test_cli_option_parsing():
    from layoutdetr_amd import generate
    assert generate.parse_range('1,3-5') == [1, 3, 4, 5] and generate.parse_range('7') == [7] and generate.parse_range('0-2,9') == [0, 1, 2, 9]
    assert generate.parse_labels('header|button') == [0, 5]
    assert generate.parse_labels('disclaimer / footnote|logo|body') == [4, 7, 3]
    with pytest.raises(ValueError, match='unknown label'):
        generate.parse_labels('header|title')
    a = generate.parse_args(['--ckpt', 's.pkl', '--bg', 'b.png', '--strings', 'Sale|Shop now', '--string-labels', 'header|button', '--seeds', '1,3-5',
                             '--out-postprocessing', 'horizontal_left_aligned', '--out-jittering-strength', '0.1', '--outfile', 'out/x'])
    assert a.seeds == [1, 3, 4, 5] and a.texts == ['Sale', 'Shop now'] and a.labels == [0, 5] and a.mode == generate.LEFT
    assert a.out_jittering_strength == 0.1 and a.outfile == 'out/x' and a.bg_preprocessing == 'none'
    with pytest.raises(ValueError, match='same number'):
        generate.parse_args(['--ckpt', 's', '--bg', 'b', '--strings', 'a|b', '--string-labels', 'header', '--outfile', 'x'])
