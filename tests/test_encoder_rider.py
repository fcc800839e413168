"""The encoder rider's host-side rules (no GPU): the LDETR_DEBUG switch, the eligibility predicate, the seed lease."""
import os
import subprocess
import sys

import torch

from layoutdetr_amd.hip import core, rider
from layoutdetr_amd.training.detr_transformer import TransformerEncoder, TransformerEncoderLayer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enc(d=256, heads=8, ff=2048, layers=2, norm=None):
    return TransformerEncoder(TransformerEncoderLayer(d, heads, ff, 0.1), layers, norm)


def test_enc_rider_switch_parses(monkeypatch):
    monkeypatch.setenv('LDETR_DEBUG', 'FFN_MAX_ROWS=512,ENC_RIDER=0')
    assert core.knob('ENC_RIDER', 1) == 0
    monkeypatch.setenv('LDETR_DEBUG', 'ENC_RIDER=1')
    assert core.knob('ENC_RIDER', 0) == 1
    monkeypatch.delenv('LDETR_DEBUG')
    assert core.knob('ENC_RIDER', 1) == 1
    code = 'from layoutdetr_amd.hip import rider; print(int(rider.ENABLED))'
    for value, want in (('ENC_RIDER=0', '0'), ('', '1')):
        env = dict(os.environ, LDETR_DEBUG=value)
        out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
        assert out.strip().splitlines()[-1] == want


def test_eligibility(monkeypatch):
    a = _enc()
    assert rider.eligible(a, _enc(), 1024, 2048)
    assert rider.eligible(a, _enc(), 128, 256)
    assert not rider.eligible(a, _enc(layers=3), 1024, 1024)                  # depth
    assert not rider.eligible(a, _enc(d=512, heads=16), 1024, 1024)           # width
    assert not rider.eligible(a, _enc(heads=4), 1024, 1024)                   # heads
    assert not rider.eligible(a, _enc(ff=1024), 1024, 1024)                   # feed-forward size
    assert not rider.eligible(a, _enc(norm=torch.nn.LayerNorm(256)), 1024, 1024)
    assert not rider.eligible(a, _enc(), 128, 1024)                           # one stack on the fused feed-forward block, the other above its limit
    assert not rider.eligible(a, _enc(), 1024, 1024, staged=True)             # a staged backward
    assert not rider.eligible(a, _enc(), 1024, 1024, higher_order=True)       # a regulariser pass
    assert not rider.eligible(a, _enc(), 1024, 1024, profiled=True)
    monkeypatch.setattr(rider, 'ENABLED', False)
    assert not rider.eligible(a, _enc(), 1024, 1024)


def _loss_on_stubs():
    """A StyleGAN2Loss over stand-ins that carry what the partner decision reads: the two transformers, the trunk bodies, D's partner hook."""
    from types import SimpleNamespace as NS

    from layoutdetr_amd.training.detr_transformer import Transformer
    from layoutdetr_amd.training.loss import StyleGAN2Loss
    mk = lambda: Transformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=1, dim_feedforward=64)
    G = NS(transformer=mk(), backbone=[NS(body=NS(stages=None))], training=True)
    D = NS(enc_transformer=mk(), backbone=[NS(body=NS(stages=None))], training=True, encoder_partner=lambda *a, **k: 'partner')
    return StyleGAN2Loss('cpu', G, D, share_D_trunk='iteration'), G, D


def test_a_staged_backward_keeps_the_encoders_apart():
    """The detection itself, through training_loop.staged_backward: with D's cuts recorded before the phases (`stages=` handed in: nothing is set on
    the trunk body) as well as with cuts recorded inside the phase (Gmain: the body is marked), the phase gets no partner; outside it does."""
    from types import SimpleNamespace as NS

    from layoutdetr_amd.training import training_loop as tl
    loss, G, D = _loss_on_stubs()
    bg, trunk = torch.zeros(2, 3, 64, 64), object()
    assert loss.encoder_partner('Dmain', trunk, bg, pair=True) == 'partner'
    assert loss.encoder_partner('Dmain', None, bg, pair=True) is None                  # no trunk output in hand
    assert loss.encoder_partner('Dmain', trunk, [bg[0], bg[1]], pair=True) is None     # ragged backgrounds
    seen = {}
    for name, module, handed in (('Dmain', D, tl.BackwardStages(3)), ('Gmain', G, None)):
        phase = NS(name=name, module=module, fm=NS(stage_segments=lambda n=3: [[(0, 1)], [(1, 2)], [(2, 3)]][:n], gflat=None))

        def stage1(name=name):
            seen[name] = (loss.encoder_partner(name, trunk, bg, pair=name == 'Dmain'), module.backbone[0].body.stages is not None)
        assert tl.staged_backward(loss, phase, None, stage1, exchange=lambda ranges: None, stages=handed, n_stages=3) is True
    assert seen['Dmain'] == (None, False)      # the handed-in stages leave the body unmarked: the driver's word alone keeps the passes apart
    assert seen['Gmain'] == (None, True)
    assert loss.backward_staged is False
    assert loss.encoder_partner('Dmain', trunk, bg, pair=True) == 'partner'


def test_recording_refuses_reads_of_unwritten_results():
    """While a stack is recorded, an ATen read (an add, a layout / dtype copy) of a tensor that a queued launch has yet to write raises."""
    import pytest
    out, other = torch.zeros(4, 8), torch.zeros(4, 8)
    try:
        with rider.mode('record'):
            rider._Pending('gemm', None, (), outs=(out,))
            rider.check_ready(other, 'add')
            core.f32c(out)                                   # contiguous fp32: no copy, nothing is read
            core.f32c(other.t())
            with pytest.raises(RuntimeError, match='queued'):
                rider.check_ready(out[1:], 'add')
            with pytest.raises(RuntimeError, match='queued'):
                core.f32c(out.t())
    finally:
        rider._unwritten.clear()
    rider.check_ready(out, 'add')                            # no mode: nothing to guard


def test_seed_lease_hands_out_the_seeds_of_its_place():
    start = core.seed_position()
    try:
        plain = [core.next_seed() for _ in range(5)]
        core._seed_counter[0] = start
        lease = core.SeedLease(start + 2)
        with lease:
            ahead = [core.next_seed() for _ in range(3)]
        assert core.seed_position() == start and ahead == plain[2:]
        assert not lease.redeem()                                             # the sequence is not at the lease's start yet
        assert [core.next_seed(), core.next_seed()] == plain[:2]
        assert lease.redeem() and core.seed_position() == start + 5
    finally:
        core._seed_counter[0] = start
