"""Two independent encoder stacks advanced in lock-step, one launch per step for both (training/detr_transformer.py: the encoder rider).

The rider stack (the one that needs no autograd graph) runs its ordinary Python path first in RECORD mode: every forward launch it would issue
(nn.Linear-shaped GEMM, fused attention, LayerNorm / feed-forward block) is queued with its argument block instead of being sent.  The owner stack
then runs its ordinary path in PAIR mode: at each of its launches the head of the queue, if it is the same kind of launch, goes out with it as ONE
two-problem launch (ldetr_gemm_pair_fwd_f32, ldetr_attention_fwd_group_f32, the token-block group entries), whose halves are bit-equal to the single
launches.  A pair the library does not take as one launch (another instantiation, a problem outside the small-tile class) is sent as two, what is
left in the queue when the owner is done is sent in order.  Nothing on the host reads a recorded launch's result before `flush`, and the queue keeps
every tensor of a recorded launch alive until it has been sent.  LDETR_DEBUG="ENC_RIDER=0" restores the single launches everywhere."""
import ctypes
import sys

from .. import _lib
from . import core

ENABLED = bool(core.knob('ENC_RIDER', 1))
MODE = None                             # None | 'record' | 'pair'
STATS = dict(paired=0, split=0, alone=0)      # launches sent as one for both stacks / pairs the library sent back / launches without a partner
_queue = []
_unwritten = set()                      # storages a queued launch will write: nothing but another queued launch may read them before `flush`
_BLOCK_KINDS = ('layernorm_fwd', 'ffn_fwd')


class _Pending(object):
    __slots__ = ('kind', 'args', 'keep')

    def __init__(self, kind, args, keep, outs=()):
        self.kind, self.args, self.keep = kind, args, keep
        if MODE == 'record':
            _unwritten.update(t.untyped_storage().data_ptr() for t in outs if t is not None)


def check_ready(t, what):
    """Called where something that is NOT a queued launch is about to read tensor `t` on the device (an ATen add, a layout / dtype copy): while a
    stack is being recorded, `t` must not be the result of a launch that is still in the queue -- it has not been written yet."""
    if MODE == 'record' and t is not None and t.untyped_storage().data_ptr() in _unwritten:
        raise RuntimeError(f'{what}: reads the result of a launch that hip.rider has queued and not sent yet')


def _take(kind):
    if _queue and _queue[0].kind == kind:
        return _queue.pop(0)
    return None


def _send_alone(p):
    l = core.lib()
    if p.kind == 'gemm':
        d = p.args
        ep = ctypes.cast(d.ep, ctypes.POINTER(_lib.Epilogue)) if d.ep else None
        core.check(l.ldetr_gemm_f32(d.A, d.lda, 0, d.B, d.ldb, 0, d.C, d.ldc, d.M, d.N, d.K, 0, ep, 0, core.stream()), 'gemm')
    elif p.kind == 'attention':
        core.check(l.ldetr_attention_fwd_group_f32(ctypes.byref(p.args), 1, core.stream()), 'attention_fwd')
    else:
        entry = getattr(l, 'ldetr_' + p.kind + '_group_f32')
        core.check(entry(ctypes.byref(p.args), 1, core.stream()), p.kind)


def _send(me):
    """`me` in the current mode: queued (record), or sent with the queue's head when that is the same kind of launch (pair)."""
    if MODE == 'record':
        _queue.append(me)
        return
    mate = _take(me.kind)
    if mate is None:
        STATS['alone'] += 1
        _send_alone(me)
        return
    l = core.lib()
    if me.kind == 'gemm':
        rc = l.ldetr_gemm_pair_fwd_f32(ctypes.byref(mate.args), ctypes.byref(me.args), core.stream())
    elif me.kind == 'attention':
        arr = (_lib.AttnArgs * 2)(mate.args, me.args)
        rc = l.ldetr_attention_fwd_group_f32(arr, 2, core.stream())
    else:
        arr = (type(me.args) * 2)(mate.args, me.args)
        rc = getattr(l, 'ldetr_' + me.kind + '_group_f32')(arr, 2, core.stream())
    if rc == 3:          # LDETR_ERR_UNSUPPORTED: nothing was launched
        STATS['split'] += 1
        _send_alone(mate)
        _send_alone(me)
        return
    core.check(rc, me.kind + ' (pair)')
    STATS['paired'] += 1


def gemm(d, out):
    """hip.core.gemm's launch of an NT problem (its core.gemm_desc, which holds the operands while it is queued) while a mode is set."""
    _send(_Pending('gemm', d, getattr(d, '_keep', None), outs=(out,)))


def attention(a, out, lse):
    """hip.attention's packed self-attention forward launch (its argument block, which holds the tensors) while a mode is set."""
    _send(_Pending('attention', a, a._keep, outs=(out, lse)))


def takes_block(what, args):
    return MODE is not None and what in _BLOCK_KINDS and len(args) == 1


def block(what, a):
    """hip.blocks.launch's one-problem launch of a token-block kernel while a mode is set (the builder left the block's tensors on `a._keep`)."""
    _send(_Pending(what, a, getattr(a, '_keep', None), outs=getattr(a, '_outs', ())))


def flush():
    """Send what is left of the queue, in order."""
    while _queue:
        STATS['alone'] += 1
        _send_alone(_queue.pop(0))


class mode(object):
    """with rider.mode('record' | 'pair'): ...  (leaving 'pair' sends the rest of the queue; an exception drops it)."""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        global MODE
        assert MODE is None, 'rider modes do not nest'
        MODE = self.m

    def __exit__(self, et, ev, tb):
        global MODE
        MODE = None
        if et is not None:
            del _queue[:]
        elif self.m == 'pair':
            flush()
        if et is not None or self.m == 'pair':
            _unwritten.clear()
        return False


def eligible(enc_a, enc_b, rows_a, rows_b, staged=False, higher_order=False, profiled=False):
    """Whether two encoder stacks (training.detr_transformer.TransformerEncoder) may run in lock-step: the same depth, width, heads and feed-forward
    size, no final norm, both on the same side of the fused feed-forward block's token limit, and a plain phase (no staged backward, no
    twice-differentiable regulariser pass, no per-launch profile).

    What recording rests on: between its first and its last queued launch the recorded stack issues NOTHING but queued launches that reads a queued
    launch's result.  The position-embedded encoder path keeps to that (training/detr_transformer.py: q / k are projected from the previous
    LayerNorm's second output (`qk_in`), so there is no `x + pos` add after the first layer's, whose operand is the stack's input; LayerNorm and GEMM
    outputs are contiguous, 16-byte aligned fp32, so `core.f32c` copies nothing; no final norm).  It is enforced, not only assumed: a library launch
    that is not queued raises in `core.stream()`, and the ATen reads on that path (`core.f32c` when it has to copy, the adds in hip/linear.py and in
    TransformerEncoder.forward2d) go through `check_ready`, which raises on a tensor a queued launch has yet to write."""
    if not ENABLED or staged or higher_order or profiled:
        return False
    la, lb = list(enc_a.layers), list(enc_b.layers)
    if len(la) != len(lb) or not la or enc_a.norm is not None or enc_b.norm is not None:
        return False
    from . import ffn as hffn
    for x, y in zip(la, lb):
        if (x.self_attn.embed_dim != y.self_attn.embed_dim or x.self_attn.num_heads != y.self_attn.num_heads
                or x.linear1.weight.shape != y.linear1.weight.shape or x.self_attn.embed_dim // x.self_attn.num_heads != 32):
            return False
    return (rows_a <= hffn.MAX_ROWS) == (rows_b <= hffn.MAX_ROWS)


core._rider = sys.modules[__name__]      # hip.core.gemm asks it while a mode is set
