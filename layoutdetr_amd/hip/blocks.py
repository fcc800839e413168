"""The argument blocks of the token-block kernels (csrc/{layernorm,ffn_fused,mha_small}.hip; include/ldetr_hip.h: ldetr_ln_args, ldetr_ffn_args,
ldetr_mha_small_args, ldetr_mha_cross_args) -- the ONE place that assigns their fields and calls their entry points.  A builder fills the fields
of one direction of one problem from tensors (the other direction's stay zero); `launch` sends one or two problems as one launch.
hip.layernorm / hip.ffn (one sub-block per autograd node) and hip.stacks (a whole stack per node) drive the same kernels through it."""
import math

from .. import _lib
from . import core, rider

D_MODEL, N_HEAD = 256, 8
SCALE = 1.0 / math.sqrt(D_MODEL // N_HEAD)      # the attention sub-blocks are built for d_model 256 with 8 heads

# what (also the prefix of an error message) -> (C entry, takes a problem count): the group entries are (blocks, n, stream), the cross-attention
# ones (block, stream)
_ENTRIES = {'layernorm_fwd': ('ldetr_layernorm_fwd_group_f32', True), 'layernorm_bwd': ('ldetr_layernorm_bwd_group_f32', True),
            'ffn_fwd': ('ldetr_ffn_fwd_group_f32', True), 'ffn_bwd': ('ldetr_ffn_bwd_group_f32', True),
            'mha_small_fwd': ('ldetr_mha_small_fwd_group_f32', True), 'mha_small_bwd': ('ldetr_mha_small_bwd_group_f32', True),
            'mha_cross_fwd': ('ldetr_mha_cross_fwd_f32', False), 'mha_cross_bwd': ('ldetr_mha_cross_bwd_f32', False)}


def launch(what, args, flops=0.0, nbytes=0.0):
    """One launch of 1-2 problems (`args`: argument blocks of one builder); flops > 0: a contraction launch, accounted with the engine's
    (bench.py roofline leg, hip.core.engine_call)."""
    entry, grouped = _ENTRIES[what]
    if rider.takes_block(what, args):      # an encoder stack in lock-step with another one: queued, or sent with the other's launch
        return rider.block(what, args[0])
    fn = getattr(core.lib(), entry)
    n = len(args)
    arr = (type(args[0]) * n)(*args)
    if grouped:
        call = lambda: core.check(fn(arr, n, core.stream()), what)
    else:
        assert n == 1
        call = lambda: core.check(fn(arr, core.stream()), what)
    if flops > 0:
        core.engine_call('ldetr_token_stack', flops, call, nbytes=nbytes)
    else:
        call()


def draw_seed(p_drop):
    """The host half of a launch's dropout seed: drawn only where something is dropped (the order of the draws is part of the results)."""
    return core.next_seed() if p_drop > 0 else 0


def _set_dropout(a, p_drop, seed):
    """The device half (hip.core.iter_seed, redrawn per iteration) is passed as a pointer only when p_drop > 0."""
    a.p_drop, a.seed, a.seed_ptr = p_drop, seed, (core.iter_seed().data_ptr() if p_drop > 0 else None)


def _p(t):
    return t.data_ptr() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, r, gamma, beta, eps, p_drop, seed, y, z, mean, rstd, r_parts=0, r_bias=None, pos=None, ypos=None):
    """y = LN(z), z = x + dropout(r).  r None: plain LayerNorm (no dropout).  r_parts > 0: r [r_parts, M, D] is a sum still to be formed,
    r_bias + sum_s r[s], added in slice order inside the launch.  pos [pos_rows, D] with ypos: second output y + pos[row % pos_rows]."""
    a = _lib.LnArgs()
    M, D = x.shape
    a.x, a.r, a.gamma, a.beta, a.y, a.z, a.mean, a.rstd = x.data_ptr(), _p(r), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _p(z), mean.data_ptr(), rstd.data_ptr()
    a.rows, a.D, a.eps = M, D, eps
    if r is not None:
        _set_dropout(a, p_drop, seed)
    a.r_parts, a.r_part_stride = r_parts, M * D
    a.r_bias = _p(r_bias) if r_parts > 0 else None
    if pos is not None:
        a.pos, a.pos_rows, a.ypos = pos.data_ptr(), pos.shape[0], ypos.data_ptr()
    if rider.MODE == 'record':
        a._keep = (x, r, gamma, beta, y, z, mean, rstd, r_bias, pos, ypos)      # a queued launch keeps its tensors alive
        a._outs = (y, z, mean, rstd, ypos)
    return a


def ln_bwd(dy, z, mean, rstd, gamma, dx, dr, dgamma, dbeta, p_drop, seed, dy2=None, parts=None, n_parts=0):
    """Incoming gradient = dy (+ dy2) + the sum of n_parts slices parts[s][M][D] -> dx (gradient of z), dr = dx * dropout mask (optional),
    dgamma / dbeta += (optional, atomics)."""
    a = _lib.LnArgs()
    M, D = z.shape
    a.dy, a.z, a.mean, a.rstd, a.gamma, a.dx = dy.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr()
    a.dy2, a.dr, a.dgamma, a.dbeta = _p(dy2), _p(dr), _p(dgamma), _p(dbeta)
    a.dy_parts = parts.data_ptr() if n_parts else None
    a.dy_nparts, a.dy_part_stride = n_parts, M * D
    a.rows, a.D = M, D
    _set_dropout(a, p_drop, seed)
    return a


# ---------------------------------------------------------------------------------------------------------------- fused feed-forward block
def ffn_fwd(x, w1, b1, w2, h, ypart, p_drop, seed):
    """x [M, 256] -> h [M, F] (hidden after relu + dropout) and ypart [F/64, M, 256] (per-hidden-slice outputs without linear2's bias)."""
    a = _lib.FfnArgs()
    a.x, a.ldx, a.w1, a.b1, a.w2, a.h, a.ypart = x.data_ptr(), x.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), h.data_ptr(), ypart.data_ptr()
    a.M, a.F = h.shape
    _set_dropout(a, p_drop, seed)
    if rider.MODE == 'record':
        a._keep = (x, w1, b1, w2, h, ypart)
        a._outs = (h, ypart)
    return a


def ffn_bwd(dy, x, h, w1, w2, dxpart, dh, p_drop):
    """dy [M, 256] -> dxpart [F/64, M, 256] (per-hidden-slice input gradients) and dh [M, F] (optional: operand of the weight gradients).
    The dropout mask is read off the saved hidden activation, so no seed."""
    a = _lib.FfnArgs()
    a.dy, a.x, a.ldx, a.h, a.w1, a.w2, a.dxpart, a.dh = dy.data_ptr(), x.data_ptr(), x.stride(0), h.data_ptr(), w1.data_ptr(), w2.data_ptr(), dxpart.data_ptr(), _p(dh)
    a.M, a.F = h.shape
    a.p_drop = p_drop
    return a


# ---------------------------------------------------------------------------------------------------------------- attention sub-blocks
def mha_small_fwd(x, w_in, b_in, w_out, kpm, qkv, o, lse, ypart, B, L, p_drop, seed):
    """Self-attention sub-block: x [B*L, 256] -> qkv, o, lse (kept for the backward) and ypart [8, B*L, 256] (per-head outputs without
    out_proj's bias)."""
    a = _lib.MhaSmallArgs()
    a.x, a.ldx, a.w_in, a.b_in, a.w_out, a.kpm = x.data_ptr(), x.stride(0), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), _p(kpm)
    a.qkv, a.o, a.lse, a.ypart, a.B, a.L, a.scale = qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), ypart.data_ptr(), B, L, SCALE
    _set_dropout(a, p_drop, seed)
    return a


def mha_small_bwd(dr, w_in, w_out, kpm, qkv, o, lse, dqkv, dxpart, B, L, p_drop, seed):
    """dr [B*L, 256] -> dxpart [8, B*L, 256] (per-head input gradients) and dqkv [B*L, 768] (optional: operand of in_proj's weight gradient)."""
    a = _lib.MhaSmallArgs()
    a.w_in, a.w_out, a.kpm, a.qkv, a.o, a.lse = w_in.data_ptr(), w_out.data_ptr(), _p(kpm), qkv.data_ptr(), o.data_ptr(), lse.data_ptr()
    a.dr, a.dqkv, a.dxpart, a.B, a.L, a.scale = dr.data_ptr(), _p(dqkv), dxpart.data_ptr(), B, L, SCALE
    _set_dropout(a, p_drop, seed)
    return a


def mha_cross_fwd(x, w_q, b_q, k, v, w_out, kpm, q, o, lse, ypart, B, Lq, Lk, p_drop, seed):
    """Cross-attention sub-block onto projected memory k, v [B*Lk, pitch]: x [B*Lq, 256] -> q, o, lse (kept for the backward) and
    ypart [8, B*Lq, 256]."""
    a = _lib.MhaCrossArgs()
    a.x, a.ldx, a.w_q, a.b_q, a.w_out, a.kpm = x.data_ptr(), x.stride(0), w_q.data_ptr(), b_q.data_ptr(), w_out.data_ptr(), _p(kpm)
    a.k, a.ldk, a.v, a.ldv = k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0)
    a.q, a.o, a.lse, a.ypart, a.B, a.Lq, a.Lk, a.scale = q.data_ptr(), o.data_ptr(), lse.data_ptr(), ypart.data_ptr(), B, Lq, Lk, SCALE
    _set_dropout(a, p_drop, seed)
    return a


def mha_cross_bwd(dr, w_q, k, v, w_out, kpm, q, o, lse, dq, dk, dv, dxpart, B, Lq, Lk, p_drop, seed):
    """dr [B*Lq, 256] -> dq [B*Lq, 256], dk / dv (views into the grouped projection's gradient buffers) and dxpart [8, B*Lq, 256]."""
    a = _lib.MhaCrossArgs()
    a.w_q, a.w_out, a.kpm, a.q, a.o, a.lse = w_q.data_ptr(), w_out.data_ptr(), _p(kpm), q.data_ptr(), o.data_ptr(), lse.data_ptr()
    a.k, a.ldk, a.v, a.ldv = k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0)
    a.dr, a.dq, a.dk, a.lddk, a.dv, a.lddv, a.dxpart = dr.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0), dxpart.data_ptr()
    a.B, a.Lq, a.Lk, a.scale = B, Lq, Lk, SCALE
    _set_dropout(a, p_drop, seed)
    return a
