"""The short token stacks of LayoutDETR -- G's / D's layout decoders (training/detr_transformer.py:265-286 x 6, 9-10 queries per sample), D's
unconditional encoder and D's two reconstruction decoders (nn.TransformerEncoderLayer x 6: training/util.py:13-43, networks_detr.py:242-243, 269,
275-276) -- as ONE autograd node per group of up to two independent stacks.

Why a node per GROUP of STACKS and not per sub-block (rounds 3-4: hip.attention._SelfAttnPartsFn / _CrossAttnPartsFn, hip.ffn._LnFfnLnFn):
  * every launch of such a stack is a fraction of a wave of work per CU, so two stacks that do not depend on each other (D's conditional and
    unconditional reconstruction decoders; D's layout decoder and its unconditional encoder) advance in lock-step with ONE launch per sub-block step:
    the second problem's blocks follow the first's in the same grid (csrc/{mha_small,ffn_fused,layernorm}.hip take one or two argument blocks);
  * inside the node gradients travel between sub-blocks as PARTIAL SUMS: the one-launch attention backward (hip.blocks:
    mha_small_bwd / mha_cross_bwd: output-projection data gradient + attention backward + input-projection data gradient, three launches of the unfused
    path) leaves one input-gradient slice per head, which the LayerNorm backward in front adds in head order while it loads its incoming gradient --
    autograd would need a materialised tensor (one more launch) at every node boundary;
  * the weight gradients of a layer (feed-forward W1 / W2, attention in_proj / out_proj: independent contractions over the tokens) are ONE launch
    (ldetr_wgrad_multi_f32) instead of three paired ones.
Per layer: forward 4 launches (decoder: 6), backward 5 (decoder: 7) -- for one stack or for two.  No atomics on the activation path: forward values and
input gradients are bit-reproducible and identical whether a stack runs alone or in a group.

How the node reads: _TokenStacksFn.forward / .backward are the launch sequence; every sub-block step is a function below them over three small
records -- _Stack (one per stack), _Saved (what a layer's forward keeps for its backward), _Scratch (a layer's backward buffers) -- and the layer's
parameters by name (_LayerParams, order: LAYOUT).  The argument blocks themselves are hip.blocks'.
"""
from operator import attrgetter

import torch

from .. import _lib
from . import blocks, core
from .blocks import D_MODEL, N_HEAD

MAX_TOKENS, MAX_ROWS, MAX_CROSS_KEYS = 16, 512, 64
ENABLED = core.knob('TOKEN_STACKS', 1) != 0    # 0: every sub-block as its own autograd node on the generic kernels (A/B and equivalence tests)

NODE_RUNS = [0]   # how many stack nodes ran (tests assert that a stack took this path)

# The order of a layer's parameters among the node's inputs: (name inside the node, attribute of the layer module).  norm_a / norm_b are the two
# LayerNorms of the tail (encoder layer: norm1 / norm2 with dropout1 / dropout2; decoder layer: norm2 / norm3 with dropout2 / dropout3).
_SELF = (('sa_w_in', 'self_attn.in_proj_weight'), ('sa_b_in', 'self_attn.in_proj_bias'), ('sa_w_out', 'self_attn.out_proj.weight'), ('sa_b_out', 'self_attn.out_proj.bias'))
_CROSS = (('n1_g', 'norm1.weight'), ('n1_b', 'norm1.bias'),
          ('ca_w_in', 'multihead_attn.in_proj_weight'), ('ca_b_in', 'multihead_attn.in_proj_bias'), ('ca_w_out', 'multihead_attn.out_proj.weight'), ('ca_b_out', 'multihead_attn.out_proj.bias'))


def _tail(norm_a, norm_b):
    return (('na_g', norm_a + '.weight'), ('na_b', norm_a + '.bias'), ('w1', 'linear1.weight'), ('b1', 'linear1.bias'), ('w2', 'linear2.weight'), ('b2', 'linear2.bias'),
            ('nb_g', norm_b + '.weight'), ('nb_b', norm_b + '.bias'))


LAYOUT = {'enc': _SELF + _tail('norm1', 'norm2'), 'dec': _SELF + _CROSS + _tail('norm2', 'norm3')}
_OFFSET = {kind: {name: j for j, (name, _) in enumerate(fields)} for kind, fields in LAYOUT.items()}
_TAIL_MODULES = {'enc': ('norm1', 'dropout1', 'norm2', 'dropout2'), 'dec': ('norm2', 'dropout2', 'norm3', 'dropout3')}     # norm_a, drop_a, norm_b, drop_b
ENC_PARAMS, DEC_PARAMS = len(LAYOUT['enc']), len(LAYOUT['dec'])     # 12, 18


class Prog(object):
    """One stack: `layers` (TransformerEncoderLayer / TransformerDecoderLayer modules) applied to x [B*L, 256] (row = b * L + l).
    kind 'enc': x = norm1(x + SA(x)); x = norm2(x + FFN(x)).   kind 'dec': ... + cross-attention onto the projected memory kvs[i] = (K_i, V_i, grad_dst_i)
    (hip.attention.grouped_kv) of S tokens per sample between the two.  kpm / mem_kpm: uint8 key-padding masks [B, L] / [B, S] or None."""

    def __init__(self, kind, layers, x, B, L, kpm, training, final_norm=None, kvs=None, S=0, mem_kpm=None):
        self.kind, self.layers, self.x, self.B, self.L, self.kpm, self.training = kind, list(layers), x, B, L, kpm, training
        self.final_norm, self.kvs, self.S, self.mem_kpm = final_norm, kvs, S, mem_kpm


def layer_params(kind, layer):
    return [attrgetter(path)(layer) for _, path in LAYOUT[kind]]


def usable(prog):
    """d_model 256 with 8 heads, at most 16 tokens per sample and 512 rows, hidden width a multiple of 64, fp32 rows the kernels can address."""
    x = prog.x
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == D_MODEL and 1 <= prog.L <= MAX_TOKENS and x.shape[0] == prog.B * prog.L
            and x.shape[0] <= MAX_ROWS and len(prog.layers) >= 1):
        return False
    for l in prog.layers:
        sa = l.self_attn
        if sa.num_heads != N_HEAD or sa.in_proj_weight.shape[1] != D_MODEL or l.linear1.weight.shape[0] % 64 != 0 or l.linear1.bias is None or l.linear2.bias is None:
            return False
        if sa.in_proj_bias is None or sa.out_proj.bias is None:        # the group kernels read both unconditionally (nn.MultiheadAttention(bias=False) takes the generic path)
            return False
        if prog.kind == 'dec' and (l.multihead_attn.num_heads != N_HEAD or l.multihead_attn.in_proj_bias is None or l.multihead_attn.out_proj.bias is None):
            return False
    if prog.kind == 'dec' and (prog.kvs is None or len(prog.kvs) != len(prog.layers)):
        return False
    return True


def _new(dev, *shape):
    return torch.empty(shape, device=dev, dtype=torch.float32)


def _rows(t):
    """fp32 rows the kernels address directly (unit inner stride, 16-byte aligned rows); anything else is copied once."""
    if t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and t.stride(0) >= t.shape[1]:
        return t
    return core.f32c(t)


def _fl_self(pr, bwd=False):
    """algorithmic FLOPs / bytes of the self-attention sub-block of one stack (projection, QK^T + PV, output projection; backward: their
    data gradients incl. the recomputed scores)."""
    M, D, att = pr.B * pr.L, D_MODEL, pr.B * N_HEAD * 2.0 * pr.L * pr.L * (D_MODEL // N_HEAD)
    fl = 2.0 * M * D * 3 * D + 2.0 * M * D * D + (5 if bwd else 2) * att
    return fl, 4.0 * (M * D * (6 if bwd else 5) + 4 * D * D + N_HEAD * M * D)


def _fl_cross(pr, bwd=False):
    M, D, att = pr.B * pr.L, D_MODEL, pr.B * N_HEAD * 2.0 * pr.L * pr.S * (D_MODEL // N_HEAD)
    fl = 2.0 * M * D * D * 2 + (5 if bwd else 2) * att
    return fl, 4.0 * (M * D * 4 + 2 * D * D + (4 if bwd else 2) * pr.B * pr.S * D + N_HEAD * M * D)


def _fl_ffn(M, F):
    return 4.0 * M * D_MODEL * F, 4.0 * (2 * D_MODEL * F + M * F + (F // 64 + 1) * M * D_MODEL)


def _launch_sum(what, args, costs):
    """One contraction launch of the group; costs: (FLOPs, bytes) per problem."""
    blocks.launch(what, args, sum(f for f, _ in costs), sum(b for _, b in costs))


# ---------------------------------------------------------------------------------------------------------------- the node's records
class _LayerParams(object):
    """One layer's parameters by name (LAYOUT): fp32 contiguous, detached; index(name): the parameter's place among the node's inputs."""

    def __init__(self, kind, tensors, base):
        self.kind, self.base = kind, base
        for j, (name, _) in enumerate(LAYOUT[kind]):
            setattr(self, name, core.f32c(tensors[base + j].detach()))

    def index(self, name):
        return self.base + _OFFSET[self.kind][name]


class _Stack(object):
    """One stack inside the node.  Kept for the backward: prog, M, dev, x_index, params (one _LayerParams per layer), final (the final norm's
    [weight, bias]) / final_index, K / V / kv_index, saved (one _Saved per layer), final_saved.  Forward only: cur (the running activation) and res
    (the open residual branch: (tensor or slices, bias, number of slices) that the next LayerNorm launch closes), keep (buffers held until their
    consumers are queued).  Backward only: need_w, g (the
    gradient of the running activation: _Grad), t (the layer's _Scratch)."""
    __slots__ = ('prog', 'M', 'dev', 'x_index', 'params', 'final', 'final_index', 'K', 'V', 'kv_index', 'saved', 'final_saved', 'cur', 'res', 'keep', 'need_w', 'g', 't')

    def __init__(self, prog, x, x_index):
        self.prog, self.M, self.dev, self.x_index, self.cur = prog, prog.B * prog.L, x.device, x_index, _rows(x)
        self.params, self.saved = [], []
        self.final = self.final_index = self.K = self.V = self.kv_index = self.final_saved = self.res = self.keep = self.need_w = self.g = self.t = None


class _Saved(object):
    """What one layer's forward keeps for its backward.  Self-attention: x (sub-block input), qkv, o, lse, p_att / seed_att.  Decoder: z1, mean1,
    rstd1, t1 (norm1 and its output), p1 / seed1; qc, oc, lse_c, p_c / seed_c, cross_small (cross-attention).  Tail: x1 (norm_a's output), za, mean_a,
    rstd_a, h (hidden activation, F wide), zb, mean_b, rstd_b and the three dropouts p_a / seed_a, p_h / seed_h, p_b / seed_b."""
    __slots__ = ('x', 'qkv', 'o', 'lse', 'p_att', 'seed_att', 'p1', 'seed1', 'z1', 'mean1', 'rstd1', 't1', 'p_c', 'seed_c', 'qc', 'oc', 'lse_c', 'cross_small',
                 'p_a', 'seed_a', 'p_h', 'seed_h', 'p_b', 'seed_b', 'F', 'x1', 'za', 'mean_a', 'rstd_a', 'h', 'zb', 'mean_b', 'rstd_b')


class _Scratch(object):
    """One layer's backward buffers.  gin: the incoming gradient (kept alive until its consumers are queued); dz / dr: norm_b's input-sum and branch
    gradients; dxpart, dh: the feed-forward backward's; dsum / da: input-sum and branch gradients of the LayerNorm in front of the current sub-block
    (norm_a, then norm1 in a decoder); da_ca: norm_a's branch gradient once norm1's has taken `da`; dq, dk, dv: cross-attention; dqkv, dxpart_sa:
    self-attention."""
    __slots__ = ('gin', 'dz', 'dr', 'dxpart', 'dh', 'dsum', 'da', 'da_ca', 'dq', 'dk', 'dv', 'dqkv', 'dxpart_sa')


class _Grad(object):
    """A gradient inside the node: `res` [M, D] + the sum of `n` slices parts[s][M][D] (n = 0: res alone); dy2: one more full tensor (the
    generic cross-attention path's query-projection gradient)."""

    def __init__(self, res, parts=None, n=0, dy2=None):
        self.res, self.parts, self.n, self.dy2 = res, parts, n, dy2


def _unpack(progs, tensors):
    """tensors (the order run() packs them in) -> one _Stack per prog."""
    st, pos = [], 0
    for pr in progs:
        s = _Stack(pr, tensors[pos], pos); pos += 1
        for _ in pr.layers:
            s.params.append(_LayerParams(pr.kind, tensors, pos)); pos += len(LAYOUT[pr.kind])
        if pr.final_norm is not None:
            s.final, s.final_index = [core.f32c(t.detach()) for t in tensors[pos:pos + 2]], pos
            pos += 2
        if pr.kind == 'dec':
            n = len(pr.layers)
            s.K, s.V, s.kv_index = list(tensors[pos:pos + n]), list(tensors[pos + n:pos + 2 * n]), pos
            pos += 2 * n
        st.append(s)
    assert pos == len(tensors)
    return st


# ---------------------------------------------------------------------------------------------------------------- forward steps
def _fwd_self_attn(act, i):
    """Self-attention sub-block of every active stack: ONE launch.  Leaves the per-head contributions as the open residual branch."""
    H, D, args = N_HEAD, D_MODEL, []
    for s in act:
        pr, M, W, dev = s.prog, s.M, s.params[i], s.dev
        sv = _Saved()
        sv.p_att = pr.layers[i].self_attn.dropout if pr.training else 0.0
        sv.x, sv.qkv, sv.o, sv.lse, sv.seed_att = s.cur, _new(dev, M, 3 * D), _new(dev, M, D), _new(dev, pr.B * H * pr.L), blocks.draw_seed(sv.p_att)
        ypart = _new(dev, H, M, D)
        args.append(blocks.mha_small_fwd(sv.x, W.sa_w_in, W.sa_b_in, W.sa_w_out, pr.kpm, sv.qkv, sv.o, sv.lse, ypart, pr.B, pr.L, sv.p_att, sv.seed_att))
        s.res = (ypart, W.sa_b_out, H)
        s.saved.append(sv)
    _launch_sum('mha_small_fwd', args, [_fl_self(s.prog) for s in act])


def _fwd_norm1_cross(s, i):
    """Decoder: norm1 closes the self-attention branch, then the cross-attention sub-block onto the projected memory opens the next one."""
    H, D = N_HEAD, D_MODEL
    pr, M, W, sv, dev = s.prog, s.M, s.params[i], s.saved[i], s.dev
    layer = pr.layers[i]
    sv.p1 = layer.dropout1.p if pr.training else 0.0
    sv.seed1, sv.z1, sv.mean1, sv.rstd1, sv.t1 = blocks.draw_seed(sv.p1), _new(dev, M, D), _new(dev, M), _new(dev, M), _new(dev, M, D)
    r, r_bias, r_parts = s.res
    blocks.launch('layernorm_fwd', [blocks.ln_fwd(s.cur, r, W.n1_g, W.n1_b, layer.norm1.eps, sv.p1, sv.seed1, sv.t1, sv.z1, sv.mean1, sv.rstd1, r_parts=r_parts, r_bias=r_bias)])
    s.cur = sv.t1
    K, V = s.K[i], s.V[i]
    sv.p_c = layer.multihead_attn.dropout if pr.training else 0.0
    sv.seed_c, sv.qc, sv.oc, sv.lse_c = blocks.draw_seed(sv.p_c), _new(dev, M, D), _new(dev, M, D), _new(dev, pr.B * H * pr.L)
    Wq, Bq = W.ca_w_in[:D], W.ca_b_in[:D]
    sv.cross_small = (1 <= pr.S <= MAX_CROSS_KEYS and K.stride(1) == 1 and V.stride(1) == 1 and K.stride(0) % 4 == 0 and V.stride(0) % 4 == 0
                      and K.data_ptr() % 16 == 0 and V.data_ptr() % 16 == 0)
    if sv.cross_small:
        ypart = _new(dev, H, M, D)
        _launch_sum('mha_cross_fwd', [blocks.mha_cross_fwd(sv.t1, Wq, Bq, K, V, W.ca_w_out, pr.mem_kpm, sv.qc, sv.oc, sv.lse_c, ypart, pr.B, pr.L, pr.S, sv.p_c, sv.seed_c)],
                    [_fl_cross(pr)])
        s.res = (ypart, W.ca_b_out, H)
    else:
        # more than 64 memory tokens (backgrounds above 256 x 256): projection, attention kernel, projection
        lib = core.lib()
        core.gemm(sv.t1, Wq, 0, 0, M, D, D, out=sv.qc, ep=core.epilogue(col_bias=Bq))
        core.check(lib.ldetr_attention_fwd_f32(
            core.ptr(sv.qc), D, core.ptr(K), K.stride(0), core.ptr(V), V.stride(0), core.ptr(pr.mem_kpm), core.ptr(sv.oc), D, core.ptr(sv.lse_c),
            pr.B, H, pr.L, pr.S, D // H, blocks.SCALE, sv.p_c, sv.seed_c, core.seed_ptr() if sv.p_c > 0 else None, 0, core.stream()), 'attention_fwd')
        s.res = (core.gemm(sv.oc, W.ca_w_out, 0, 0, M, D, D, ep=core.epilogue(col_bias=W.ca_b_out)), None, 0)


def _fwd_tail(act, i):
    """Tail of every active stack: norm_a(x + drop(open branch)), feed-forward, norm_b: three launches."""
    D, ln_a, ffn, ln_b = D_MODEL, [], [], []
    for s in act:
        pr, M, W, sv, dev = s.prog, s.M, s.params[i], s.saved[i], s.dev
        layer = pr.layers[i]
        norm_a, drop_a, norm_b, drop_b = [getattr(layer, m) for m in _TAIL_MODULES[pr.kind]]
        sv.p_a, sv.p_h, sv.p_b = (drop_a.p, layer.dropout.p, drop_b.p) if pr.training else (0.0, 0.0, 0.0)
        sv.seed_a, sv.seed_h, sv.seed_b = blocks.draw_seed(sv.p_a), blocks.draw_seed(sv.p_h), blocks.draw_seed(sv.p_b)
        sv.F = W.w1.shape[0]
        ns = sv.F // 64
        sv.x1, sv.za, sv.mean_a, sv.rstd_a, sv.h = _new(dev, M, D), _new(dev, M, D), _new(dev, M), _new(dev, M), _new(dev, M, sv.F)
        sv.zb, sv.mean_b, sv.rstd_b = _new(dev, M, D), _new(dev, M), _new(dev, M)
        parts, y = _new(dev, ns, M, D), _new(dev, M, D)
        r, r_bias, r_parts = s.res
        ln_a.append(blocks.ln_fwd(s.cur, r, W.na_g, W.na_b, norm_a.eps, sv.p_a, sv.seed_a, sv.x1, sv.za, sv.mean_a, sv.rstd_a, r_parts=r_parts, r_bias=r_bias))
        ffn.append(blocks.ffn_fwd(sv.x1, W.w1, W.b1, W.w2, sv.h, parts, sv.p_h, sv.seed_h))
        ln_b.append(blocks.ln_fwd(sv.x1, parts, W.nb_g, W.nb_b, norm_b.eps, sv.p_b, sv.seed_b, y, sv.zb, sv.mean_b, sv.rstd_b, r_parts=ns, r_bias=W.b2))
        s.keep = (r, parts)      # (alive until their consumers have been queued: same stream, so queue order is enough)
        s.cur, s.res = y, None
    blocks.launch('layernorm_fwd', ln_a)
    _launch_sum('ffn_fwd', ffn, [_fl_ffn(s.M, s.saved[i].F) for s in act])
    blocks.launch('layernorm_fwd', ln_b)


def _fwd_final_norm(s):
    """The stack's closing LayerNorm (no residual: its input doubles as the saved pre-norm sum)."""
    M, dev = s.M, s.dev
    z, mean, rstd, y = s.cur, _new(dev, M), _new(dev, M), _new(dev, M, D_MODEL)
    blocks.launch('layernorm_fwd', [blocks.ln_fwd(z, None, s.final[0], s.final[1], s.prog.final_norm.eps, 0.0, 0, y, z, mean, rstd)])
    s.final_saved, s.cur = (z, mean, rstd), y


# ---------------------------------------------------------------------------------------------------------------- backward steps
class _Backward(object):
    """What the backward steps share: the node's inputs and which of them need a gradient, the gradients returned to autograd (index 0: progs), and
    the accumulation targets of the parameters."""

    def __init__(self, ctx):
        self.tensors, self.need = ctx.params, ctx.needs_input_grad
        self.grads = [None] * (1 + len(self.tensors))
        self.wg_off = core.WEIGHT_GRADIENTS_DISABLED[0]
        self.temps = {}

    def target(self, idx):
        """Accumulation target of parameter tensors[idx]: its flat .grad view (the kernels add in place, autograd gets None) or a zero-filled
        temporary returned to autograd."""
        fg = core.flat_grad(self.tensors[idx])
        if fg is not None and fg.is_contiguous():
            return fg
        if idx not in self.temps:
            self.temps[idx] = torch.zeros_like(self.tensors[idx], memory_format=torch.contiguous_format)
            self.grads[1 + idx] = self.temps[idx]
        return self.temps[idx]

    def norm_targets(self, W, gamma, beta, wanted):
        """-> (dgamma, dbeta) targets of a layer's LayerNorm, or (None, None) when its weights do not train."""
        return (self.target(W.index(gamma)), self.target(W.index(beta))) if wanted else (None, None)


def _bwd_enter(s, dy, bw):
    """The stack's output gradient enters the node, through the final norm's backward if there is one."""
    pr, M, dev = s.prog, s.M, s.dev
    npar = len(LAYOUT[pr.kind])
    s.need_w = (not bw.wg_off) and any(bw.need[1 + j] for W in s.params for j in range(W.base, W.base + npar))
    g = _Grad(_rows(dy.reshape(M, D_MODEL)))
    if pr.final_norm is not None:
        z, mean, rstd = s.final_saved
        dx = _new(dev, M, D_MODEL)
        want = (not bw.wg_off) and (bw.need[1 + s.final_index] or bw.need[2 + s.final_index])
        dgamma, dbeta = (bw.target(s.final_index), bw.target(s.final_index + 1)) if want else (None, None)
        blocks.launch('layernorm_bwd', [blocks.ln_bwd(g.res, z, mean, rstd, s.final[0], dx, None, dgamma, dbeta, 0.0, 0)])
        g = _Grad(dx)
    s.g = g


def _bwd_tail(act, i, bw):
    """Tail backward of every active stack: norm_b, feed-forward, norm_a: three launches."""
    D, ln_b, ffn, ln_a = D_MODEL, [], [], []
    for s in act:
        sv, M, W, dev, g = s.saved[i], s.M, s.params[i], s.dev, s.g
        ns = sv.F // 64
        t = s.t = _Scratch()
        t.gin = g
        t.dz = _new(dev, M, D)
        t.dr = _new(dev, M, D) if sv.p_b > 0 else t.dz
        dgamma, dbeta = bw.norm_targets(W, 'nb_g', 'nb_b', s.need_w)
        ln_b.append(blocks.ln_bwd(g.res, sv.zb, sv.mean_b, sv.rstd_b, W.nb_g, t.dz, t.dr if sv.p_b > 0 else None, dgamma, dbeta, sv.p_b, sv.seed_b,
                                  dy2=g.dy2, parts=g.parts, n_parts=g.n))
        t.dxpart, t.dh = _new(dev, ns, M, D), (_new(dev, M, sv.F) if s.need_w else None)
        ffn.append(blocks.ffn_bwd(t.dr, sv.x1, sv.h, W.w1, W.w2, t.dxpart, t.dh, sv.p_h))
        t.dsum = _new(dev, M, D)
        t.da = _new(dev, M, D) if sv.p_a > 0 else t.dsum
        dgamma, dbeta = bw.norm_targets(W, 'na_g', 'na_b', s.need_w)
        ln_a.append(blocks.ln_bwd(t.dz, sv.za, sv.mean_a, sv.rstd_a, W.na_g, t.dsum, t.da if sv.p_a > 0 else None, dgamma, dbeta, sv.p_a, sv.seed_a,
                                  parts=t.dxpart, n_parts=ns))
    blocks.launch('layernorm_bwd', ln_b)
    _launch_sum('ffn_bwd', ffn, [_fl_ffn(s.M, s.saved[i].F) for s in act])
    blocks.launch('layernorm_bwd', ln_a)


def _bwd_cross_norm1(s, i, bw):
    """Decoder: cross-attention backward, then norm1's.  Afterwards t.dsum / t.da are norm1's (what the self-attention backward continues from)
    and t.da_ca is the cross-attention sub-block's output gradient (operand of its out_proj weight gradient)."""
    H, D = N_HEAD, D_MODEL
    pr, sv, M, W, t, dev = s.prog, s.saved[i], s.M, s.params[i], s.t, s.dev
    K, V = s.K[i], s.V[i]
    dk, dv = pr.kvs[i][2]()            # views into the grouped projection's gradient buffers (hip.attention.grouped_kv)
    Wq = W.ca_w_in[:D]
    dq = _new(dev, M, D)
    if sv.cross_small:
        dxpart_c = _new(dev, H, M, D)
        _launch_sum('mha_cross_bwd', [blocks.mha_cross_bwd(t.da, Wq, K, V, W.ca_w_out, pr.mem_kpm, sv.qc, sv.oc, sv.lse_c, dq, dk, dv, dxpart_c, pr.B, pr.L, pr.S, sv.p_c, sv.seed_c)],
                    [_fl_cross(pr, bwd=True)])
        g1 = _Grad(t.dsum, dxpart_c, H)
    else:
        d_o = core.gemm(t.da, W.ca_w_out, 0, 1, M, D, D)
        core.check(core.lib().ldetr_attention_bwd_f32(
            core.ptr(sv.qc), D, core.ptr(K), K.stride(0), core.ptr(V), V.stride(0), core.ptr(pr.mem_kpm), core.ptr(sv.oc), D, core.ptr(sv.lse_c),
            core.ptr(d_o), D, core.ptr(dq), D, core.ptr(dk), dk.stride(0), core.ptr(dv), dv.stride(0), pr.B, H, pr.L, pr.S, D // H, blocks.SCALE, sv.p_c, sv.seed_c,
            core.seed_ptr() if sv.p_c > 0 else None, 0, core.stream()), 'attention_bwd')
        g1 = _Grad(t.dsum, dy2=core.gemm(dq, Wq, 0, 1, M, D, D))
    t.dq, t.dk, t.dv = dq, dk, dv
    i_k, i_v = 1 + s.kv_index + i, 1 + s.kv_index + len(pr.layers) + i
    if bw.need[i_k]:
        bw.grads[i_k] = dk
    if bw.need[i_v]:
        bw.grads[i_v] = dv
    dsum1 = _new(dev, M, D)
    da1 = _new(dev, M, D) if sv.p1 > 0 else dsum1
    dgamma, dbeta = bw.norm_targets(W, 'n1_g', 'n1_b', s.need_w)
    blocks.launch('layernorm_bwd', [blocks.ln_bwd(g1.res, sv.z1, sv.mean1, sv.rstd1, W.n1_g, dsum1, da1 if sv.p1 > 0 else None, dgamma, dbeta, sv.p1, sv.seed1,
                                                   dy2=g1.dy2, parts=g1.parts, n_parts=g1.n)])
    t.da_ca, t.da, t.dsum = t.da, da1, dsum1


def _bwd_self_attn(act, i):
    """Self-attention backward of every active stack: ONE launch."""
    H, D, args = N_HEAD, D_MODEL, []
    for s in act:
        pr, sv, M, W, t, dev = s.prog, s.saved[i], s.M, s.params[i], s.t, s.dev
        t.dqkv = _new(dev, M, 3 * D) if s.need_w else None
        t.dxpart_sa = _new(dev, H, M, D)
        args.append(blocks.mha_small_bwd(t.da, W.sa_w_in, W.sa_w_out, pr.kpm, sv.qkv, sv.o, sv.lse, t.dqkv, t.dxpart_sa, pr.B, pr.L, sv.p_att, sv.seed_att))
    _launch_sum('mha_small_bwd', args, [_fl_self(s.prog, bwd=True) for s in act])


def _bwd_weights(act, i, bw):
    """Every weight gradient of the layer(s): contractions over the tokens, up to 8 per launch."""
    descs = []
    for s in act:
        if not s.need_w:
            continue
        sv, M, W, t = s.saved[i], s.M, s.params[i], s.t

        def desc(A, Bm, weight, bias, rows=None):
            d = _lib.WgradDesc()
            dW, db = bw.target(W.index(weight)), bw.target(W.index(bias))
            nrows = A.shape[1] if rows is None else rows
            d.A, d.lda, d.B, d.ldb, d.dW, d.ldw, d.db = A.data_ptr(), A.stride(0), Bm.data_ptr(), Bm.stride(0), dW.data_ptr(), dW.shape[1], db.data_ptr()
            d.M, d.rows, d.cols = M, nrows, Bm.shape[1]
            return d
        descs.append(desc(t.dr, sv.h, 'w2', 'b2'))                                   # dW2 += dr^T h, db2
        descs.append(desc(t.dh, sv.x1, 'w1', 'b1'))                                  # dW1 += dh^T x1, db1
        descs.append(desc(t.da, sv.o, 'sa_w_out', 'sa_b_out'))                       # self-attention out_proj
        descs.append(desc(t.dqkv, sv.x, 'sa_w_in', 'sa_b_in'))                       # self-attention in_proj (packed q | k | v)
        if s.prog.kind == 'dec':
            descs.append(desc(t.da_ca, sv.oc, 'ca_w_out', 'ca_b_out'))               # cross-attention out_proj
            descs.append(desc(t.dq, sv.t1, 'ca_w_in', 'ca_b_in', rows=D_MODEL))      # cross-attention query rows of in_proj (K / V rows: the grouped projection)
    lib = core.lib()
    for j in range(0, len(descs), 8):
        chunk = descs[j:j + 8]
        arr = (_lib.WgradDesc * len(chunk))(*chunk)
        wf = sum(2.0 * d.M * d.rows * d.cols for d in chunk)
        wb = sum(4.0 * (d.M * (d.rows + d.cols) + d.rows * d.cols) for d in chunk)
        core.engine_call('ldetr_token_stack', wf, lambda: core.check(lib.ldetr_wgrad_multi_f32(arr, len(chunk), core.stream()), 'wgrad_multi'), nbytes=wb)


def _bwd_leave(s, bw):
    """The stack's input gradient leaves the node as ONE tensor."""
    if bw.need[1 + s.x_index]:
        g, M = s.g, s.M
        dx = _new(s.dev, M, D_MODEL)
        core.check(core.lib().ldetr_sum_parts_f32(core.ptr(g.res), core.ptr(g.parts), g.n, M * D_MODEL, core.ptr(dx), M * D_MODEL, core.stream()), 'sum_parts')
        bw.grads[1 + s.x_index] = dx.reshape(bw.tensors[s.x_index].shape)


class _TokenStacksFn(torch.autograd.Function):
    """forward(progs, *tensors) -> one output [B*L, 256] per stack.  tensors = per stack: x, every layer's parameters (layer_params order), the final
    norm's (weight, bias) if any, then for 'dec' K_0..K_{n-1}, V_0..V_{n-1} of hip.attention.grouped_kv."""

    @staticmethod
    def forward(ctx, progs, *tensors):
        ctx.set_materialize_grads(False)
        core.require_gpu(*[t for t in tensors if t is not None])
        st = _unpack(progs, tensors)
        for i in range(max(len(s.prog.layers) for s in st)):
            act = [s for s in st if i < len(s.prog.layers)]
            _fwd_self_attn(act, i)
            for s in act:
                if s.prog.kind == 'dec':
                    _fwd_norm1_cross(s, i)
            _fwd_tail(act, i)
        outs = []
        for s in st:
            if s.prog.final_norm is not None:
                _fwd_final_norm(s)
            outs.append(s.cur)
            s.cur = s.res = s.keep = None        # forward-only state: the backward keeps what _Stack's docstring lists
        ctx.progs, ctx.params, ctx.state = progs, tensors, st
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        bw = _Backward(ctx)
        live = []
        for s, dy in zip(ctx.state, douts):
            if dy is not None:
                _bwd_enter(s, dy, bw)
                live.append(s)
        if not live:
            return tuple(bw.grads)
        for i in reversed(range(max(len(s.prog.layers) for s in live))):
            act = [s for s in live if i < len(s.prog.layers)]
            _bwd_tail(act, i, bw)
            for s in act:
                if s.prog.kind == 'dec':
                    _bwd_cross_norm1(s, i, bw)
            _bwd_self_attn(act, i)
            _bwd_weights(act, i, bw)
            for s in act:
                s.g, s.t = _Grad(s.t.dsum, s.t.dxpart_sa, N_HEAD), None
        for s in live:
            _bwd_leave(s, bw)
        return tuple(bw.grads)


def run(progs):
    """Run one or two independent stacks (Prog) in lock-step -> list of outputs [B*L, 256]."""
    NODE_RUNS[0] += 1
    tensors = []
    for pr in progs:
        tensors.append(pr.x)
        for layer in pr.layers:
            tensors += layer_params(pr.kind, layer)
        if pr.final_norm is not None:
            tensors += [pr.final_norm.weight, pr.final_norm.bias]
        if pr.kind == 'dec':
            tensors += [kv[0] for kv in pr.kvs] + [kv[1] for kv in pr.kvs]
    return list(_TokenStacksFn.apply(progs, *tensors))
