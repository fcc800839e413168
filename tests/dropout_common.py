"""What tests/test_dropout_ref_cpu.py and tests/test_dropout_parity_gpu.py share: the inputs of every train-mode parity case and its float64 torch
reference with explicit dropout masks (oracle/dropout_ref.py).  A reference takes the masks as tensors or through a `Masks` object, so the CPU file
can evaluate it with a deliberately wrong convention and the GPU file with the seeds the kernels were actually given."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detr_ref
from oracle import dropout_ref as DR

# tolerances: the project's own from the matching dropout-off tests (test_kernels_gpu.py), in rel_err's measure max|a - b| / max|b|
TOL_ATTN = dict(o=5e-6, grad=2e-5)            # test_attention
TOL_STACK = dict(y=2e-5, grad=5e-5)           # test_token_stack_node_vs_fp64_oracle
TOL_LN = dict(y=3e-6, grad=1e-5)              # test_layernorm
TOL_FFN = dict(y=5e-6, thresh=2e-5, share=0.03)   # test_ln_ffn_ln_fused_tail_vs_fp64_reference (close_up_to_relu_flips)
TOL_LINEAR = dict(y=3e-6, grad=5e-6)          # test_linear_autograd
# mha_forward block = K-256 projection GEMM -> attention core -> K-256 projection GEMM: the stages' own bounds add up to 3e-6 + 5e-6 + 3e-6 <= 2e-5 forward
# and 5e-6 + 2e-5 + 5e-6 <= 5e-5 backward, the figures the stacks (chains of such blocks) are held to
TOL_MHA = TOL_STACK


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def ragged_kpm(B, Lk):
    """Ragged key-padding mask that never masks a whole row: the tail third of sample 0 (when there is another sample) and every fifth key of the
    last sample from key 2 on -- so keys of every 16-key tile and every 256-key chunk stay visible."""
    kpm = torch.zeros(B, Lk, dtype=torch.bool)
    if B > 1:
        kpm[0, Lk - Lk // 3:] = True
    if Lk > 2:
        kpm[B - 1, 2::5] = True
    return kpm


class Masks(object):
    """Scale tensors (0 or 1 / (1 - p)) per dropout site from (host seed, device word, p), with switches for the WRONG conventions the CPU file shows
    the tolerances to reject: seed_shift (seed + 1), device word dropped, q / key swapped (square attention), b*H + h -> h*B + b."""

    def __init__(self, device_word, seed_shift=0, use_device_word=True, swap_qk=False, swap_bh=False):
        self.word, self.shift, self.use_word, self.swap_qk, self.swap_bh = int(device_word), seed_shift, use_device_word, swap_qk, swap_bh

    def seed(self, host_seed):
        return DR.total_seed(host_seed + self.shift, self.word if self.use_word else 0)

    def attention(self, host_seed, p, B, H, Lq, Lk):
        """[B, H, Lq, Lk]"""
        idx = DR.attention_index(B, H, Lq, Lk)
        if self.swap_qk and Lq == Lk:             # (a square site only: self-attention)
            idx = np.ascontiguousarray(idx.transpose(0, 1, 3, 2))
        if self.swap_bh:
            idx = np.ascontiguousarray(DR.attention_index(H, B, Lq, Lk).transpose(1, 0, 2, 3))
        return t64(DR.scale(self.seed(host_seed), idx, p))

    def rows(self, host_seed, p, rows, cols, ld=None):
        """[rows, cols]: LayerNorm residual (cols = D), feed-forward hidden (cols = F), GEMM epilogue (ld = ldc)."""
        return t64(DR.scale(self.seed(host_seed), DR.rows_index(rows, cols, ld), p))


# ---------------------------------------------------------------------------------------------------------------- attention core
def attention_inputs(B, H, Lq, Lk, dh):
    g = torch.Generator().manual_seed(9000 + 131 * B + 17 * H + 7 * Lq + 3 * Lk + dh)
    d = H * dh
    q, k, v = torch.randn(B * Lq, d, generator=g), torch.randn(B * Lk, d, generator=g), torch.randn(B * Lk, d, generator=g)
    go = torch.randn(B * Lq, d, generator=g)
    return q, k, v, go, ragged_kpm(B, Lk)


def attention_ref(q, k, v, go, kpm, B, H, Lq, Lk, dh, mask, causal=False):
    """fp64: o = (softmax(q k^T / sqrt(dh) + key mask) * mask) v -> (o, dq, dk, dv); mask [B, H, Lq, Lk] or None."""
    qr, kr, vr = [t.double().clone().requires_grad_(True) for t in (q, k, v)]

    def heads(t, L):
        return t.view(B, L, H, dh).permute(0, 2, 1, 3)
    s = heads(qr, Lq) @ heads(kr, Lk).transpose(-1, -2) / math.sqrt(dh)
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float('-inf'))
    if causal:
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float('-inf'))
    p = s.softmax(-1)
    if mask is not None:
        p = p * mask
    o = (p @ heads(vr, Lk)).permute(0, 2, 1, 3).reshape(B * Lq, H * dh)
    o.backward(go.double())
    return o.detach(), qr.grad, kr.grad, vr.grad


# ---------------------------------------------------------------------------------------------------------------- token stacks
STACK_P = dict(attn=0.15, cross=0.25, res1=0.1, res2=0.2, res3=0.3, hidden=0.35)      # a different p at every site of a layer
SEED_ORDER = {'enc': ('attn', 'res1', 'hidden', 'res2'), 'dec': ('attn', 'res1', 'cross', 'res2', 'hidden', 'res3')}     # a lone stack's draws per layer


def set_stack_p(mod, kind):
    """The module's dropout probabilities site by site (STACK_P): hip.stacks reads them off the layer modules."""
    for layer in mod.layers:
        layer.self_attn.dropout = STACK_P['attn']
        layer.dropout1.p, layer.dropout2.p, layer.dropout.p = STACK_P['res1'], STACK_P['res2'], STACK_P['hidden']
        if kind == 'dec':
            layer.multihead_attn.dropout, layer.dropout3.p = STACK_P['cross'], STACK_P['res3']


def stack_module(kind):
    from layoutdetr_amd.training import detr_transformer as T
    d, H = 256, 8
    torch.manual_seed(317)                        # (the constructors draw the weights from the global generator)
    if kind == 'enc':
        mod = T.TransformerEncoder(T.TransformerEncoderLayer(d_model=d, nhead=H, dim_feedforward=2048), num_layers=2)
    else:
        mod = T.TransformerDecoder(T.TransformerDecoderLayer(d_model=d, nhead=H, dim_feedforward=2048), num_layers=2, norm=torch.nn.LayerNorm(d))
    g = torch.Generator().manual_seed(17)
    for n, p_ in mod.named_parameters():          # (test_kernels_gpu._randomise)
        if n.endswith('bias'):
            p_.data = torch.randn(p_.shape, generator=g) * 0.2
        elif 'norm' in n and n.endswith('weight'):
            p_.data = torch.rand(p_.shape, generator=g) + 0.5
    set_stack_p(mod, kind)
    return mod.train()


def stack_inputs(kind, B, L, S):
    g = torch.Generator().manual_seed(300 + 7 * B + L + S)
    d = 256
    x, gy = torch.randn(B * L, d, generator=g), torch.randn(B * L, d, generator=g)
    kpm = torch.zeros(B, L, dtype=torch.bool)
    mem_kpm = torch.zeros(B, max(S, 1), dtype=torch.bool)
    if L > 1:                                     # ragged, never a whole row (the set-up of test_token_stack_node_vs_fp64_oracle)
        kpm[0, L - L // 3:] = True
        if B > 2:
            kpm[2, 1:] = True
    if S:
        mem_kpm[1 % B, S - S // 3:] = True
    mem = torch.randn(B * S, d, generator=g) if S else None
    pos = torch.randn(S, d, generator=g) * 0.3 if S else None
    return x, gy, kpm, mem_kpm, mem, pos


def stack_drop(kind, seeds, masks, B, L, S, H=8, n_layers=2, p_of=None):
    """The oracle's drop(site, tensor) for a lone stack whose host seeds were drawn in `seeds` order (SEED_ORDER per layer).
    p_of: place -> p (default STACK_P; the CPU file passes a wrong one)."""
    p_of = STACK_P if p_of is None else p_of
    order = [f'layers.{i}.{place}' for i in range(n_layers) for place in SEED_ORDER[kind]]
    assert len(seeds) == len(order), (len(seeds), len(order))
    seed_of = dict(zip(order, seeds))

    def drop(site, t):
        place = site.rsplit('.', 1)[1]
        p, sd = p_of[place], seed_of[site]
        if place in ('attn', 'cross'):
            Lk = t.shape[-1]
            m = masks.attention(sd, p, B, H, L, Lk).reshape(B * H, L, Lk)
        else:                                     # seq-first [L, B, C]; the kernels' row is b * L + l
            C = t.shape[-1]
            m = masks.rows(sd, p, B * L, C).reshape(B, L, C).permute(1, 0, 2)
        return t * m
    return drop


def stack_ref(kind, mod, x, gy, kpm, mem_kpm, mem, pos, B, L, S, drop):
    """fp64 oracle of the 2-layer stack -> (y, dx, d memory or None, {parameter name: gradient})."""
    d, H = 256, 8
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in mod.state_dict().items()}
    xr = x.double().requires_grad_(True)
    sf = lambda t, n: t.reshape(B, n, d).permute(1, 0, 2)
    memr = None
    if kind == 'enc':
        yr = detr_ref.torch_encoder(sd, '', sf(xr, L), H, kpm, drop)
    else:
        memr = mem.double().requires_grad_(True)
        y_ = sf(xr, L)
        for i in range(2):
            y_ = detr_ref.decoder_layer(sd, f'layers.{i}.', y_, sf(memr, S), H, kpm, mem_kpm, pos.double()[:, None, :].expand(S, B, d), drop)
        yr = detr_ref._ln(sd, 'norm.', y_)
    yr = yr.permute(1, 0, 2).reshape(B * L, d)
    (yr * gy.double()).sum().backward()
    return yr.detach(), xr.grad, (memr.grad if memr is not None else None), {k: v.grad for k, v in sd.items() if v.grad is not None}


# ---------------------------------------------------------------------------------------------------------------- LayerNorm(x + dropout(r))
def layernorm_inputs(rows, D, pos_rows=0):
    g = torch.Generator().manual_seed(1100 + rows + D)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(x=r(rows, D), r=r(rows, D), gamma=torch.rand(D, generator=g) + 0.5, beta=r(D), gy=r(rows, D))
    if pos_rows:
        t['pos'], t['gp'] = r(pos_rows, D), r(rows, D)
    return t


def layernorm_ref(t, mask):
    """-> dict(y, [ypos,] dx, dr, dgamma, dbeta) in fp64."""
    x, r, gm, bt = [t[k].double().clone().requires_grad_(True) for k in ('x', 'r', 'gamma', 'beta')]
    D = x.shape[1]
    y = F.layer_norm(x + r * mask, (D,), gm, bt, 1e-5)
    loss = (y * t['gy'].double()).sum()
    out = dict(y=y.detach())
    if 'pos' in t:
        ypos = y + t['pos'].double().repeat(x.shape[0] // t['pos'].shape[0], 1)
        loss = loss + (ypos * t['gp'].double()).sum()
        out['ypos'] = ypos.detach()
    loss.backward()
    out.update(dx=x.grad, dr=r.grad, dgamma=gm.grad, dbeta=bt.grad)
    return out


# ---------------------------------------------------------------------------------------------------------------- fused feed-forward tail
def ffn_modules(M, F_):
    """(linear1, linear2, norm_a, norm_b) fp32 on the CPU + inputs (test_ln_ffn_ln_fused_tail_vs_fp64_reference's set-up)."""
    torch.manual_seed(60 + M)
    D = 256
    l1 = torch.nn.Linear(D, F_); l2 = torch.nn.Linear(F_, D); lna = torch.nn.LayerNorm(D); lnb = torch.nn.LayerNorm(D)
    for ln in (lna, lnb):
        ln.weight.data.uniform_(0.5, 1.5); ln.bias.data.normal_(0, 0.1)
    x = torch.randn(M, D); r = torch.randn(M, D); gy = torch.randn(M, D)
    return (l1, l2, lna, lnb), x, r, gy


def ffn_ref(mods, x, r, gy, m_a, m_h, m_b):
    """fp64: x1 = LN_a(x + r * m_a); y = LN_b(x1 + linear2(relu(linear1(x1)) * m_h) * m_b) -> (y, dx, dr, [parameter gradients in module order])."""
    D = x.shape[1]
    ps = [[p_.detach().double().clone().requires_grad_(True) for p_ in m.parameters()] for m in mods]
    (w1, b1), (w2, b2), (ga, ba), (gb, bb) = ps
    xr, rr = x.double().requires_grad_(True), r.double().requires_grad_(True)
    x1 = F.layer_norm(xr + rr * m_a, (D,), ga, ba, 1e-5)
    h = torch.relu(F.linear(x1, w1, b1)) * m_h
    y = F.layer_norm(x1 + F.linear(h, w2, b2) * m_b, (D,), gb, bb, 1e-5)
    (y * gy.double()).sum().backward()
    return y.detach(), xr.grad, rr.grad, [p_.grad for grp in ps for p_ in grp]


def relu_flip_share(a, b, thresh):
    """close_up_to_relu_flips' measure: the share of entries whose error, relative to the reference's maximum, exceeds `thresh` (and the largest)."""
    e = (a.detach().double().cpu() - b).abs() / b.abs().max()
    return (e > thresh).double().mean().item(), e.max().item()


# ---------------------------------------------------------------------------------------------------------------- linear + relu + dropout (GEMM epilogue)
LINEAR_CLEARANCE = 6e-6      # twice the largest fp32 error of a K = 256 pre-activation at these magnitudes (2.9e-6 measured against fp64)


def linear_inputs(M, N, K):
    """x, w, b, gy.  No pre-activation lies within LINEAR_CLEARANCE of 0, so the relu cannot land on different sides in fp32 and fp64 (one such unit moves
    a row of dW by percents: the flips test_ln_ffn_ln_fused_tail_vs_fp64_reference tolerates by share): with a million outputs that takes a searched
    seed (tests/test_dropout_ref_cpu.py asserts the clearance)."""
    g = torch.Generator().manual_seed({(520, 2048): 3875}.get((M, N), 1200 + M + N))
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05, torch.randn(N, generator=g), torch.randn(M, N, generator=g)


def linear_ref(x, w, b, gy, mask):
    xr, wr, br = [t.double().clone().requires_grad_(True) for t in (x, w, b)]
    y = F.relu(F.linear(xr, wr, br)) * mask
    y.backward(gy.double())
    return y.detach(), xr.grad, wr.grad, br.grad


# ---------------------------------------------------------------------------------------------------------------- mha_forward(same_qk=True, qk_pos=...)
def mha_inputs(B, L, d):
    g = torch.Generator().manual_seed(1300 + B + L)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {'in_proj_weight': r(3 * d, d) / math.sqrt(d), 'in_proj_bias': r(3 * d) * 0.2, 'out_proj.weight': r(d, d) / math.sqrt(d), 'out_proj.bias': r(d) * 0.2}
    return sd, r(B * L, d), r(L, d) * 0.3, r(B * L, d), ragged_kpm(B, L)


def mha_ref(sd, x, pos, gy, kpm, B, L, d, H, mask):
    """fp64 detr_ref.mha with q = k = x + pos, v = x and the probabilities' mask [B, H, L, L] -> (y, dx, {parameter: gradient})."""
    sdr = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    sf = lambda t: t.reshape(B, L, d).permute(1, 0, 2)
    xs = sf(xr)
    qk = xs + pos.double()[:, None, :]
    y = detr_ref.mha(sdr, '', qk, qk, xs, H, kpm, drop=lambda site, p: p * mask.reshape(B * H, L, L))
    y = y.permute(1, 0, 2).reshape(B * L, d)
    (y * gy.double()).sum().backward()
    return y.detach(), xr.grad, {k: v.grad for k, v in sdr.items()}
