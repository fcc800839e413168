"""Shared-condition decode of the generator: everything of `Generator.forward` (training/networks_detr.py:134-160 of the reference) that does
not depend on the latent runs ONCE per condition, and K candidates are decoded against it.

The reference's inference loop (generate_util.py:415-423) calls G once per seed with the same background, strings and labels: the ResNet
trunk, input_proj, the six encoder layers, the BERT text encoder and the label / text-length embeddings are recomputed K times although G_ema
is in eval mode (FrozenBatchNorm, no dropout) and only z differs.  Here, per condition c of C (`encode_condition`):
    trunk, input_proj, encoder            -> memory [C * S, d], memory + pos
    K / V projections of all six layers   -> hip.attention.grouped_kv: one [C * S, 2 * layers * d] buffer the layers read in place
    emb_label, text encoder, enc_text_len -> the latent-independent 3 * bert_f_dim columns of fc_in's input
and per candidate (`decode_candidates`): fc_z, fc_in, the decoder, bbox_embed + sigmoid on C * K * N rows (row = (c * K + k) * N + n).
    self-attention:  batch C * K, L = N                       (each candidate attends over its own N slots)
    cross-attention: batch C,     Lq = K * N, Lk = S           (the K * N query rows of one condition's candidates are consecutive and
                                                               independent, so the attention entry points read ONE K / V copy per condition:
                                                               the memory and its projections are never expanded or copied K times)
Every row of a GEMM / LayerNorm / attention launch is computed from that row's inputs alone, so the values equal the K separate forward calls
up to the summation order of whichever tile policy the launch picks for the larger row count.  The stack node (hip/stacks.py) assumes one
memory per sample and is not used: the per-layer launches run.
Candidates are decoded in passes of CHUNK candidates per condition (CHUNK * N query rows), the last pass padded with zero latents, because
the contraction engine picks tiles and split-K by row count: measured on an MI355X, one candidate's boxes differ in the last bit (6e-8) between
launches of 9, 18, ... 1152 rows.  Only launches of ONE shape make a candidate's boxes independent of how many others are decoded beside it,
so that sample(seeds a) and sample(seeds b) on one Condition equal sample(seeds a + b) bit for bit.  A pass is bound by its ~60 launches, not
by its rows (1.76 ms at 144 rows, 1.91 ms at 1152), so CHUNK is large: K <= 128 is ONE pass over the K * N rows of each
condition, as a plain K * N-row decode would be, K = 1 pays about 0.15 ms for the padding, and K = 1024 takes 8 passes.
Limits: CHUNK * N = 1152 query rows per condition and launch; K * N <= 16384 rows per condition and call."""
import torch

from ..hip.attention import grouped_kv, mha_cross_kv
from ..hip.layernorm import add_layernorm

MAX_QUERY_ROWS = 16384
CHUNK = 128      # candidates per decoder pass and condition: 1152 query rows at N = 9


class Condition(object):
    """What `Generator.encode_condition` keeps for any number of `decode_candidates` calls."""

    def __init__(self, kvs, mem_kpm, S, feat, padding_mask):
        self.kvs = kvs                      # per decoder layer (K_i, V_i): [C * S, d] column blocks of the grouped projection
        self.mem_kpm = mem_kpm              # [C, S] uint8 key-padding mask of the memory
        self.S = S
        self.feat = feat                    # [C, N, 3 * bert_f_dim]: label | text | text-length features
        self.padding_mask = padding_mask    # [C, N] bool, a prefix mask
        self.C, self.N = feat.shape[0], feat.shape[1]
        self.num = (~padding_mask).sum(1).to(torch.int32)     # valid prefix length per condition

    @property
    def device(self):
        return self.feat.device


def check_prefix_mask(padding_mask):
    """The reference builds `mask = [1] * n + [0] * (9 - n)` (generate_util.py:413): the finishing functions index the first n slots."""
    pm = padding_mask.to(torch.bool)
    if pm.ndim != 2:
        raise ValueError(f'padding_mask must be [C, N] (got {tuple(pm.shape)})')
    if pm.shape[1] > 1 and bool((pm[:, :-1] & ~pm[:, 1:]).any()):
        raise ValueError('padding_mask must be a prefix mask: the valid elements first, the padded slots after them (generate_util.py:413)')
    return pm


def encode_memory(transformer, src, mask, pos_embed):
    """Transformer.forward up to the decoder, plus the decoder layers' memory K / V projections -> (kvs, mem_kpm uint8 [B, S], S)."""
    from .detr_transformer import _mask_u8, _rows_from_nchw
    bs = src.shape[0]
    x2, S = _rows_from_nchw(src)
    pos2, _ = _rows_from_nchw(pos_embed)
    pos2 = pos2.contiguous()
    mem_kpm = _mask_u8(mask.flatten(1))
    mem2, mem_pos2 = transformer.encoder.forward2d(x2, bs, S, mem_kpm, pos2, want_pos=True)
    kvs = grouped_kv(mem_pos2, mem2, [l.multihead_attn for l in transformer.decoder.layers])
    return [(k, v) for k, v, _ in kvs], mem_kpm, S


def decode_rows(transformer, t2, C, K, N, S, tgt_kpm, mem_kpm, kvs):
    """The decoder stack on t2 [C * K * N, d] against C memories (per-layer launches; see the module docstring for the two batch shapes)."""
    from .detr_transformer import _add_ln, _add_ln_ffn_add_ln, _mha, _mask_u8
    dec = transformer.decoder
    tgt_kpm = _mask_u8(tgt_kpm)
    for layer, (Kp, Vp) in zip(dec.layers, kvs):
        a, t2 = _mha(layer.self_attn, t2, t2, t2, C * K, N, N, tgt_kpm, layer.training, same_qkv=True)
        t2 = _add_ln(layer.norm1, t2, a, layer.dropout1, layer.training)
        m = layer.multihead_attn
        a, t2 = mha_cross_kv(t2, Kp, Vp, None, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias, m.num_heads, C, K * N, S,
                             key_padding_mask=mem_kpm, p_drop=m.dropout if layer.training else 0.0)
        t2 = _add_ln_ffn_add_ln(layer, layer.norm2, t2, a, layer.dropout2, layer.norm3, layer.dropout3)
    if dec.norm is not None:
        t2 = add_layernorm(t2, None, dec.norm.weight, dec.norm.bias, dec.norm.eps)
    return t2


def encode_condition(G, background, bbox_class, bbox_text, padding_mask):
    from . import networks_detr as nd
    pm = check_prefix_mask(padding_mask)
    C, N = pm.shape
    with torch.no_grad():
        bg_feat, pos = G.trunk(background)
        bg_feat, mask = bg_feat[-1].decompose()
        kvs, mem_kpm, S = encode_memory(G.transformer, G.input_proj(bg_feat), mask, pos[-1])
        bbox_text = nd._coerce_text(G, bbox_text, bbox_class.device)
        l = G.emb_label(bbox_class)
        text_feat, text_len = nd._text_inputs(G, bbox_text, C, N, bbox_class.device)
        feat = torch.cat([l, text_feat, G.enc_text_len(text_len)], dim=-1)
    return Condition(kvs, mem_kpm, S, feat, pm.to(feat.device))


def decode_candidates(G, cond, z):
    """z: [K, N, z_dim] (the same latents for every condition) or [C, K, N, z_dim] -> bbox [C, K, N, 4]."""
    from . import networks_detr as nd
    C, N = cond.C, cond.N
    if z.ndim == 3:
        z = z.unsqueeze(0).expand(C, -1, -1, -1)
    if z.ndim != 4 or z.shape[0] != C or z.shape[2] != N or z.shape[3] != G.z_dim:
        raise ValueError(f'z must be [K, {N}, {G.z_dim}] or [{C}, K, {N}, {G.z_dim}] (got {tuple(z.shape)})')
    K = z.shape[1]
    if K < 1 or K * N > MAX_QUERY_ROWS:
        raise ValueError(f'decode_candidates: K * N = {K} * {N} query rows per condition; needs 1 <= K and K * N <= {MAX_QUERY_ROWS}')
    with torch.no_grad():
        z = z.to(device=cond.device, dtype=torch.float32)
        tgt_kpm = cond.padding_mask.unsqueeze(1).expand(-1, CHUNK, -1).reshape(C * CHUNK, N)
        feat = cond.feat.unsqueeze(1).expand(-1, CHUNK, -1, -1)
        out = []
        for k0 in range(0, K, CHUNK):
            zc = z[:, k0:k0 + CHUNK]
            if zc.shape[1] < CHUNK:
                zc = torch.cat([zc, zc.new_zeros((C, CHUNK - zc.shape[1], N, G.z_dim))], dim=1)
            z0 = nd.normalize_2nd_moment(zc.reshape(C * CHUNK, -1))
            zf = G.fc_z(z0).view(C, CHUNK, 1, -1).expand(-1, -1, N, -1)
            t2 = G.fc_in(torch.cat([zf, feat], dim=-1).reshape(C * CHUNK * N, -1), final_relu=True)
            hs = decode_rows(G.transformer, t2, C, CHUNK, N, cond.S, tgt_kpm, cond.mem_kpm, cond.kvs)
            out.append(G.bbox_embed(hs).sigmoid().view(C, CHUNK, N, 4))
        return (out[0] if len(out) == 1 else torch.cat(out, dim=1))[:, :K].contiguous()
