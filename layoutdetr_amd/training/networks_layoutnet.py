"""LayoutNet, the feature network of the layout FID (reference: training/networks_layoutnet.py:17-66; from LayoutGAN++).

Same parameter names and shapes as the reference, so `load_state_dict(strict=True)` takes a reference `layoutnet_*.pth.tar`.  Only
`extract_features` is evaluated on this path (the metric); `forward` -- the reconstruction head that TRAINS LayoutNet -- is not built.
`extract_features` runs one of two ways, chosen from what it is given:
* fused: one launch of csrc/layoutnet.hip (ldetr_layoutnet_features_f32) when no gradient is asked for and a sample fits one 16-row
  tile (N + 1 <= 16);
* composed: the existing modules (TransformerWithToken_layoutganpp on the generic attention kernels: 4 heads of width 64) otherwise.
There is no CPU path."""
import ctypes

import torch
import torch.nn as nn

from ..hip import core
from ..hip.linear import linear
from .detr_transformer import TransformerEncoder, TransformerEncoderLayer
from .util import TransformerWithToken_layoutganpp

# the NET effect of the reference's in-place assignment sequences (:50-61), as lookups for the labels they are defined on
LABEL_MAP = (2, 2, 2, 2, 2, 4, 7, 3)        # label_idx_replace: 0..4 -> 2 (TEXT), 5 -> 4 (BUTTON), 6 -> 7 (ADVERTISEMENT), 7 -> 3 (PICTOGRAM)
LABEL_MAP_2 = (3, 2, 4, 3, 2)               # label_idx_replace_2: 0 -> 3, 1 -> 2, 2 -> 4, 3 -> 3, 4 -> 2

FUSED_MAX_TOKENS = 16
PATH_RUNS = dict(fused=0, composed=0)       # which way extract_features went (tests assert it, like hip.stacks.NODE_RUNS)


def map_labels(label, label_idx_replace=False, label_idx_replace_2=False):
    """The relabelled copy of `label` (the caller's tensor is left alone; the reference overwrites it)."""
    table = LABEL_MAP if label_idx_replace else (LABEL_MAP_2 if label_idx_replace_2 else None)
    if table is None:
        return label
    t = torch.tensor(table, dtype=label.dtype, device=label.device)
    inside = (label >= 0) & (label < len(table))
    return torch.where(inside, t[label.clamp(0, len(table) - 1)], label)


class LayoutNet(nn.Module):
    def __init__(self, num_label):
        super().__init__()
        d_model, nhead, num_layers, max_bbox = 256, 4, 4, 50
        self.num_label = num_label
        # encoder
        self.emb_label = nn.Embedding(num_label, d_model)
        self.fc_bbox = nn.Linear(4, d_model)
        self.enc_fc_in = nn.Linear(d_model * 2, d_model)
        self.enc_transformer = TransformerWithToken_layoutganpp(d_model=d_model, dim_feedforward=d_model // 2, nhead=nhead, num_layers=num_layers)
        self.fc_out_disc = nn.Linear(d_model, 1)
        # decoder: parameters only (a reference checkpoint carries them; strict loading wants them), never evaluated here
        self.pos_token = nn.Parameter(torch.rand(max_bbox, 1, d_model))
        self.dec_fc_in = nn.Linear(d_model * 2, d_model)
        self.dec_transformer = TransformerEncoder(TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=d_model // 2), num_layers=num_layers)
        self.fc_out_cls = nn.Linear(d_model, num_label)
        self.fc_out_bbox = nn.Linear(d_model, 4)
        self._packed = None

    def forward(self, bbox, label, padding_mask):
        raise NotImplementedError('LayoutNet.forward (the reconstruction head that trains LayoutNet) is not part of this path; use extract_features')

    # ---- fused path
    def _encoder_tensors(self):
        ts = [self.emb_label.weight, self.fc_bbox.weight, self.fc_bbox.bias, self.enc_fc_in.weight, self.enc_fc_in.bias, self.enc_transformer.token]
        for l in self.enc_transformer.core.layers:
            ts += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias, l.norm1.weight, l.norm1.bias,
                   l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm2.weight, l.norm2.bias]
        return ts

    def _packed_weights(self):
        """The encoder's parameters as the one buffer ldetr_layoutnet_features_f32 reads (include/ldetr_hip.h lists the order); rebuilt when a
        parameter was replaced or written (load_state_dict, .to())."""
        ts = self._encoder_tensors()
        key = tuple((t.data_ptr(), t._version, t.device) for t in ts)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, torch.cat([t.detach().to(torch.float32).reshape(-1) for t in ts]).contiguous())
        return self._packed[1]

    def _fused_usable(self, bbox, label, padding_mask):
        wants_grad = torch.is_grad_enabled() and (bbox.requires_grad or any(t.requires_grad for t in self._encoder_tensors()))
        return (bbox.is_cuda and bbox.dtype == torch.float32 and bbox.dim() == 3 and bbox.shape[1] + 1 <= FUSED_MAX_TOKENS and bbox.shape[1] >= 1
                and not wants_grad)

    def _extract_fused(self, bbox, label, padding_mask, table):
        B, N, _ = bbox.shape
        x = core.f32c(bbox.detach())
        lb = label.to(torch.int64).contiguous()
        pm = (padding_mask if padding_mask.dtype == torch.bool else padding_mask != 0).contiguous().view(torch.uint8)
        w = self._packed_weights()
        out = torch.empty((B, 256), device=x.device, dtype=torch.float32)
        n = len(table) if table else 0
        cmap = (ctypes.c_int * 16)(*(list(table) if table else []))
        core.check(core.lib().ldetr_layoutnet_features_f32(core.ptr(x), core.ptr(lb), core.ptr(pm), cmap, n, core.ptr(w), w.numel(), self.num_label, B, N,
                                                           core.ptr(out), core.stream()), 'layoutnet_features')
        PATH_RUNS['fused'] += 1
        return out

    # ---- composed path
    def _extract_composed(self, bbox, label, padding_mask, table):
        B, N, _ = bbox.shape
        if table:
            label = map_labels(label, label_idx_replace=table is LABEL_MAP, label_idx_replace_2=table is LABEL_MAP_2)
        b = linear(bbox.reshape(B * N, 4), self.fc_bbox.weight, self.fc_bbox.bias)
        l = self.emb_label.weight[label.reshape(-1)]
        x = linear(torch.cat([b, l], dim=-1), self.enc_fc_in.weight, self.enc_fc_in.bias, act=core.ACT_RELU)
        x = x.reshape(B, N, -1).permute(1, 0, 2)
        x = self.enc_transformer(x, padding_mask)
        PATH_RUNS['composed'] += 1
        return x[0]

    def extract_features(self, bbox, label, padding_mask, label_idx_replace=False, label_idx_replace_2=False):
        """bbox [B, N, 4], label [B, N] int64, padding_mask [B, N] bool (True = padded) -> [B, 256]: row 0 (the class token) of the encoder."""
        core.require_gpu(bbox, label, padding_mask)
        table = LABEL_MAP if label_idx_replace else (LABEL_MAP_2 if label_idx_replace_2 else None)
        if self._fused_usable(bbox, label, padding_mask):
            return self._extract_fused(bbox, label, padding_mask, table)
        return self._extract_composed(bbox, label, padding_mask, table)
