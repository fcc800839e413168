"""LayoutNet, the feature network of the layout FID (reference: training/networks_layoutnet.py:17-66; from LayoutGAN++).

Same parameter names and shapes as the reference, so `load_state_dict(strict=True)` takes a reference `layoutnet_*.pth.tar`, and a
file written by layoutdetr_amd/train_layoutnet.py loads into the reference.  `extract_features` (the metric) and `forward` (:68-86, the
reconstruction that TRAINS LayoutNet: real / fake logit, class logits and boxes of the valid elements) each run one of two ways, chosen
from what they are given:
* fused: one launch (csrc/layoutnet.hip: ldetr_layoutnet_features_f32; csrc/layoutnet_train.hip: ldetr_layoutnet_forward_f32) when no
  gradient is asked for and a sample fits one 16-row tile (N + 1 <= 16; forward: at most 16 labels as well).  Eval-mode arithmetic;
* composed: the existing modules (TransformerWithToken_layoutganpp / TransformerEncoder on the generic attention kernels: 4 heads of
  width 64) otherwise: differentiable in every parameter and in bbox, dropout as the layers are configured.
`forward_dense` is forward before its gather of the valid rows (which synchronises with the host).  The fused paths read packed copies
of the parameters, rebuilt when a parameter's `_version` or storage changes; a caller that writes parameters through raw pointers calls
`invalidate_packs()`.  There is no CPU path."""
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
FUSED_MAX_LABELS = 16                       # forward only: the class head is one 16-column tile of the fused kernel
# which way extract_features ('fused' / 'composed') and forward ('forward_fused' / 'forward_composed') went (tests assert it, like hip.stacks.NODE_RUNS)
PATH_RUNS = dict(fused=0, composed=0, forward_fused=0, forward_composed=0)


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
        # decoder (forward only: the reconstruction that trains the network; the metric never evaluates it)
        self.pos_token = nn.Parameter(torch.rand(max_bbox, 1, d_model))
        self.dec_fc_in = nn.Linear(d_model * 2, d_model)
        self.dec_transformer = TransformerEncoder(TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=d_model // 2), num_layers=num_layers)
        self.fc_out_cls = nn.Linear(d_model, num_label)
        self.fc_out_bbox = nn.Linear(d_model, 4)
        self._packed = None
        self._packed_dec = None

    def forward(self, bbox, label, padding_mask):
        """bbox [B, N, 4], label [B, N] int64, padding_mask [B, N] bool (True = padded) -> logit_disc [B], logit_cls [M, num_label],
        bbox_pred [M, 4] (after the sigmoid); M = the non-padded elements in batch-major order (reference :68-86)."""
        if not (bbox.is_cuda and label.is_cuda and padding_mask.is_cuda):
            raise NotImplementedError('LayoutNet.forward: no CPU path (bbox, label and padding_mask must live in GPU memory)')
        logit_disc, logit_cls, bbox_pred = self.forward_dense(bbox, label, padding_mask)
        keep = ~(padding_mask if padding_mask.dtype == torch.bool else padding_mask != 0)
        return logit_disc, logit_cls[keep], bbox_pred[keep]

    def forward_dense(self, bbox, label, padding_mask, return_features=False):
        """forward() before the gather (which synchronises with the host: M is data): logit_disc [B], logit_cls [B, N, num_label],
        bbox_pred [B, N, 4][, features [B, 256]].  Padded rows hold 0 on the fused path and unspecified finite values on the composed one;
        the masked losses of train_layoutnet.detector_loss do not read them."""
        if not (bbox.is_cuda and label.is_cuda and padding_mask.is_cuda):
            raise NotImplementedError('LayoutNet.forward_dense: no CPU path (bbox, label and padding_mask must live in GPU memory)')
        if self._forward_fused_usable(bbox):
            out = self._forward_fused(bbox, label, padding_mask)
        else:
            out = self._forward_composed(bbox, label, padding_mask)
        return out if return_features else out[:3]

    def invalidate_packs(self):
        """Forget the packed copies of the parameters: for a caller that writes parameters through raw pointers (the flat-buffer Adam of
        training_loop.DataParallelStep), which `_version` does not see."""
        self._packed = None
        self._packed_dec = None

    # ---- forward, fused: one launch of csrc/layoutnet_train.hip
    def _decoder_tensors(self):
        ts = [self.pos_token, self.dec_fc_in.weight, self.dec_fc_in.bias]
        for l in self.dec_transformer.layers:
            ts += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias, l.norm1.weight, l.norm1.bias,
                   l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm2.weight, l.norm2.bias]
        return ts + [self.fc_out_cls.weight, self.fc_out_cls.bias, self.fc_out_bbox.weight, self.fc_out_bbox.bias, self.fc_out_disc.weight, self.fc_out_disc.bias]

    def _packed_decoder(self):
        """The decoder and the three heads as the second buffer ldetr_layoutnet_forward_f32 reads (include/ldetr_hip.h lists the order): the
        heads zero-padded to whole 16-row tiles, every tensor 16-byte aligned."""
        ts = self._decoder_tensors()
        key = tuple((t.data_ptr(), t._version, t.device) for t in ts)
        if self._packed_dec is None or self._packed_dec[0] != key:
            pad_to = [None] * (len(ts) - 6) + [16 * 256, 16, 16 * 256, 16, 256, 4]
            parts = []
            for t, n in zip(ts, pad_to):
                v = t.detach().to(torch.float32).reshape(-1)
                parts.append(v if n is None or n == v.numel() else torch.cat([v, v.new_zeros(n - v.numel())]))
            self._packed_dec = (key, torch.cat(parts).contiguous())
        return self._packed_dec[1]

    def _forward_fused_usable(self, bbox):
        wants_grad = torch.is_grad_enabled() and (bbox.requires_grad or any(p.requires_grad for p in self.parameters()))
        return (bbox.dtype == torch.float32 and bbox.dim() == 3 and 1 <= bbox.shape[1] and bbox.shape[1] + 1 <= FUSED_MAX_TOKENS
                and self.num_label <= FUSED_MAX_LABELS and not wants_grad)

    def _forward_fused(self, bbox, label, padding_mask):
        B, N, _ = bbox.shape
        x = core.f32c(bbox.detach())
        lb = label.to(torch.int64).contiguous()
        pm = (padding_mask if padding_mask.dtype == torch.bool else padding_mask != 0).contiguous().view(torch.uint8)
        w, wd = self._packed_weights(), self._packed_decoder()
        dev = x.device
        disc = torch.empty((B,), device=dev, dtype=torch.float32)
        cls = torch.empty((B, N, self.num_label), device=dev, dtype=torch.float32)
        box = torch.empty((B, N, 4), device=dev, dtype=torch.float32)
        feat = torch.empty((B, 256), device=dev, dtype=torch.float32)
        core.check(core.lib().ldetr_layoutnet_forward_f32(core.ptr(x), core.ptr(lb), core.ptr(pm), core.ptr(w), w.numel(), core.ptr(wd), wd.numel(), self.num_label,
                                                          B, N, core.ptr(disc), core.ptr(cls), core.ptr(box), core.ptr(feat), core.stream()), 'layoutnet_forward')
        PATH_RUNS['forward_fused'] += 1
        return disc, cls, box, feat

    # ---- forward, composed: the existing modules and kernels, differentiable in every parameter and in bbox; dropout is the layers' own
    def _forward_composed(self, bbox, label, padding_mask):
        B, N, _ = bbox.shape
        pm = padding_mask if padding_mask.dtype == torch.bool else padding_mask != 0
        feat = self._encode_composed(bbox, label, pm, None)
        disc = linear(feat, self.fc_out_disc.weight, self.fc_out_disc.bias).squeeze(-1)
        x = torch.cat([feat.unsqueeze(1).expand(B, N, -1), self.pos_token[:N, 0].unsqueeze(0).expand(B, N, -1)], dim=-1).reshape(B * N, -1)
        x = linear(x, self.dec_fc_in.weight, self.dec_fc_in.bias, act=core.ACT_RELU)
        x = self.dec_transformer.forward2d(x, B, N, pm, None)                   # batch-major rows: the reference's x.permute(1, 0, 2)
        cls = linear(x, self.fc_out_cls.weight, self.fc_out_cls.bias).reshape(B, N, -1)
        box = torch.sigmoid(linear(x, self.fc_out_bbox.weight, self.fc_out_bbox.bias)).reshape(B, N, 4)
        PATH_RUNS['forward_composed'] += 1
        return disc, cls, box, feat

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
        x = self._encode_composed(bbox, label, padding_mask, table)
        PATH_RUNS['composed'] += 1
        return x

    def _encode_composed(self, bbox, label, padding_mask, table):
        B, N, _ = bbox.shape
        if table:
            label = map_labels(label, label_idx_replace=table is LABEL_MAP, label_idx_replace_2=table is LABEL_MAP_2)
        b = linear(bbox.reshape(B * N, 4), self.fc_bbox.weight, self.fc_bbox.bias)
        l = self.emb_label.weight[label.reshape(-1)]
        x = linear(torch.cat([b, l], dim=-1), self.enc_fc_in.weight, self.enc_fc_in.bias, act=core.ACT_RELU)
        x = x.reshape(B, N, -1).permute(1, 0, 2)
        x = self.enc_transformer(x, padding_mask)
        return x[0]

    def extract_features(self, bbox, label, padding_mask, label_idx_replace=False, label_idx_replace_2=False):
        """bbox [B, N, 4], label [B, N] int64, padding_mask [B, N] bool (True = padded) -> [B, 256]: row 0 (the class token) of the encoder."""
        core.require_gpu(bbox, label, padding_mask)
        table = LABEL_MAP if label_idx_replace else (LABEL_MAP_2 if label_idx_replace_2 else None)
        if self._fused_usable(bbox, label, padding_mask):
            return self._extract_fused(bbox, label, padding_mask, table)
        return self._extract_composed(bbox, label, padding_mask, table)
