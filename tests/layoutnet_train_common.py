"""Shared by tools/gen_layoutnet_train_golden.py (which drives the reference) and tests/test_layoutnet_train_*.py: the seeded cases of
tests/golden/layoutnet_train.npz, the batches of its training trajectory, and a restatement of LayoutNet.forward and of the detector's loss as
pure functions over a state dict (reference training/networks_layoutnet.py:48-86), built from oracle.detr_ref and F.linear so that it shares no
code with layoutdetr_amd and runs in float32 or float64.  Everything is a function of names and seeds (oracle/seeded.py)."""
import math

import torch
import torch.nn.functional as F

from oracle import detr_ref, seeded

import layout_eval_common as C

NHEAD = 4
W_BBOX = 10.0
# lengths cycle 1..N (layout_eval_common.seeded_layouts): one valid element, a full tile (N = 15 with the class token = 16 rows) and 1 of 15 all occur
CASES = dict(A=dict(num_label=13, N=9, n=18), B=dict(num_label=5, N=15, n=15), C=dict(num_label=13, N=20, n=6))
TRAJ = dict(num_label=13, N=9, n=64, batch=16, steps=8, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, noise_std=0.01, noise_p=0.5)


def case_inputs(tag):
    """-> bbox [n, N, 4], label [n, N], padding_mask [n, N] bool, is_real [n] bool (alternating)."""
    c = CASES[tag]
    bbox, label, pad = C.seeded_layouts(f'train.{tag}', n=c['n'], N=c['N'], num_label=c['num_label'])
    return bbox, label, pad, torch.arange(c['n']) % 2 == 0


def to_dtype(sd, dtype):
    return {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}


def _lin(sd, pre, x):
    return F.linear(x, sd[pre + '.weight'], sd[pre + '.bias'])


def forward_ref(sd, bbox, label, pad):
    """-> logit_disc [B], logit_cls [M, L], bbox_pred [M, 4], features [B, 256]."""
    B, N, _ = bbox.shape
    x = torch.cat([_lin(sd, 'fc_bbox', bbox), sd['emb_label.weight'][label]], dim=-1)
    x = torch.relu(_lin(sd, 'enc_fc_in', x)).permute(1, 0, 2)
    feat = detr_ref.token_encoder_layoutganpp(sd, 'enc_transformer.', x, pad, NHEAD)[0]
    disc = _lin(sd, 'fc_out_disc', feat).squeeze(-1)
    x = torch.cat([feat.unsqueeze(0).expand(N, -1, -1), sd['pos_token'][:N].expand(-1, B, -1)], dim=-1)
    x = torch.relu(_lin(sd, 'dec_fc_in', x))
    x = detr_ref.torch_encoder(sd, 'dec_transformer.', x, NHEAD, pad)
    x = x.permute(1, 0, 2)[~pad]
    return disc, _lin(sd, 'fc_out_cls', x), torch.sigmoid(_lin(sd, 'fc_out_bbox', x)), feat


def loss_terms(disc, cls, box, bbox, label, pad, is_real, w_bbox=W_BBOX):
    """The detector's loss from forward's outputs -> (L_disc, L_cls, L_bbox, total); the box target is data (no gradient)."""
    l_disc = F.binary_cross_entropy_with_logits(disc, is_real.to(disc.dtype))
    l_cls = F.cross_entropy(cls, label[~pad])
    l_bbox = F.mse_loss(box, bbox.detach()[~pad].to(box.dtype))
    return l_disc, l_cls, l_bbox, l_disc + l_cls + w_bbox * l_bbox


def loss_ref(sd, bbox, label, pad, is_real, w_bbox=W_BBOX):
    disc, cls, box, _ = forward_ref(sd, bbox, label, pad)
    return loss_terms(disc, cls, box, bbox, label, pad, is_real, w_bbox)


def perturb_ref(bbox, flags, eps, std):
    return torch.where(flags[:, None, None], (bbox + std * eps).clamp(0.0, 1.0), bbox)


def trajectory_batches():
    """The eight batches of the stored trajectory: two passes over 64 seeded layouts in batches of 16; per step seeded flags (perturbed with
    probability noise_p -> the fake class) and unit-variance uniform noise -> [(bbox, label, padding_mask, is_real)]."""
    t = TRAJ
    bbox, label, pad = C.seeded_layouts('train.traj', n=t['n'], N=t['N'], num_label=t['num_label'])
    a = math.sqrt(3.0)
    out = []
    for k in range(t['steps']):
        sl = slice((k * t['batch']) % t['n'], (k * t['batch']) % t['n'] + t['batch'])
        flags = seeded.uniform(f'layoutnet_train.flags.{k}', (t['batch'],), 7, 0.0, 1.0) < t['noise_p']
        eps = seeded.uniform(f'layoutnet_train.eps.{k}', (t['batch'], t['N'], 4), 7, -a, a)
        out.append((perturb_ref(bbox[sl], flags, eps, t['noise_std']), label[sl], pad[sl], ~flags))
    return out
