"""Train LayoutNet, the feature detector of the layout FID, on a banner archive:  python -m layoutdetr_amd.train_layoutnet --data <train.zip>

The metric `layout_fid50k_train|val` opens `pretrained/layoutnet_<dataset name>.pth.tar` (metrics/layout_frechet_inception_distance.py); this writes
that file.  The task is LayoutGAN++'s pre-training of the network in outline (Kikuchi et al., "Constrained Graphic Layout Generation via Latent
Optimization"): a layout whose boxes were perturbed is the "fake" class, the encoder's class token is asked to tell the two apart, and the decoder
reconstructs the labels and the boxes the network was given.  That recipe is not part of the reference tree, so every constant is a named
argument and the defaults are starting values, not tuned ones: judge them by the periodic evaluation lines.

The layouts of the whole archive live on the device (LayoutDataset.layouts(): no image is decoded); a batch is an index gather.  A training step
is LayoutNet.forward's composed path (differentiable), the loss tail of hip/losses.py and the flat-parameter fused Adam of the training loop; the
evaluation passes go through the fused forward (one launch per batch, csrc/layoutnet_train.hip)."""
import argparse
import os
import sys
import uuid

import torch

from .hip import losses as hl
from .metrics.metric_layoutnet import detector_num_label
from .metrics.metric_utils_layout import _label_flags
from .training.networks_layoutnet import LayoutNet, map_labels


def detector_path(dataset_name):
    """Where the metric looks for the detector of a dataset (layout_frechet_inception_distance.py: 'pretrained/layoutnet_%s.pth.tar')."""
    return 'pretrained/layoutnet_%s.pth.tar' % dataset_name


def perturb(bbox, flags, eps, std):
    """clamp(bbox + std * eps, 0, 1) for the samples whose flag is set, bbox for the others.  bbox, eps [B, N, 4]; flags [B] bool."""
    return torch.where(flags.reshape(-1, 1, 1), (bbox + std * eps).clamp(0.0, 1.0), bbox)


def detector_loss(net, bbox, label, padding_mask, is_real, w_bbox=10.0):
    """-> ({'L_disc', 'L_cls', 'L_bbox', 'total'}: detached device scalars, total with autograd).
    L_disc = mean binary cross entropy with logits of logit_disc against is_real [B] bool; L_cls = mean cross entropy of the M valid rows against
    their labels; L_bbox = mean squared error of bbox_pred against the valid rows of the boxes that went in (as data: the target carries no
    gradient); total = L_disc + L_cls + w_bbox * L_bbox.  Evaluated on the dense outputs, without the gather of the valid rows: no host
    synchronisation."""
    from .training.med import softmax_cross_entropy
    pm = padding_mask if padding_mask.dtype == torch.bool else padding_mask != 0
    logit_disc, logit_cls, bbox_pred = net.forward_dense(bbox, label, pm)
    # BCE with logits against 1 is softplus(-x), against 0 softplus(x)
    sign = torch.where(is_real.reshape(-1).to(torch.bool), -1.0, 1.0).to(logit_disc.dtype)
    ce = softmax_cross_entropy(logit_cls.flatten(0, 1), label.flatten().masked_fill(pm.flatten(), -100), raw=True)
    mse = hl.masked_mse(bbox_pred, bbox.detach(), (~pm).contiguous().view(torch.uint8))
    total, rep = hl.combine([hl.Term('L_disc', logit_disc * sign, 1.0, hl.SOFTPLUS), hl.Term('L_cls', ce, 1.0, hl.RATIO),
                             hl.Term('L_bbox', mse, float(w_bbox))])
    terms = dict(L_disc=rep['L_disc'].mean(), L_cls=rep['L_cls'], L_bbox=mse.detach(), total=total.detach())
    return terms, total


def set_dropout(net, p):
    """The dropout rate of every transformer layer of `net` (nn.TransformerEncoderLayer's single `dropout` argument)."""
    for stack in (net.enc_transformer.core, net.dec_transformer):
        for layer in stack.layers:
            layer.self_attn.dropout = float(p)
            for d in (layer.dropout, layer.dropout1, layer.dropout2):
                d.p = float(p)


class LayoutNetTrainer(object):
    """`net` (on the GPU) under the flat-parameter fused Adam of the training loop (one launch per step over parameters, gradients and moments)."""

    def __init__(self, net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, dropout=None, w_bbox=10.0):
        from .training import training_loop as tl
        if next(net.parameters()).device.type != 'cuda':
            raise NotImplementedError('LayoutNetTrainer: the network must live in GPU memory (no CPU path)')
        self.net, self.w_bbox = net, float(w_bbox)
        if dropout is not None:
            set_dropout(net, dropout)
        net.requires_grad_(True)
        self.phase = tl.Phase('LayoutNet', net, lr=lr, betas=betas, eps=eps)
        self.dp = tl.DataParallelStep(world_size=1)
        net.invalidate_packs()

    def step(self, bbox, label, padding_mask, is_real):
        """One optimiser step on a batch -> the loss terms of detector_loss as device scalars (nothing comes to the host)."""
        from .hip import core
        net = self.net
        net.train()
        net.requires_grad_(True)
        core.reseed(bbox.device)
        self.phase.fm.zero_grad()
        with torch.enable_grad():
            terms, total = detector_loss(net, bbox, label, padding_mask, is_real, self.w_bbox)
            total.backward()
        self.dp.apply(self.phase)
        net.invalidate_packs()       # Adam wrote the parameters through raw pointers: the fused paths' packed copies are stale
        return terms

    @torch.no_grad()
    def evaluate(self, bboxes, labels, mask, is_real=None, batch=1024):
        """The whole set through the fused forward (eval mode) -> floats: total and per-term loss, class accuracy, box MSE, real / fake accuracy.
        mask [n, N] bool: True = a real element; is_real [n] bool (default: all real)."""
        net = self.net
        was_training = net.training
        net.eval()
        net.invalidate_packs()
        n = bboxes.shape[0]
        if is_real is None:
            is_real = torch.ones(n, dtype=torch.bool, device=bboxes.device)
        acc = torch.zeros(6, dtype=torch.float64, device=bboxes.device)      # sums of: bce, ce, squared error, class hits, disc hits, valid rows
        for i in range(0, n, batch):
            bb, lb, valid, real = bboxes[i:i + batch], labels[i:i + batch], mask[i:i + batch], is_real[i:i + batch]
            disc, cls, box = net.forward_dense(bb, lb, ~valid)
            sign = torch.where(real, -1.0, 1.0)
            bce = torch.nn.functional.softplus(disc * sign).double().sum()
            logp = torch.log_softmax(cls.double(), -1)
            ce = -(logp.gather(-1, lb.clamp(0, cls.shape[-1] - 1).unsqueeze(-1)).squeeze(-1) * valid).sum()
            se = ((box.double() - bb.double()).square().sum(-1) * valid).sum()
            hits = ((cls.argmax(-1) == lb) & valid).sum()
            dhits = ((disc > 0) == real).sum()
            acc += torch.stack([bce, ce, se, hits.double(), dhits.double(), valid.sum().double()])
        net.train(was_training)
        bce, ce, se, hits, dhits, rows = acc.tolist()
        rows = max(rows, 1.0)
        out = dict(L_disc=bce / n, L_cls=ce / rows, L_bbox=se / (4.0 * rows), cls_acc=hits / rows, bbox_mse=se / (4.0 * rows), disc_acc=dhits / n)
        out['total'] = out['L_disc'] + out['L_cls'] + self.w_bbox * out['L_bbox']
        return out


def prepare_labels(labels, mask, out):
    """The training labels as the metric will present them to the detector at `out`: relabelled by the metric's own rule (_label_flags /
    map_labels) -> (labels, num_label).  Refuses when a mapped label of a real element falls outside the detector's table."""
    num_label = detector_num_label(out)
    flags = _label_flags(out)
    mapped = map_labels(labels, **flags)
    used = mapped[mask]
    if used.numel() and (int(used.min()) < 0 or int(used.max()) >= num_label):
        raise ValueError(f'train_layoutnet: labels {int(used.min())}..{int(used.max())} do not fit the {num_label}-label detector that the metric builds for {out!r} '
                         f'(13 labels when the path names one of the datasets the reference lists, else 5; relabelling {flags}): the metric could not '
                         'evaluate this archive under that name')
    return mapped, num_label


def save_detector(net, out):
    """torch.save(state_dict) with the reference's keys, as plain CPU tensors, written to a temporary name and renamed."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    tmp = out + '.' + uuid.uuid4().hex
    torch.save(sd, tmp)
    os.replace(tmp, out)
    return out


def _corpus(dataset_kwargs):
    from .training.training_loop import construct_class_by_name
    ds = construct_class_by_name(**dataset_kwargs)
    bboxes, labels, mask = ds.layouts()
    return ds, bboxes, labels, mask


def train_layoutnet(training_set_kwargs, validation_set_kwargs=None, out=None, steps=20000, batch=64, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, dropout=0.1,
                    w_bbox=10.0, noise_std=0.01, noise_p=0.5, seed=0, eval_every=1000, device=None, log=print):
    """Train a LayoutNet on the layouts of `training_set_kwargs` (LayoutDataset keyword arguments) and write it where the metric opens it
    (`out`, default pretrained/layoutnet_<dataset.name>.pth.tar relative to the working directory) -> (out, last evaluation).
    Each sample of a batch is perturbed with probability `noise_p` (Gaussian, `noise_std`, clamped to [0, 1]) and is then the fake class.  Every
    `eval_every` steps and at the end the validation set (else the training set) is evaluated, as it is and with every layout perturbed."""
    device = torch.device(device if device is not None else 'cuda')
    if device.type != 'cuda':
        raise NotImplementedError('train_layoutnet: no CPU path')
    kw = dict(training_set_kwargs)
    kw.setdefault('class_name', 'layoutdetr_amd.training.dataset_layoutganpp.LayoutDataset')
    ds, bboxes, labels, mask = _corpus(kw)
    if out is None:
        out = detector_path(ds.name)
    labels, num_label = prepare_labels(labels, mask, out)
    bboxes, labels, mask = bboxes.to(device), labels.to(device), mask.to(device)
    if validation_set_kwargs is not None:
        vkw = dict(validation_set_kwargs)
        vkw.setdefault('class_name', kw['class_name'])
        _, vb, vl, vm = _corpus(vkw)
        vl, _ = prepare_labels(vl, vm, out)
        val = (vb.to(device), vl.to(device), vm.to(device))
    else:
        val = (bboxes, labels, mask)
    torch.manual_seed(seed)
    gen = torch.Generator(device=device).manual_seed(seed)
    net = LayoutNet(num_label).to(device)
    trainer = LayoutNetTrainer(net, lr=lr, betas=betas, eps=eps, dropout=dropout, w_bbox=w_bbox)
    n = bboxes.shape[0]
    log(f'train_layoutnet: {n} layouts of {ds.name!r}, {num_label} labels, {sum(p.numel() for p in net.parameters())} parameters -> {out}')

    def evaluate(step):
        vb, vl, vm = val
        real = trainer.evaluate(vb, vl, vm)
        noise = torch.randn(vb.shape, device=device, generator=gen)
        every = torch.ones(vb.shape[0], dtype=torch.bool, device=device)
        fake = trainer.evaluate(perturb(vb, every, noise, noise_std), vl, vm, is_real=~every)
        log(f'step {step:7d}  ' + '  '.join(f'{k} {real[k]:.5f}' for k in ('total', 'L_disc', 'L_cls', 'L_bbox', 'cls_acc', 'bbox_mse'))
            + f"  disc_acc real {real['disc_acc']:.4f} fake {fake['disc_acc']:.4f}")
        return dict(real, disc_acc_fake=fake['disc_acc'])

    last = None
    for step in range(1, steps + 1):
        idx = torch.randint(0, n, (batch,), device=device, generator=gen)
        bb, lb, pm = bboxes[idx], labels[idx], ~mask[idx]
        flags = torch.rand(batch, device=device, generator=gen) < noise_p
        noise = torch.randn(bb.shape, device=device, generator=gen)
        trainer.step(perturb(bb, flags, noise, noise_std), lb, pm, ~flags)
        if eval_every and step % eval_every == 0 and step < steps:
            last = evaluate(step)
    last = evaluate(steps)
    save_detector(net, out)
    log(f'train_layoutnet: wrote {out}')
    return out, last


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m layoutdetr_amd.train_layoutnet', description='Train the layout-FID detector (LayoutNet) on a banner archive.')
    p.add_argument('--data', required=True, help='training archive (<...>/<dataset name>/zip/train.zip)')
    p.add_argument('--val', default=None, help='validation archive (default: evaluate on the training set)')
    p.add_argument('--out', default=None, help='detector file (default: pretrained/layoutnet_<dataset name>.pth.tar, where the metric opens it)')
    p.add_argument('--steps', type=int, default=20000)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--beta1', type=float, default=0.9)
    p.add_argument('--beta2', type=float, default=0.999)
    p.add_argument('--eps', type=float, default=1e-8)
    p.add_argument('--dropout', type=float, default=0.1)
    p.add_argument('--w-bbox', type=float, default=10.0)
    p.add_argument('--noise-std', type=float, default=0.01)
    p.add_argument('--noise-p', type=float, default=0.5)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--eval-every', type=int, default=1000)
    p.add_argument('--max-size', type=int, default=None, help='use a seeded subset of the archive')
    return p.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    ds_kw = lambda path: dict(path=path, max_size=a.max_size, use_labels=False, xflip=False)
    train_layoutnet(ds_kw(a.data), ds_kw(a.val) if a.val else None, out=a.out, steps=a.steps, batch=a.batch, lr=a.lr, betas=(a.beta1, a.beta2), eps=a.eps,
                    dropout=a.dropout, w_bbox=a.w_bbox, noise_std=a.noise_std, noise_p=a.noise_p, seed=a.seed, eval_every=a.eval_every)
    return 0


if __name__ == '__main__':
    sys.exit(main())
