"""StyleGAN2Loss for the LayoutDETR G/D step (reference: training/loss.py:28-218) over the gfx950 modules.
Same class name, constructor arguments, phase names and loss composition; the default `gamma=0,
pl_weight=0` configuration (train.py:135-136) makes Greg/Dreg no-ops exactly as loss.py:77-80 does.
R1 (`--gamma`, loss.py:207-215) and path-length regularisation (loss.py:119-142) differentiate D's score / G's boxes with
`create_graph=True`: those phases run the heads and the decoder stack between the differentiated input and output on the
twice-differentiable nodes of hip/composite.py (SURVEY §7 'second-order autograd'); everything else keeps the fused kernels."""

import torch
import torch.nn.functional as F

from ..detr_util.misc import NestedTensor
from ..hip import composite, core

from ..hip import losses as hl
from ..metrics.metric_layoutnet import compute_alignment, compute_overlap, generalized_iou_loss, layout_losses_per_sample
from ..hip import rider as hrider
from .detr_backbone import ResNet50Body, dual_trunk_forward, trunk_body
from .detr_transformer import Transformer


def _masked_mse(a, b, valid):
    """F.mse_loss(a[valid], b[valid]) without the gather: a, b [B,N,D], valid [B,N] bool."""
    if a.is_cuda and a.dtype == torch.float32 and not b.requires_grad:
        return hl.masked_mse(a, b, valid.contiguous().view(torch.uint8))      # one launch per direction (csrc/layout_loss.hip) instead of ~9 + ~12
    vf = valid.to(a.dtype)
    return ((a - b).square().sum(-1) * vf).sum() / (vf.sum().clamp_min(1.0) * a.shape[-1])


def _masked_ce(logits, target, valid):
    """F.cross_entropy(logits[valid], target[valid]) without the gather, as the (loss sum, count) pair of hip.losses.combine's RATIO term:
    logits [B,N,L]; the padded slots become ignored targets of the fused softmax-cross-entropy kernel (csrc/xent.hip: loss and row log-sum-exp
    in one pass, gradient in one pass): the same mean over the same slots in 4 launches instead of ~13."""
    from .med import softmax_cross_entropy
    return softmax_cross_entropy(logits.flatten(0, 1), target.flatten().masked_fill(~valid.flatten(), -100), raw=True)


def _masked_giou(a, b, valid):
    """generalized_iou_loss(a[valid], b[valid]) without the gather (padded slots are replaced by a unit box first)."""
    unit = a.new_full((4,), 0.5)
    unit[2:] = 1.0                      # [0.5, 0.5, 1, 1] built on device (no host copy: stays hipGraph-capturable)
    v3 = valid.unsqueeze(-1)
    a2 = torch.where(v3, a, unit).flatten(0, 1)
    b2 = torch.where(v3, b, unit).flatten(0, 1)
    l1, t1, r1, b1 = a2[:, 0] - a2[:, 2] / 2, a2[:, 1] - a2[:, 3] / 2, a2[:, 0] + a2[:, 2] / 2, a2[:, 1] + a2[:, 3] / 2
    l2, t2, r2, bb2 = b2[:, 0] - b2[:, 2] / 2, b2[:, 1] - b2[:, 3] / 2, b2[:, 0] + b2[:, 2] / 2, b2[:, 1] + b2[:, 3] / 2
    a_1, a_2 = (r1 - l1) * (b1 - t1), (r2 - l2) * (bb2 - t2)
    lm, rm, tm, bm = torch.maximum(l1, l2), torch.minimum(r1, r2), torch.maximum(t1, t2), torch.minimum(b1, bb2)
    ai = torch.where((lm < rm) & (tm < bm), (rm - lm) * (bm - tm), torch.zeros_like(a_1))
    au = a_1 + a_2 - ai
    ah = (torch.maximum(r1, r2) - torch.minimum(l1, l2)) * (torch.maximum(b1, bb2) - torch.minimum(t1, t2))
    per = 1.0 - (ai / au - (ah - au) / ah)
    vf = valid.to(a.dtype).flatten()
    return (per * vf).sum() / vf.sum().clamp_min(1.0)


def _detached(trunk_out):
    """A trunk output (Generator / Discriminator `trunk_out`) without its autograd graph."""
    feats, pos = trunk_out
    return [NestedTensor(f.tensors.detach(), f.mask, getattr(f, 'uniform', False)) for f in feats], [p.detach() for p in pos]


def _staged(module):
    body = trunk_body(module)
    return getattr(body, 'stages', None) is not None


def encoder_partner_applies(G, D, background, staged=False, higher_order=False):
    """Whether D's image encoder may run beside G's in a main phase: both modules have the hooks, one background tensor (not a ragged list with
    masks of its own), encoders of the same geometry (hip.rider.eligible: depth, width, heads, feed-forward size), a backward in one piece."""
    gt, dt = getattr(G, 'transformer', None), getattr(D, 'enc_transformer', None)
    if not (hasattr(D, 'encoder_partner') and isinstance(gt, Transformer) and isinstance(dt, Transformer) and isinstance(background, torch.Tensor)):
        return False
    return hrider.eligible(gt.encoder, dt.encoder, 1, 1, staged=staged, higher_order=higher_order)


class Loss:
    def accumulate_gradients(self, phase, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gen_z, gen_c, gain, cur_nimg,
                             trunks=None):
        raise NotImplementedError()


class StyleGAN2Loss(Loss):
    def __init__(self, device, G, D, augment_pipe=None, r1_gamma=0.0, style_mixing_prob=0, pl_weight=0.0, pl_batch_shrink=2,
                 pl_decay=0.01, pl_no_weight_grad=False, blur_init_sigma=0, blur_fade_kimg=0,
                 Dreal_bbox_cls_weight=50.0, Dreal_bbox_rec_weight=500.0, Dreal_text_rec_weight=0.1, Dreal_text_len_rec_weight=2.0,
                 Dreal_im_rec_weight=0.5, Ggen_bbox_rec_weight=100.0, Ggen_bbox_gIoU_weight=4.0, Ggen_overlapping_weight=7.0,
                 Ggen_alignment_weight=17.0, Ggen_z_rec_weight=5.0, Ggen_bbox_cls_weight=50.0, Ggen_text_rec_weight=1.0,
                 Ggen_text_len_rec_weight=1.0, report_fn=None, share_D_trunk=True):
        super().__init__()
        self.device = device
        self.G = G
        self.D = D
        self.augment_pipe = augment_pipe
        self.r1_gamma = r1_gamma
        self.style_mixing_prob = style_mixing_prob
        self.pl_weight = pl_weight
        self.pl_batch_shrink = pl_batch_shrink
        self.pl_decay = pl_decay
        self.pl_no_weight_grad = pl_no_weight_grad
        self.pl_mean = torch.zeros([], device=device)
        self.pl_noise_fn = None       # tests: callable(bbox_fake) -> the noise of loss.py:131 instead of torch.randn_like
        self.w = dict(Dreal_bbox_cls=Dreal_bbox_cls_weight, Dreal_bbox_rec=Dreal_bbox_rec_weight, Dreal_text_rec=Dreal_text_rec_weight,
                      Dreal_text_len_rec=Dreal_text_len_rec_weight, Dreal_im_rec=Dreal_im_rec_weight, Ggen_bbox_rec=Ggen_bbox_rec_weight,
                      Ggen_bbox_gIoU=Ggen_bbox_gIoU_weight, Ggen_overlapping=Ggen_overlapping_weight, Ggen_alignment=Ggen_alignment_weight,
                      Ggen_z_rec=Ggen_z_rec_weight, Ggen_bbox_cls=Ggen_bbox_cls_weight, Ggen_text_rec=Ggen_text_rec_weight,
                      Ggen_text_len_rec=Ggen_text_len_rec_weight)
        # Dmain evaluates D on the generated and on the real layout of the SAME backgrounds with the SAME weights; D's ResNet
        # trunk is deterministic, so both passes can read one trunk evaluation and its backward runs once on the summed
        # gradient (the reference recomputes it, training/loss.py:176-210: two run_D calls, two backward calls).  Same losses and
        # gradients up to fp32 summation order; share_D_trunk=False restores the reference's call pattern.
        self.share_D_trunk = share_D_trunk
        # with a shared trunk, D(fake) and D(real) of Dmain also run as one batch of 2B (values identical)
        self.pair_D_passes = bool(share_D_trunk) and hasattr(D, 'forward_pair')
        # share_D_trunk='iteration' goes one step further: D's weights do not change between the Gmain and the Dmain phase of one
        # iteration (Gmain updates G only, training_loop.py:281-313), so ONE trunk evaluation per iteration serves D(fake) in Gmain
        # (values only: D is frozen there) and both D passes of Dmain (with its autograd graph).  The iteration driver gets it from
        # precompute_D_trunk() before the phases and hands it to them (accumulate_gradients(trunks=)); without it the per-phase behaviour
        # above applies.
        self.backward_staged = False      # set by training_loop.staged_backward while a phase whose backward runs in stages is evaluated
        self._enc_plan = {}      # detr_transformer.EncoderPartner: the measured place of D's image encoder in each main phase's seed sequence
        self._reporting = report_fn is not None   # the sign() statistics cost a launch each: only formed when someone listens
        self.report = report_fn if report_fn is not None else (lambda name, value: None)
        self.last = {}

    def precompute_D_trunk(self, background, stages=None):
        """share_D_trunk='iteration': D's trunk on `background` with gradient tracking, evaluated once for this iteration's phases, and G's trunk
        for the Gmain phase beside it (grouped_trunks) -> (G's trunk output or None, D's): what accumulate_gradients(trunks=) takes.  None in the
        other share modes.  stages: a detr_backbone.BackwardStages that records D's trunk cuts (Dmain's staged backward continues from them); G's
        trunk is then left to Gmain."""
        if self.share_D_trunk != 'iteration' or not hasattr(self.D, 'trunk'):
            return None
        body = self.D.backbone[0].body
        trunk_params = [p for m in (self.G, self.D) if hasattr(m, 'backbone') for p in m.backbone.parameters()]
        was = [p.requires_grad for p in trunk_params]
        for p in trunk_params:
            p.requires_grad_(True)     # the autograd graphs are built now, used by the phases' backward passes (training_loop.py:282 sets it there)
        try:
            if stages is not None:
                body.stages = stages
            with torch.enable_grad():
                g_out, d_out = self.grouped_trunks(background)
                return g_out, (d_out if d_out is not None else self.D.trunk(background))
        finally:
            if stages is not None:
                body.stages = None
            for p, w in zip(trunk_params, was):
                p.requires_grad_(w)

    def grouped_trunks(self, background):
        """(G's, D's) trunk output on `background` (networks_detr `trunk_out`), every plane-format convolution of the two trunks as one grouped launch
        (detr_backbone.dual_trunk_forward); each module's autograd graph is built by its own replayed forward, so a frozen module gets none.
        (None, None) where grouping does not apply -- ragged backgrounds, a staged backward's cuts, the trunk off the plane-format engine --: each
        forward then evaluates its own trunk."""
        g_body, d_body = trunk_body(self.G), trunk_body(self.D)
        if (not isinstance(background, torch.Tensor) or not isinstance(g_body, ResNet50Body) or type(d_body) is not type(g_body)
                or g_body.stages is not None or d_body.stages is not None):
            return None, None
        outs = dual_trunk_forward(g_body, d_body, background, background)
        if outs is None:
            return None, None
        return self.G.trunk(background, body_out=outs[0]), self.D.trunk(background, body_out=outs[1])

    def run_G(self, z, bbox_class, bbox_real, bbox_text, bbox_patch, padding_mask, background, c, reconst=False, update_emas=False, trunk_out=None,
              enc_partner=None):
        kw = {} if trunk_out is None else dict(trunk_out=trunk_out)
        if enc_partner is not None:
            kw['enc_partner'] = enc_partner
        if not reconst:
            return self.G(z, bbox_class, bbox_real, bbox_text, bbox_patch, padding_mask, background, c, **kw)
        return self.G(z, bbox_class, bbox_real, bbox_text, bbox_patch, padding_mask, background, c, reconst, **kw)

    def run_D(self, bbox, bbox_class, bbox_text, bbox_patch, padding_mask, background, c, reconst=False, blur_sigma=0, update_emas=False,
              trunk_out=None, enc_memory=None):
        kw = {} if trunk_out is None else dict(trunk_out=trunk_out)
        if enc_memory is not None:
            kw['enc_memory'] = enc_memory
        if not reconst:
            return self.D(bbox, bbox_class, bbox_text, bbox_patch, padding_mask, background, c, **kw)
        return self.D(bbox, bbox_class, bbox_text, bbox_patch, padding_mask, background, c, reconst, **kw)

    def g_main_loss(self, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, gain=1.0, trunks=None):
        """trunks: (G's, D's) trunk output of precompute_D_trunk; D's is read without its graph (D is frozen in this phase).  None: both trunks are
        evaluated here, grouped."""
        w = self.w
        valid = ~padding_mask
        static = bool(getattr(self.G, 'static_shapes', False))
        g_trunk, d_trunk = self.grouped_trunks(background) if trunks is None else (trunks[0], _detached(trunks[1]))
        # D's image encoder needs nothing G computes (only D's decoder sees the generated boxes): it rides on G's, one launch per step for both
        partner = self.encoder_partner('Gmain', d_trunk, background)
        bbox_fake, loss_z, cls_logits, loss_lm, loss_text_len = self.run_G(gen_z, bbox_class, bbox_real, bbox_text, bbox_patch, padding_mask, background, gen_c,
                                                                           reconst=True, trunk_out=g_trunk, enc_partner=partner)
        gen_logits, gen_logits_uncond = self.run_D(bbox_fake, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_c, trunk_out=d_trunk,
                                                   enc_memory=partner)
        T = hl.Term
        lay = None
        if static and bbox_fake.is_cuda and bbox_fake.shape[1] <= 64:
            # one launch for the four layout terms and their gradients (csrc/layout_loss.hip) instead of ~280 elementwise ones
            lay = layout_losses_per_sample(bbox_fake, bbox_real, valid)
        elif static:
            l_rec, l_giou = _masked_mse(bbox_fake, bbox_real, valid), _masked_giou(bbox_fake, bbox_real, valid)
            l_ovl, l_aln = compute_overlap(bbox_fake, valid), compute_alignment(bbox_fake, valid)
        else:
            l_rec, l_giou = F.mse_loss(bbox_fake[valid], bbox_real[valid]), generalized_iou_loss(bbox_fake[valid], bbox_real[valid])
            l_ovl, l_aln = compute_overlap(bbox_fake, valid), compute_alignment(bbox_fake, valid)
        self.report('Loss/scores/fake', gen_logits)
        if self._reporting:
            self.report('Loss/signs/fake', gen_logits.sign())
        # the whole tail -- softplus of the two scores, the weights, the sum over the terms, the batch mean and the gain -- and its backward as one
        # launch per direction (hip.losses.combine) instead of ~30 + ~40 scalar-sized ATen launches
        terms = [T('loss_Ggen', gen_logits, 1.0, hl.SOFTPLUS_NEG), T('loss_Ggen_uncond', gen_logits_uncond, 1.0, hl.SOFTPLUS_NEG)]
        if lay is not None:
            terms.append(T(['loss_Ggen_bbox_rec', 'loss_Ggen_bbox_gIoU', 'loss_Ggen_overlapping', 'loss_Ggen_alignment'], lay,
                           [w['Ggen_bbox_rec'], w['Ggen_bbox_gIoU'], w['Ggen_overlapping'], w['Ggen_alignment']], hl.IDENT, [True, True, False, False]))
        else:
            terms += [T('loss_Ggen_bbox_rec', l_rec, w['Ggen_bbox_rec']), T('loss_Ggen_bbox_gIoU', l_giou, w['Ggen_bbox_gIoU']),
                      T('loss_Ggen_overlapping', l_ovl, w['Ggen_overlapping']), T('loss_Ggen_alignment', l_aln, w['Ggen_alignment'])]
        terms.append(T('loss_Ggen_z_rec', loss_z, w['Ggen_z_rec']))
        if static:
            terms.append(T('loss_Ggen_bbox_cls', _masked_ce(cls_logits, bbox_class, valid), w['Ggen_bbox_cls'], hl.RATIO))
        else:
            terms.append(T('loss_Ggen_bbox_cls', F.cross_entropy(cls_logits, bbox_class[valid]), w['Ggen_bbox_cls']))
        terms += [T('loss_Ggen_text_rec', loss_lm, w['Ggen_text_rec']), T('loss_Ggen_text_len_rec', loss_text_len, w['Ggen_text_len_rec'])]
        total, rep = hl.combine(terms, gain)
        for k, v in rep.items():
            self.report('Loss/G/' + k, v)
        self.last = dict(bbox_fake=bbox_fake.detach(), **{k: v.detach() for k, v in rep.items()})
        return total

    def encoder_partner(self, phase, d_trunk, background, pair=False):
        """D's image encoder on its trunk output as the partner of G's in a main phase (detr_transformer.EncoderPartner: handed to G's forward, which
        evaluates both encoders in lock-step, then to D's, which collects its memory), or None where the phases keep the two encoder passes apart:
        no trunk output in hand, ragged backgrounds, a staged backward, a twice-differentiable regulariser pass, modules without the hooks,
        LDETR_DEBUG="ENC_RIDER=0"."""
        # staged: training_loop.staged_backward says so (backward_staged); a trunk body that is recording cuts says the same for drivers of their own
        staged = self.backward_staged or _staged(self.G) or _staged(self.D)
        if d_trunk is None or not encoder_partner_applies(self.G, self.D, background, staged=staged, higher_order=composite.active()):
            return None
        return self.D.encoder_partner(d_trunk, self._enc_plan, (phase, tuple(background.shape), self.G.training, self.D.training), pair=pair)

    def _generate_for_D(self, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, trunk_out=None, enc_partner=None):
        """G's layouts for a D phase (loss.py:146-149) and D's trunk output on the backgrounds: `trunk_out` if given, else evaluated here grouped with
        G's trunk (grouped_trunks; None where that does not apply: D then evaluates its own) -> (bbox_fake, D's trunk_out)."""
        g_trunk = None
        if trunk_out is None:
            g_trunk, trunk_out = self.grouped_trunks(background)
        bbox_fake = self.run_G(gen_z, bbox_class, bbox_real, bbox_text, bbox_patch, padding_mask, background, gen_c, update_emas=True, trunk_out=g_trunk,
                               enc_partner=enc_partner)
        return bbox_fake, trunk_out

    def d_gen_terms(self, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, trunk_out=None, gen_out=None):
        """-> the terms of loss.py:146-160 (D on the generated layout) as hip.losses.Term objects."""
        if gen_out is None:
            bbox_fake, trunk_out = self._generate_for_D(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, trunk_out)
            gen_out = self.run_D(bbox_fake, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_c, update_emas=True, trunk_out=trunk_out)
        gen_logits, gen_logits_uncond = gen_out
        self.report('Loss/scores/fake', gen_logits)
        if self._reporting:
            self.report('Loss/signs/fake', gen_logits.sign())
        return [hl.Term('loss_Dgen', gen_logits, 1.0, hl.SOFTPLUS), hl.Term('loss_Dgen_uncond', gen_logits_uncond, 1.0, hl.SOFTPLUS)]

    def d_real_terms(self, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, trunk_out=None, real_out=None):
        """-> the terms of loss.py:162-218 (D on the real layout with the reconstruction heads)."""
        w = self.w
        valid = ~padding_mask
        static = bool(getattr(self.D, 'static_shapes', False))
        bbox_real_tmp = bbox_real.detach()
        if real_out is None:
            real_out = self.run_D(bbox_real_tmp, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, reconst=True, trunk_out=trunk_out)
        (real_logits, real_logits_uncond, bbox_rec, cls_logits, loss_lm, loss_text_len, bg_rec, bbox_rec_uncond, cls_logits_uncond) = real_out
        T = hl.Term

        def ce(logits):
            if static:
                return dict(x=_masked_ce(logits, bbox_class, valid), fn=hl.RATIO)
            return dict(x=F.cross_entropy(logits, bbox_class[valid]))
        mse = (lambda a: _masked_mse(a, bbox_real_tmp, valid)) if static else (lambda a: F.mse_loss(a, bbox_real_tmp[valid]))
        self.report('Loss/scores/real', real_logits)
        if self._reporting:
            self.report('Loss/signs/real', real_logits.sign())
        return [T('loss_Dreal', real_logits, 1.0, hl.SOFTPLUS_NEG), T('loss_Dreal_uncond', real_logits_uncond, 1.0, hl.SOFTPLUS_NEG),
                T('loss_Dreal_bbox_rec', mse(bbox_rec), w['Dreal_bbox_rec']), T('loss_Dreal_bbox_cls', weight=w['Dreal_bbox_cls'], **ce(cls_logits)),
                T('loss_Dreal_text_rec', loss_lm, w['Dreal_text_rec']), T('loss_Dreal_text_len_rec', loss_text_len, w['Dreal_text_len_rec']),
                T('loss_Dreal_bg_rec', F.mse_loss(bg_rec, background), w['Dreal_im_rec']),
                T('loss_Dreal_bbox_rec_uncond', mse(bbox_rec_uncond), w['Dreal_bbox_rec']),
                T('loss_Dreal_bbox_cls_uncond', weight=w['Dreal_bbox_cls'], **ce(cls_logits_uncond))]

    def _finish(self, terms, prefix, gain=1.0):
        """sum of the terms -> batch mean -> x gain (loss.py:213, 253 + the .mul(gain) of :116, 160, 218), every term reported like the reference does:
        one launch per direction for all of it (hip.losses.combine)."""
        total, rep = hl.combine(terms, gain)
        for k, v in rep.items():
            self.report(prefix + k, v)
        return total

    def d_gen_loss(self, *args, gain=1.0, **kwargs):
        return self._finish(self.d_gen_terms(*args, **kwargs), 'Loss/D/', gain)

    def d_real_loss(self, *args, gain=1.0, **kwargs):
        return self._finish(self.d_real_terms(*args, **kwargs), 'Loss/D/', gain)

    def accumulate_gradients(self, phase, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gen_z, gen_c, gain, cur_nimg,
                             trunks=None):
        """trunks: this micro-batch's (G's, D's) trunk output of precompute_D_trunk, read by the main phases (Gmain: both, D's without its graph;
        Dmain: D's, its backward included).  None: each phase evaluates the trunks it needs itself."""
        assert phase in ['Gmain', 'Greg', 'Gboth', 'Dmain', 'Dreg', 'Dboth']
        if self.pl_weight == 0:
            phase = {'Greg': 'none', 'Gboth': 'Gmain'}.get(phase, phase)
        if self.r1_gamma == 0:
            phase = {'Dreg': 'none', 'Dboth': 'Dmain'}.get(phase, phase)
        if isinstance(background, torch.Tensor) and background.is_cuda:
            core.zero_arena_begin(background.device)      # one fill for the phase's small accumulation targets (hip.core._ZeroArena)
        try:
            self._run_phase(phase, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gen_z, gen_c, gain, trunks)
        finally:
            core.zero_arena_end()

    def g_pl_loss(self, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, gain=1.0):
        """Path-length regularisation (loss.py:119-142): the first `batch / pl_batch_shrink` samples, || d(bbox_fake . noise) / d z || against
        its running mean.  G's heads and layout decoder run on hip/composite.py (differentiated twice)."""
        bs = gen_z.shape[0] // self.pl_batch_shrink
        z = gen_z[:bs].detach().requires_grad_(True)
        with composite.higher_order():
            bbox_fake = self.run_G(z, bbox_class[:bs], bbox_real[:bs], bbox_text[:bs], bbox_patch[:bs], padding_mask[:bs], background[:bs], gen_c[:bs])
        noise = self.pl_noise_fn(bbox_fake) if self.pl_noise_fn is not None else torch.randn_like(bbox_fake)
        pl_noise = noise / float(bbox_fake.shape[2])
        pl_grads = torch.autograd.grad(outputs=[(bbox_fake * pl_noise).sum()], inputs=[z], create_graph=True, only_inputs=True)[0]
        pl_lengths = pl_grads.square().sum([1, 2]).sqrt()
        pl_mean = self.pl_mean.lerp(pl_lengths.mean(), self.pl_decay)
        self.pl_mean.copy_(pl_mean.detach())
        pl_penalty = (pl_lengths - pl_mean).square()
        self.report('Loss/pl_penalty', pl_penalty)
        loss_Gpl = pl_penalty * self.pl_weight
        self.report('Loss/G/reg', loss_Gpl)
        self.last = dict(pl_penalty=pl_penalty.detach(), pl_lengths=pl_lengths.detach(), pl_grads=pl_grads.detach())
        return loss_Gpl.mean().mul(gain)

    def d_r1_loss(self, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gain=1.0):
        """R1 (loss.py:162-166, 207-217 in phase 'Dreg'): gamma / 2 * || d D(real) / d bbox_real ||^2 per sample.  The reference evaluates
        D with reconst=True here and discards the seven reconstruction outputs; only the conditional score is formed.  D's `fc_bbox`,
        `enc_fc_in`, layout decoder and `fc_out_disc` run on hip/composite.py (differentiated twice)."""
        bbox_real_tmp = bbox_real.detach().requires_grad_(True)
        with composite.higher_order():
            real_logits, _ = self.run_D(bbox_real_tmp, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c)
        self.report('Loss/scores/real', real_logits)
        if self._reporting:
            self.report('Loss/signs/real', real_logits.sign())
        r1_grads = torch.autograd.grad(outputs=[real_logits.sum()], inputs=[bbox_real_tmp], create_graph=True, only_inputs=True)[0]
        r1_penalty = r1_grads.square().sum([1, 2])
        loss_Dr1 = r1_penalty * (self.r1_gamma / 2)
        self.report('Loss/r1_penalty', r1_penalty)
        self.report('Loss/D/reg', loss_Dr1)
        self.last = dict(r1_penalty=r1_penalty.detach(), r1_grads=r1_grads.detach(), real_logits=real_logits.detach())
        return loss_Dr1.mean().mul(gain)

    def _run_phase(self, phase, bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gen_z, gen_c, gain, trunks):
        # 'Gboth' / 'Dboth' (no lazy regularisation: reg_interval None) = the main phase, then the regulariser on a forward pass of its own.
        # The reference shares Dreal's forward with R1 in 'Dboth' (loss.py:162-217): same expected gradient, independent dropout draws here.
        if phase in ('Greg', 'Gboth'):
            if phase == 'Gboth':
                self._run_phase('Gmain', bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gen_z, gen_c, gain, trunks)
            self.g_pl_loss(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, gain=gain).backward()
        if phase in ('Dreg', 'Dboth'):
            if phase == 'Dboth':
                self._run_phase('Dmain', bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gen_z, gen_c, gain, trunks)
            self.d_r1_loss(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gain=gain).backward()
        if phase == 'Gmain':
            self.g_main_loss(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, gain=gain, trunks=trunks).backward()
        if phase == 'Dmain':
            if self.share_D_trunk and hasattr(self.D, 'trunk'):   # True / 'phase' / 'iteration'
                # the phase's one D-trunk evaluation (with the generator's no-grad trunk grouped beside it), unless the iteration's is handed in
                # D's (trained, 2B-row) image encoder is evaluated beside the no-grad generator's; forward_pair collects its memory, graph included
                partner = self.encoder_partner('Dmain', trunks[1], background, pair=True) if (trunks is not None and self.pair_D_passes) else None
                bbox_fake, trunk = self._generate_for_D(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c,
                                                        None if trunks is None else trunks[1], enc_partner=partner)
                if self.pair_D_passes:
                    # both D passes of the phase as ONE batch of 2B layouts (Discriminator.forward_pair): half the transformer / head launches
                    gen_out, real_out = self.D.forward_pair(bbox_fake, bbox_real.detach(), bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c,
                                                            trunk_out=trunk, **({} if partner is None else dict(enc_memory=partner)))
                else:
                    trunk = trunk if trunk is not None else self.D.trunk(background)
                    gen_out = self.run_D(bbox_fake, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_c, update_emas=True, trunk_out=trunk)
                    real_out = None
                t_gen = self.d_gen_terms(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, gen_out=gen_out)
                t_real = self.d_real_terms(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, trunk_out=trunk, real_out=real_out)
                # one backward: the trunk sees the summed gradient of both passes; mean(gen terms) + mean(real terms) = one combine over all of them
                self._finish(t_gen + t_real, 'Loss/D/', gain).backward()
            else:
                # reference call pattern: D(fake) groups its trunk with the generator's (d_gen_terms); D(real) evaluates its own
                self.d_gen_loss(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, gen_z, gen_c, gain=gain).backward()
                self.d_real_loss(bbox_real, bbox_class, bbox_text, bbox_patch, padding_mask, background, real_c, gain=gain).backward()
