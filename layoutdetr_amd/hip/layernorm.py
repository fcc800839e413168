"""y = LayerNorm(x + dropout(residual)) fused into one forward and one backward launch.
Reference chain: training/detr_transformer.py:210-214 / 275-285 (post-norm blocks, eps 1e-5)."""
import torch

from . import blocks, core


class _AddLnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps, p_drop, pos=None):
        core.require_gpu(x, r, gamma, beta, pos)
        ctx.set_materialize_grads(False)
        D = x.shape[-1]
        x2 = core.f32c(x.reshape(-1, D))
        r2 = core.f32c(r.reshape(-1, D)) if r is not None else None
        g, b = core.f32c(gamma), core.f32c(beta)
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        z = torch.empty_like(x2) if r2 is not None else None      # without a residual the pre-norm sum is x itself
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
        if r2 is None:
            p_drop = 0.0
        seed = blocks.draw_seed(p_drop)
        pos2 = core.f32c(pos.reshape(-1, D)) if pos is not None else None
        ypos = torch.empty_like(x2) if pos2 is not None else None
        blocks.launch('layernorm_fwd', [blocks.ln_fwd(x2, r2, g, b, eps, p_drop, seed, y, z, mean, rstd, pos=pos2, ypos=ypos)])
        ctx.save_for_backward(z if z is not None else x2, mean, rstd, g)
        ctx.cfg = (x.shape, r is not None, p_drop, seed, D)
        ctx.params = (gamma, beta)
        if pos is not None:
            return y.reshape(x.shape), ypos.reshape(x.shape)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy, dypos=None):
        z, mean, rstd, g = ctx.saved_tensors
        xshape, has_r, p_drop, seed, D = ctx.cfg
        if dy is None and dypos is None:
            return (None,) * 7
        if dy is None:
            dy, dypos = dypos, None
        dy2 = core.f32c(dy.reshape(-1, D))
        dyp = core.f32c(dypos.reshape(-1, D)) if dypos is not None else None
        need_x, need_r = ctx.needs_input_grad[0], has_r and ctx.needs_input_grad[1]
        need_g = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        dx = torch.empty_like(dy2)
        dr = None
        if need_r:
            dr = torch.empty_like(dy2) if p_drop > 0 else dx
        gg, gbt = core.flat_grad(ctx.params[0]), core.flat_grad(ctx.params[1])
        fused = need_g and gg is not None and gbt is not None
        if fused:
            dgamma, dbeta = gg, gbt          # the kernel's atomics accumulate straight into the flat .grad views
        else:
            dgamma = torch.zeros(D, device=dy2.device, dtype=torch.float32) if need_g else None
            dbeta = torch.zeros(D, device=dy2.device, dtype=torch.float32) if need_g else None
        blocks.launch('layernorm_bwd', [blocks.ln_bwd(dy2, z, mean, rstd, g, dx, dr if (need_r and p_drop > 0) else None, dgamma, dbeta, p_drop, seed, dy2=dyp)])
        if fused:
            dgamma = dbeta = None
        return (dx.reshape(xshape) if need_x else None, dr.reshape(xshape) if need_r else None, dgamma, dbeta, None, None, None)


def add_layernorm(x, residual, gamma, beta, eps=1e-5, p_drop=0.0, pos=None):
    """LayerNorm(x + dropout(residual)); residual may be None (plain LayerNorm).
    pos ([S, D], rows broadcast over the batch): returns (y, y + pos) — the second tensor is what the next attention block projects
    q / k from, produced by the same launch instead of a separate add; its gradient is summed inside the backward launch."""
    return _AddLnFn.apply(x, residual, gamma, beta, eps, p_drop, pos)
