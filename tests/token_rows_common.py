"""What tests/test_token_rows_ref_cpu.py and tests/test_token_rows_gpu.py share for the token-row kernels (csrc/layernorm.hip: the grouped LayerNorm
forward / backward and ldetr_sum_parts_f32; csrc/xent.hip: the label-smoothed softmax cross entropy and the token embedding gather / scatter):
float64 references written from the formulas of include/ldetr_hip.h, the case tables, and one predicate per family that restates the host-side
selection and names the paths a case takes.  The CPU file asserts that every path name is reached by a table case; the GPU file runs the tables.
Nothing here touches the GPU or the kernel library.

Every reference takes `dtype`: float64 is the reference, float32 is the yardstick for the checks that have no project bound (the same formula
evaluated by torch on the CPU in the kernels' number format; a sum over rows is taken left to right there, as the kernels add their block partials
one atomic at a time).  FP32_BASELINE holds those float32 errors as measured over the tables, the GPU file allows 4 x them (other summation order,
fma contraction, __expf), and the CPU file re-measures them and asserts that each recorded figure is within a factor 4 of what it finds."""
import math
import os

import numpy as np
import torch

from oracle import dropout_ref as DR

F64, F32 = torch.float64, torch.float32


def limit_threads():
    """CPU references: more threads than this are slower on many-core hosts."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel_err(a, b):
    """max |a - b| / max |b|, the suite's measure."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def as_f32(v):
    """A scalar as the C ABI receives it: rounded to float32."""
    return float(torch.tensor(v, dtype=F32))


def seq_sum(t, dtype):
    """Sum over dim 0.  float64: torch's; float32: left to right in float32 (torch's own float32 reductions use wider or cascaded accumulators)."""
    if dtype == F64:
        return t.sum(0)
    acc = torch.zeros(t.shape[1:], dtype=dtype)
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


# Bounds the project already has, in rel_err's measure.
TOL_LN = dict(y=3e-6, grad=1e-5)                       # test_layernorm, dropout_common.TOL_LN
TOL_XENT = dict(loss_rel=2e-6, loss_abs=1e-6, dlogits=2e-5)     # test_softmax_cross_entropy_label_smoothing
TOL_EMB = 2e-5                                         # test_token_embedding_gather_and_scatter

# float32 torch on the CPU against the float64 reference, worst case over the tables below (measure_fp32_baselines; the CPU file re-measures
# them); the GPU file allows FP32_FACTOR x these.  All in rel_err's measure except xent_big_loss_sum, which is |sum32 - sum64| / |sum64|.
#   ln_mean, ln_rstd        row statistics over LN_SHAPE_CASES and the value edges
#   ln_offset_y, _grad      rows offset by +100 with unit spread: y and the worst of dx / dgamma / dbeta
#   ln_big_dgamma, _dbeta   the 2053-row cases
#   xent_x30_loss, _dlogits logits x 30: mean loss and its gradient
#   xent_big_loss_sum       the loss sum over the 2053-row cases (both smoothing values, rows summed first to last and last to first)
FP32_BASELINE = dict(ln_mean=1.33e-6, ln_rstd=1.54e-7, ln_offset_y=2.73e-6, ln_offset_grad=2.83e-6, ln_big_dgamma=1.75e-6, ln_big_dbeta=1.15e-6,
                     xent_x30_loss=7.94e-8, xent_x30_dlogits=6.95e-6, xent_big_loss_sum=8.15e-7)
FP32_FACTOR = 4.0      # -> bounds 5.3e-6, 6.2e-7, 1.1e-5, 1.1e-5, 7.0e-6, 4.6e-6, 3.2e-7, 2.8e-5, 3.3e-6


def fp32_bound(key):
    return FP32_FACTOR * FP32_BASELINE[key]


# ------------------------------------------------------------------------------------------------------------------------ dropout
def drop_rows(host_seed, device_word, p, rows, D):
    """[rows, D] float64: what element row*D + col of the residual branch is multiplied by (0 or 1 / (1 - p)), as dropout_common.Masks.rows."""
    if not p > 0:
        return None
    return torch.from_numpy(np.ascontiguousarray(DR.scale(DR.total_seed(host_seed, device_word), DR.rows_index(rows, D), p))).double()


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-5
LN_MAX_BWD_BLOCKS = 512       # csrc/layernorm.hip:234
LN_ROWS_PER_BLOCK = 4         # one wave per row, four waves per block (csrc/layernorm.hip:22, :113)


def ln_nv(D):
    """float4 vectors per lane: the instantiation the host picks (csrc/layernorm.hip:211, :238)."""
    return (D + 255) // 256


def ln_pw(D):
    """Slices loaded per round of the in-launch partial-sum reduction (csrc/layernorm.hip:42, :128)."""
    return 16 if ln_nv(D) == 1 else 8


def ln_shape_path(rows, D):
    """The instantiation, whether the last vector of a row has idle lanes (csrc/layernorm.hip:33), whether the last block has idle waves (:23) and
    whether the backward's grid is capped so that a wave makes a second sweep (:113, :234)."""
    out = {f'NV{ln_nv(D)}'}
    out.add('idle_lanes' if D // 4 < ln_nv(D) * 64 else 'all_lanes')
    if rows % LN_ROWS_PER_BLOCK:
        out.add('ragged_last_block')
    out.add('bwd_stride_loop' if (rows + 3) // 4 > LN_MAX_BWD_BLOCKS else 'bwd_one_sweep')
    return out


def ln_slices_path(D, slices, direction):
    """The rounds of the slice loop: the forward's starts at slice 1 (slice 0 is loaded as the residual; csrc/layernorm.hip:43), the backward's at
    slice 0 (:129).  slices 0 forward = plain residual, r_bias ignored."""
    pw = ln_pw(D)
    if direction == 'fwd' and slices == 0:
        return {f'fwd/PW{pw}/plain_residual'}
    n = slices - 1 if direction == 'fwd' else slices
    if n == 0:
        return {f'{direction}/PW{pw}/no_round'}
    rounds, tail = (n + pw - 1) // pw, n % pw
    return {f'{direction}/PW{pw}/' + ('one_round' if rounds == 1 else 'many_rounds') + ('_ragged' if tail else '_full')}


def ln_group_path(rows0, rows1):
    out = set()
    if rows0 == 0:
        out.add('first_empty')
    elif rows1 == 0:
        out.add('second_empty')
    else:
        out.add('both')
        if rows0 % LN_ROWS_PER_BLOCK:
            out.add('first_last_block_idle_waves')
        if (rows1 + 3) // 4 > LN_MAX_BWD_BLOCKS:
            out.add('second_bwd_stride_loop')
    return out


LN_DS = [4, 64, 256, 260, 512, 516, 768, 1024]
LN_SHAPE_CASES = [(rows, D) for D in LN_DS for rows in (1, 5, 18)] + [(2053, 256), (2053, 1024)]
LN_SHAPE_PATHS = ['NV1', 'NV2', 'NV3', 'NV4', 'idle_lanes', 'all_lanes', 'ragged_last_block', 'bwd_stride_loop', 'bwd_one_sweep']
LN_SHAPE_P = 0.1
# (D, slices); every one runs with and without r_bias (forward) / dy2 (backward) and with p_drop 0 and 0.3
LN_FWD_SLICE_CASES = [(256, s) for s in (0, 1, 2, 8, 16, 17, 18, 32, 33)] + [(512, s) for s in (1, 8, 9, 10, 17)]
LN_BWD_SLICE_CASES = [(256, s) for s in (0, 1, 8, 15, 16, 17, 32)] + [(768, s) for s in (0, 7, 8, 9, 16)]
LN_SLICE_ROWS = 5
LN_SLICE_P = 0.3
LN_SLICE_PATHS = [f'fwd/PW{pw}/{k}' for pw in (16, 8) for k in ('no_round', 'one_round_ragged', 'one_round_full', 'many_rounds_ragged', 'many_rounds_full')] + \
                 ['fwd/PW16/plain_residual'] + \
                 [f'bwd/PW{pw}/{k}' for pw in (16, 8) for k in ('no_round', 'one_round_ragged', 'one_round_full', 'many_rounds_ragged', 'many_rounds_full')]
# (rows of the first problem, rows of the second); the members differ in slice count and p_drop (LN_GROUP_MEMBERS: forward slices, backward
# slices, p_drop)
LN_GROUP_CASES = [(18, 37), (5, 2053), (0, 9), (9, 0)]
LN_GROUP_MEMBERS = [dict(fwd_slices=8, bwd_slices=3, p=0.1), dict(fwd_slices=2, bwd_slices=9, p=0.25)]
LN_GROUP_D = 256
LN_GROUP_PATHS = ['both', 'first_empty', 'second_empty', 'first_last_block_idle_waves', 'second_bwd_stride_loop']
LN_POS_ROWS = [9, 7, 1]       # at 18 rows: divides, does not divide, one row for all
LN_OPTIONAL_NULL = ['z', 'mean', 'rstd', 'dx', 'dgamma_with_dr']
LN_OPT_ROWS, LN_OPT_D = 18, 256


def ln_inputs(rows, D, fwd_slices=0, bwd_slices=0, pos_rows=0, seed=0, offset=0.0):
    """float32 inputs of one LayerNorm problem, both directions.  r [max(fwd_slices, 1), rows, D]; parts [bwd_slices, rows, D]; dg0 / db0: running
    gradients dgamma / dbeta start from."""
    g = torch.Generator().manual_seed(2100 + 7 * rows + D + 131 * fwd_slices + 17 * bwd_slices + 1009 * seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(x=rn(rows, D) + offset, r=rn(max(fwd_slices, 1), rows, D), r_bias=rn(D), gamma=torch.rand(D, generator=g) + 0.5, beta=rn(D),
             dy=rn(rows, D), dy2=rn(rows, D), parts=rn(max(bwd_slices, 1), rows, D)[:bwd_slices], dg0=rn(D), db0=rn(D))
    if pos_rows:
        t['pos'] = rn(pos_rows, D)
    return t


def _stats(z, eps):
    mean = z.mean(1)
    zc = z - mean[:, None]
    rstd = ((zc * zc).mean(1) + eps).rsqrt()       # two passes: the mean first, then the spread around it
    return mean, zc, rstd


def ln_fwd_ref(x, r, gamma, beta, r_parts=0, r_bias=None, drop=None, pos=None, eps=LN_EPS, dtype=F64, pos_index='mod'):
    """include/ldetr_hip.h: z = x + drop * r, where r_parts > 0 makes r the sum (r[0] + r_bias) + r[1] + ... + r[r_parts - 1] in that order and
    r_parts = 0 the plain residual r (r_bias ignored; r None: z = x);  y = (z - mean) * rstd * gamma + beta;  ypos = y + pos[row % pos_rows].
    pos_index 'div': the WRONG row // (rows / pos_rows) the CPU file shows the bound to reject.  -> dict(z, y, mean, rstd[, ypos])"""
    eps = as_f32(eps)
    z = x.to(dtype)
    rows = z.shape[0]
    if r is not None:
        r = r.to(dtype)
        rr = r[0] if r.dim() == 3 else r
        if r_parts > 0:
            if r_bias is not None:
                rr = rr + r_bias.to(dtype)
            for s in range(1, r_parts):
                rr = rr + r[s]
        if drop is not None:
            rr = rr * drop.to(dtype)
        z = z + rr
    mean, zc, rstd = _stats(z, eps)
    y = zc * rstd[:, None] * gamma.to(dtype) + beta.to(dtype)
    out = dict(z=z, y=y, mean=mean, rstd=rstd)
    if pos is not None:
        pr = pos.shape[0]
        idx = torch.arange(rows) % pr if pos_index == 'mod' else (torch.arange(rows) // max(rows // pr, 1)).clamp(max=pr - 1)
        out['ypos'] = y + pos.to(dtype)[idx]
    return out


def ln_bwd_total_dy(dy, dy2=None, parts=None, n_parts=0, dtype=F64):
    """dy (+ dy2) + parts[0] + ... in slice order (csrc/layernorm.hip:123-137)."""
    d = dy.to(dtype)
    if dy2 is not None:
        d = d + dy2.to(dtype)
    for s in range(n_parts):
        d = d + parts[s].to(dtype)
    return d


def ln_bwd_ref(z, gamma, dy, dy2=None, parts=None, n_parts=0, drop=None, dg0=None, db0=None, eps=LN_EPS, dtype=F64):
    """Closed form (csrc/layernorm.hip:97): with d the total incoming gradient, g = d * gamma, xh = (z - mean) * rstd:
    dx = rstd * (g - mean(g) - xh * mean(g * xh));  dr = dx * drop;  dgamma = dg0 + sum_rows d * xh;  dbeta = db0 + sum_rows d."""
    eps = as_f32(eps)
    z = z.to(dtype)
    d = ln_bwd_total_dy(dy, dy2, parts, n_parts, dtype)
    _, zc, rstd = _stats(z, eps)
    xh = zc * rstd[:, None]
    g = d * gamma.to(dtype)
    dx = rstd[:, None] * (g - g.mean(1)[:, None] - xh * (g * xh).mean(1)[:, None])
    dr = dx * drop.to(dtype) if drop is not None else dx
    dgamma, dbeta = seq_sum(d * xh, dtype), seq_sum(d, dtype)
    if dg0 is not None:
        dgamma, dbeta = dg0.to(dtype) + dgamma, db0.to(dtype) + dbeta
    return dict(dx=dx, dr=dr, dgamma=dgamma, dbeta=dbeta)


def ln_autograd_ref(t, r_parts=0, use_bias=False, drop=None, use_dy2=False, n_parts=0, eps=LN_EPS):
    """The same quantities by torch's float64 autograd through F.layer_norm of the explicitly formed sum -> dict(y, dx, dr (of every slice used),
    dgamma, dbeta); t: ln_inputs."""
    x, r, gm, bt = [t[k].double().clone().requires_grad_(True) for k in ('x', 'r', 'gamma', 'beta')]
    rr = r[0]
    if r_parts > 0:
        if use_bias:
            rr = rr + t['r_bias'].double()
        for s in range(1, r_parts):
            rr = rr + r[s]
    if drop is not None:
        rr = rr * drop
    z = x + rr
    y = torch.nn.functional.layer_norm(z, (x.shape[1],), gm, bt, as_f32(eps))
    d = t['dy'].double()
    if use_dy2:
        d = d + t['dy2'].double()
    for s in range(n_parts):
        d = d + t['parts'][s].double()
    y.backward(d)
    return dict(y=y.detach(), z=z.detach(), dx=x.grad, dr=r.grad[:max(r_parts, 1)], dgamma=gm.grad, dbeta=bt.grad)


# ------------------------------------------------------------------------------------------------------------------------ sum_parts
SUM_MAX_BLOCKS = 1024         # csrc/layernorm.hip:268
SUM_ROUND = 8                 # csrc/layernorm.hip:251
SUM_NS = [4, 1028, 1024 * 256 * 4 + 148]
SUM_SLICES = [0, 1, 7, 8, 9, 16, 17]
SUM_STRIDE_PAD = [0, 64]
SUM_PATHS = ['single_sweep', 'grid_stride', 'no_slices', 'one_round_ragged', 'one_round_full', 'many_rounds_ragged', 'many_rounds_full']


def sum_parts_path(n, slices):
    out = {'grid_stride' if n // 4 > SUM_MAX_BLOCKS * 256 else 'single_sweep'}
    if slices == 0:
        out.add('no_slices')
    else:
        rounds, tail = (slices + SUM_ROUND - 1) // SUM_ROUND, slices % SUM_ROUND
        out.add(('one_round' if rounds == 1 else 'many_rounds') + ('_ragged' if tail else '_full'))
    return out


def sum_parts_inputs(n):
    """base [n] and parts [17, n + 64] (a case uses the first `slices` rows with the pitch n or n + 64)."""
    g = torch.Generator().manual_seed(3100 + n % 1000)
    return torch.randn(n, generator=g), torch.randn(max(SUM_SLICES), n + max(SUM_STRIDE_PAD), generator=g)


def sum_parts_ref(base, parts, slices, n, dtype=F64):
    """out = base (or 0) + parts[0] + parts[1] + ..., in slice order (include/ldetr_hip.h: ldetr_sum_parts_f32); parts [S, n]."""
    v = base.to(dtype) if base is not None else torch.zeros(n, dtype=dtype)
    for s in range(slices):
        v = v + parts[s][:n].to(dtype)
    return v


# ------------------------------------------------------------------------------------------------------------------------ cross entropy
XENT_MAX_BLOCKS = 1024        # csrc/xent.hip:169
XENT_THREADS = 256
XENT_IGNORE = -100
XENT_G = 2.5                  # the upstream gradient
XENT_SHAPES = [(5, 1, 3), (5, 3, 1), (37, 70, 2), (9, 1023, 1), (9, 1028, 64), (1030, 70, 2), (2053, 258, 2), (37, 30524, 0)]       # (rows, V, ld - V)
XENT_EPS = [0.0, 0.1]
XENT_BIG_ROWS = 2053
XENT_X30 = (37, 70, 90.0)     # rows, V, spread of the logits: 30 x the other cases' 3
XENT_PATHS = ['no_vector_part', 'vector_and_tail', 'vector_only', 'idle_threads', 'all_threads', 'second_quad_per_thread',
              'one_row_per_block', 'second_row_per_block', 'third_row_per_block', 'dense_or_padded_pitch', 'pitch_beyond_padding']


def xent_path(rows, V, pad):
    """xent_fwd_kernel (csrc/xent.hip:33-84): the float4 part (:42) and the scalar tail (:50), threads that see no logit and carry (-inf, 0) into
    the merge, rows dealt round-robin to at most 1024 blocks (:35, :169), the row pitch."""
    v4 = V // 4
    out = {'no_vector_part' if v4 == 0 else ('vector_and_tail' if V % 4 else 'vector_only')}
    out.add('idle_threads' if max(v4, V % 4) < XENT_THREADS else 'all_threads')
    if v4 > XENT_THREADS:
        out.add('second_quad_per_thread')
    per_block = (rows + XENT_MAX_BLOCKS - 1) // XENT_MAX_BLOCKS
    out.add({1: 'one_row_per_block', 2: 'second_row_per_block'}.get(per_block, 'third_row_per_block'))
    out.add('pitch_beyond_padding' if pad >= 4 else 'dense_or_padded_pitch')
    return out


def xent_inputs(rows, V, kind='mixed', scale=3.0, seed=0):
    """logits [rows, V] float32 and targets: every 4th ignored, from row 2 every 7th negative (-3), from row 3 every 7th V, from row 5 every 11th
    V + 5 (kind 'mixed');  'all_ignored';  'valid': all in range;  'neg_inf': columns 0..7 are -inf in every row, 1024..1027 in the odd rows,
    targets on finite columns."""
    g = torch.Generator().manual_seed(4100 + rows + V + seed)
    x = torch.randn(rows, V, generator=g) * scale
    t = torch.randint(0, V, (rows,), generator=g)
    if kind == 'mixed':
        t[2::7] = -3
        t[3::7] = V
        t[5::11] = V + 5
        t[0::4] = XENT_IGNORE
    elif kind == 'all_ignored':
        t[:] = XENT_IGNORE
    elif kind == 'neg_inf':
        assert V >= 1028
        x[:, :8] = -math.inf
        x[1::2, 1024:1028] = -math.inf
        t = torch.randint(8, 1024, (rows,), generator=g)
    return x, t


def xent_ref(logits, targets, ignore_index, eps, g=1.0, dtype=F64, order='forward'):
    """include/ldetr_hip.h / csrc/xent.hip:6-7: targets outside [0, V) count as ignored; over the other rows
        loss_i = lse_i - (1 - eps) x_i[t_i] - eps mean_c x_i[c]   (no smoothing term at eps = 0, as F.cross_entropy),   loss_sum = sum_i loss_i,
        dlogits[i, c] = (softmax_i[c] - (1 - eps) [c == t_i] - eps / V) g / count, zero rows where ignored (everywhere when count = 0);
    row_lse is 0 on ignored rows.  order: the direction the float32 yardstick adds the rows in.  -> (loss_sum, count, row_lse, dlogits)"""
    eps = as_f32(eps)
    x = logits.to(dtype)
    rows, V = x.shape
    valid = (targets != ignore_index) & (targets >= 0) & (targets < V)
    tt = torch.where(valid, targets, torch.zeros_like(targets))
    lse = torch.logsumexp(x, 1)
    li = lse - (1.0 - eps) * x.gather(1, tt[:, None])[:, 0]
    if eps > 0:
        li = li - eps * x.mean(1)
    li = li[valid]
    if order != 'forward':
        li = li.flip(0)
    loss_sum = seq_sum(li, dtype) if li.numel() else torch.zeros((), dtype=dtype)
    count = int(valid.sum())
    d = torch.zeros_like(x)
    if count:
        onehot = torch.zeros_like(x).scatter_(1, tt[:, None], 1.0)
        d = ((x - lse[:, None]).exp() - (1.0 - eps) * onehot - eps / V) * (g / count)
        d = torch.where(valid[:, None], d, torch.zeros_like(d))
    return loss_sum, count, torch.where(valid, lse, torch.zeros_like(lse)), d


def golden_logits(rows, V):
    """Logits built from integers (multiples of 1/16 in [-8, 8]): the same bits on every host, for the comparison with values recorded from the
    kernel before its -inf guard (tests/golden/xent_guard.npz)."""
    i = torch.arange(rows, dtype=torch.int64)[:, None]
    j = torch.arange(V, dtype=torch.int64)[None, :]
    return (((i * 131 + j * 71 + (i * j) % 13) % 257 - 128).float() / 16.0).contiguous()


def golden_targets(rows, V, only_block0=False):
    """In-range targets; only_block0: all ignored but the rows block 0 of the capped grid owns (0, 1024, 2048, ...), so that exactly one block
    adds to the loss sum and the sum does not depend on the order of the atomics."""
    t = (torch.arange(rows, dtype=torch.int64) * 37 + 11) % V
    if only_block0:
        keep = torch.arange(rows) % XENT_MAX_BLOCKS == 0
        t = torch.where(keep, t, torch.full_like(t, XENT_IGNORE))
    return t


GOLDEN_XENT = dict(rows_lse=1030, rows_sum=2049, V=70, pad=2, eps=0.1)


# ------------------------------------------------------------------------------------------------------------------------ embedding
EMB_FWD_MAX_BLOCKS = 4096     # csrc/xent.hip:195
EMB_BWD_MAX_BLOCKS = 8192     # csrc/xent.hip:207
# (n, T, V, d, kind): 'mixed' ids hold -1, V, V + 5, the padding id 0 and V - 1; 'one_id': every token hits row 1; 'in_range'
EMB_CASES = [(21, 7, 50, 64, 'mixed'), (20, 7, 50, 4, 'mixed'), (1024, 512, 1000, 128, 'mixed'), (4096, 1, 3, 256, 'one_id'), (5800, 40, 1000, 768, 'mixed')]
EMB_PATHS = ['one_quad_per_row', 'many_quads_per_row', 'fwd_single_sweep', 'fwd_grid_stride', 'bwd_single_sweep', 'bwd_grid_stride']


def emb_path(n, T, V, d):
    """embedding_fwd_kernel: one thread per float4 of the output, at most 4096 blocks (csrc/xent.hip:126, :195); embedding_bwd_kernel: one thread per
    element, at most 8192 blocks (:141, :207)."""
    return {'one_quad_per_row' if d == 4 else 'many_quads_per_row',
            'fwd_grid_stride' if n * (d // 4) > EMB_FWD_MAX_BLOCKS * 256 else 'fwd_single_sweep',
            'bwd_grid_stride' if n * d > EMB_BWD_MAX_BLOCKS * 256 else 'bwd_single_sweep'}


def emb_inputs(n, T, V, d, kind):
    g = torch.Generator().manual_seed(5100 + n + T + V + d)
    rn = lambda *s: torch.randn(*s, generator=g)
    ids = torch.randint(0, V, (n,), generator=g)
    if kind == 'one_id':
        ids[:] = 1
    elif kind == 'mixed':
        ids[1], ids[4], ids[7], ids[9], ids[n - 1] = -1, V, V + 5, 0, V - 1
        ids[12::5] = 0
    return dict(ids=ids, w=rn(V, d), pos=rn(T, d), dy=rn(n, d), dw0=rn(V, d))


def embedding_ref(w, ids, pos=None, T=1, padding_idx=-1, dy=None, dw0=None, dtype=F64):
    """include/ldetr_hip.h: out[i] = w[ids[i]] (a zero row when ids[i] is outside [0, V)) + pos[i % T];  dweight = dw0 + sum over the tokens whose
    id is inside [0, V) and is not padding_idx of dy[i] scattered to row ids[i]  (padding_idx -1: no padding row).  -> (out, dweight or None)"""
    w = w.to(dtype)
    V, d = w.shape
    n = ids.numel()
    ok = (ids >= 0) & (ids < V)
    safe = torch.where(ok, ids, torch.zeros_like(ids))
    out = torch.where(ok[:, None], w[safe], torch.zeros(n, d, dtype=dtype))
    if pos is not None:
        out = out + pos.to(dtype)[torch.arange(n) % T]
    dw = None
    if dy is not None:
        use = ok & (ids != padding_idx)
        dw = dw0.to(dtype).clone() if dw0 is not None else torch.zeros(V, d, dtype=dtype)
        dw.index_add_(0, ids[use], dy.to(dtype)[use])
    return out, dw


# ------------------------------------------------------------------------------------------------------------------------ float32 yardstick
LN_EDGE_ROWS, LN_EDGE_D = 18, 256
LN_OFFSET = 100.0


def measure_fp32_baselines():
    """The float32 CPU evaluation of every formula that has no project bound against its float64 evaluation, worst case over the tables
    -> dict like FP32_BASELINE."""
    out = dict.fromkeys(FP32_BASELINE, 0.0)

    def up(key, v):
        out[key] = max(out[key], v)

    def both(fn):
        return fn(F32), fn(F64)
    for rows, D in LN_SHAPE_CASES + [(LN_EDGE_ROWS, LN_EDGE_D)]:
        offset = LN_OFFSET if (rows, D) == (LN_EDGE_ROWS, LN_EDGE_D) else 0.0
        t = ln_inputs(rows, D, offset=offset)
        drop = drop_rows(12345 + rows, 6789 + D, LN_SHAPE_P, rows, D)
        f32, f64 = both(lambda dt: ln_fwd_ref(t['x'], t['r'], t['gamma'], t['beta'], drop=drop, dtype=dt))
        up('ln_mean', rel_err(f32['mean'], f64['mean']))
        up('ln_rstd', rel_err(f32['rstd'], f64['rstd']))
        if offset or rows == 2053:
            # the backward as the kernels run it: from the forward's own z in its number format
            b32, b64 = both(lambda dt: ln_bwd_ref((f32 if dt == F32 else f64)['z'], t['gamma'], t['dy'], drop=drop, dtype=dt))
            if offset:
                up('ln_offset_y', rel_err(f32['y'], f64['y']))
                up('ln_offset_grad', max(rel_err(b32[k], b64[k]) for k in ('dx', 'dgamma', 'dbeta')))
            else:
                up('ln_big_dgamma', rel_err(b32['dgamma'], b64['dgamma']))
                up('ln_big_dbeta', rel_err(b32['dbeta'], b64['dbeta']))
    x, tg = xent_inputs(*XENT_X30[:2], scale=XENT_X30[2])
    for eps in XENT_EPS:
        (s32, n, _, d32), (s64, _, _, d64) = both(lambda dt: xent_ref(x, tg, XENT_IGNORE, eps, XENT_G, dt))
        up('xent_x30_loss', abs(float(s32) / n - float(s64) / n) / abs(float(s64) / n))
        up('xent_x30_dlogits', rel_err(d32, d64))
    rows, V, _ = next(s for s in XENT_SHAPES if s[0] == XENT_BIG_ROWS)
    x, tg = xent_inputs(rows, V)
    for eps in XENT_EPS:
        s64 = float(xent_ref(x, tg, XENT_IGNORE, eps)[0])
        for order in ('forward', 'reverse'):
            up('xent_big_loss_sum', abs(float(xent_ref(x, tg, XENT_IGNORE, eps, dtype=F32, order=order)[0]) - s64) / abs(s64))
    return out
