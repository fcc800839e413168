"""What tests/test_token_stack_ref_cpu.py and tests/test_token_stack_gpu.py share for the token-stack kernels (csrc/mha_small.hip: mha_small_fwd/bwd,
mha_cross_fwd/bwd, wgrad_multi; csrc/ffn_fused.hip: ffn_fwd/bwd): float64 references written from the formulas of include/ldetr_hip.h:260-341, the
case tables, one predicate per family that restates the host-side selection and names the paths a case takes, and the error measures.  The CPU file
asserts that every path name is reached by a table case; the GPU file runs the tables.  Nothing here touches the GPU or the kernel library.

Every reference takes `dtype`: float64 is the reference, float32 is the yardstick (the same formula evaluated by torch on the CPU in the kernels'
number format), and returns every buffer the kernel writes.  A backward reference is fed the saved tensors of the float64 forward reference rounded to
float32 (`saved32`), never a kernel's outputs: a forward error cannot cancel a backward one, and the feed-forward's ReLU / dropout mask (read off the
saved h) is the same on both sides, so no share of entries may be off.

Three input kinds.  'gauss': the rounding tier (scores with a spread of ~2, ragged masks).  'dyadic': integer x, weights and biases multiples of 1/4
in [-1, 1] -- every partial sum of a projection, of the whole feed-forward and of wgrad_multi is a float32, so the result does not depend on the
order of summation and must EQUAL float64.  'uniform' (attention): dyadic, and the q rows of the projection and their bias are zero, so every score
is 0, and the number of unmasked keys of every sample is a power of two: p = 1 / n exactly, o, ypart, dk (= 0: q is 0) and dv are exact; dq and
dxpart carry the factor `scale` (no dyadic number) and lse = log n, they stay in the rounding tier.  The exact backward reference takes p from the
softmax (exactly 1 / n) where the kernel takes expf(s - lse) of the rounded lse: |float32(log n) - log n| < 2^-25 for n = 2 .. 64 (asserted by the CPU
file), so a faithful expf returns 1 / n.

The measure is per block: the largest, over (sample, head) blocks -- (row tile, hidden slice) blocks for the feed-forward -- of max|a - b| / max|b|
within the block, so that one wrong head cannot hide under another's scale.  Where a buffer is a difference of large terms (dq, dk and what is made
of them: ds = p (dp - delta), which is 0 up to rounding for a sample with one visible key; lse, which for one visible key is the score itself, a sum
of 32 signed products), the references also return the sums of |terms| (`mag`).  A block whose max|b| is at least CANCELLED = 1/32 of its largest sum
of |terms| is measured as said, unchanged; a block below that has lost five or more bits to cancellation, max|a - b| / max|b| there is a ratio of
rounding noise to rounding noise (0 / 0 for the single visible key), and its error is divided by the sum of |terms| instead -- the scale on which a
float32 evaluation can be right.  A wrong key, head or mask in such a block still shows as an error of the order of that sum.  In the tables only
blocks of samples with a single visible key fall below the threshold (asserted by the CPU file): every other block is measured as the first
sentence says."""
import functools
import math
import os

import numpy as np
import torch

import dropout_common as DC

F64, F32 = torch.float64, torch.float32
D, H, DH, FHS = 256, 8, 32, 64                          # hip/blocks.py:10; csrc/mha_small.hip:31; csrc/ffn_fused.hip:29
SCALE = float(np.float32(1.0 / math.sqrt(DH)))          # hip/blocks.py:11, as the c_float field of the argument block holds it
CANCELLED = 1.0 / 32                                    # a block that lost five or more of its 24 bits to cancellation
WORD = -0x00000FFF89ABCDEF                              # the device half of the seed on the CPU (tests/test_dropout_ref_cpu.py's); the GPU file draws one
NEG_INF = float('-inf')


def limit_threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def host_seed(k):
    """The host half of a case's dropout seed, formed like hip.core.next_seed() forms one."""
    return ((0x1234 << 32) ^ ((k + 1) * 0x9E3779B1)) & 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------------ measures and bounds
def block_err(a, b, blocks, mag=None):
    """max over blocks of max|a - b| / max|b| within the block; `blocks` maps a buffer to [blocks, elements].  A block whose max|b| is below
    CANCELLED x its largest sum of |terms| (max|mag|) is divided by max|mag| instead.  A block whose reference (and mag) is exactly 0 must be exactly 0."""
    a, b = blocks(a.detach().double().cpu()), blocks(b.detach().double().cpu())
    den = b.abs().amax(1)
    if mag is not None:
        m = blocks(mag.detach().double().cpu()).abs().amax(1)
        den = torch.where(den < CANCELLED * m, m, den)
    err = (a - b).abs().amax(1)
    r = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))))
    r = torch.where(err.isnan(), torch.full_like(err, float('nan')), r)
    return float('nan') if bool(r.isnan().any()) else r.max().item()


def blk_rows(B, L, parts=1):
    """[B*L, parts*256] -> one block per (sample, part, head)."""
    return lambda t: t.reshape(B, L, parts * H, DH).permute(0, 2, 1, 3).reshape(B * parts * H, L * DH)


def blk_lse(B, L):
    return lambda t: t.reshape(B * H, L)


def blk_parts(B, L):
    """[8, B*L, 256] -> one block per (head, sample)."""
    return lambda t: t.reshape(H * B, L * D)


def _pad_rows(t, axis, mult):
    n = t.shape[axis]
    pad = (-n) % mult
    if pad:
        shape = list(t.shape)
        shape[axis] = pad
        t = torch.cat([t, torch.zeros(shape, dtype=t.dtype)], axis)
    return t


def blk_tiles(M, F):
    """[M, F] -> one block per (32-row tile, 64-wide hidden slice)."""
    def f(t):
        t = _pad_rows(t, 0, 32)
        nt = t.shape[0] // 32
        return t.reshape(nt, 32, F // FHS, FHS).permute(0, 2, 1, 3).reshape(nt * (F // FHS), 32 * FHS)
    return f


def blk_slices(M, F):
    """[F/64, M, 256] -> one block per (hidden slice, 32-row tile)."""
    def f(t):
        t = _pad_rows(t, 1, 32)
        return t.reshape(F // FHS * (t.shape[1] // 32), 32 * D)
    return f


def blk_whole(t):
    return t.reshape(1, -1)


# Bounds the project already holds for these quantities (tests/dropout_common.py): attention buffers at TOL_STACK (forward buffers 'y', gradients
# 'grad'; weight gradients are held to 'grad' by the same test), feed-forward buffers at TOL_FFN['y'].
FWD_KEYS = ['self_qkv', 'self_o', 'self_lse', 'self_ypart', 'cross_q', 'cross_o', 'cross_lse', 'cross_ypart']
BWD_KEYS = ['self_dqkv', 'self_dxpart', 'cross_dq', 'cross_dk', 'cross_dv', 'cross_dxpart', 'wgrad_dw', 'wgrad_db']
FFN_KEYS = ['ffn_h', 'ffn_ypart', 'ffn_dh', 'ffn_dxpart']
PROJECT_BOUND = dict([(k, DC.TOL_STACK['y']) for k in FWD_KEYS] + [(k, DC.TOL_STACK['grad']) for k in BWD_KEYS] + [(k, DC.TOL_FFN['y']) for k in FFN_KEYS])

# float32 torch on the CPU against the float64 reference in block_err's measure, worst case over the tables below (test_token_stack_ref_cpu.py
# re-measures them and asserts each is within a factor 4 of what it finds); the GPU file allows FP32_FACTOR x these (other summation order, fma
# contraction, expf / logf) and at most PROJECT_BOUND:
#   key          baseline  bound   | key           baseline  bound   | key          baseline  bound
#   self_qkv     8.74e-7   3.5e-6  | cross_q       7.85e-7   3.1e-6  | ffn_h        6.74e-7   2.7e-6
#   self_o       1.38e-6   5.5e-6  | cross_o       1.45e-6   5.8e-6  | ffn_ypart    5.37e-7   2.1e-6
#   self_lse     1.13e-6   4.5e-6  | cross_lse     1.27e-6   5.1e-6  | ffn_dh       7.46e-7   3.0e-6
#   self_ypart   1.54e-6   6.2e-6  | cross_ypart   1.32e-6   5.3e-6  | ffn_dxpart   5.13e-7   2.1e-6
#   self_dqkv    1.81e-6   7.2e-6  | cross_dq      1.55e-6   6.2e-6  | wgrad_dw     3.58e-7   1.4e-6
#   self_dxpart  1.71e-6   6.8e-6  | cross_dk      1.96e-6   7.8e-6  | wgrad_db     2.92e-7   1.2e-6
#                                  | cross_dv      2.46e-6   9.8e-6  |
#                                  | cross_dxpart  1.42e-6   5.7e-6  |
FP32_BASELINE = dict(self_qkv=8.74e-7, self_o=1.38e-6, self_lse=1.13e-6, self_ypart=1.54e-6, self_dqkv=1.81e-6, self_dxpart=1.71e-6,
                     cross_q=7.85e-7, cross_o=1.45e-6, cross_lse=1.27e-6, cross_ypart=1.32e-6, cross_dq=1.55e-6, cross_dk=1.96e-6, cross_dv=2.46e-6,
                     cross_dxpart=1.42e-6, ffn_h=6.74e-7, ffn_ypart=5.37e-7, ffn_dh=7.46e-7, ffn_dxpart=5.13e-7, wgrad_dw=3.58e-7, wgrad_db=2.92e-7)
FP32_FACTOR = 4.0


def bound(key):
    return min(FP32_FACTOR * FP32_BASELINE[key], PROJECT_BOUND[key])


# ------------------------------------------------------------------------------------------------------------------------ shared pieces
def _heads(t, B, L):
    """[B*L, 256] -> [B, 8, L, 32]: head h in columns 32 h .. 32 h + 31."""
    return t.reshape(B, L, H, DH).permute(0, 2, 1, 3)


def _rows(t):
    B, _, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, D)


def _scores(q, k, kpm, B, Lq, Lk, scale):
    s = scale * (_heads(q, B, Lq) @ _heads(k, B, Lk).transpose(-1, -2))
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], NEG_INF)
    return s


def head_out(o, w_out):
    """ypart[h] = o_h W_out[:, 32h:32h+32]^T -> [8, M, 256], no bias."""
    return torch.einsum('mhc,nhc->hmn', o.reshape(-1, H, DH), w_out.reshape(D, H, DH))


def head_in(g, w, parts):
    """dxpart[h] = g_h W_h: g [M, parts*256] (head h of part p in columns 256 p + 32 h ..), w [parts*256, 256] -> [8, M, 256]."""
    return torch.einsum('mphc,phcn->hmn', g.reshape(-1, parts, H, DH), w.reshape(parts, H, DH, D))


def attn_fwd_core(q, k, v, kpm, drop, B, Lq, Lk, scale):
    """-> o [B*Lq, 256] (before out_proj), lse [B, 8, Lq], and the largest sum of |terms| of a row's visible scores (lse is as accurate as they
    are); drop [B, 8, Lq, Lk] (0 or 1 / keep) or None.  A sample with every key masked: o NaN."""
    s = _scores(q, k, kpm, B, Lq, Lk, scale)
    lse = torch.logsumexp(s, -1)
    p = s.softmax(-1)
    if drop is not None:
        p = p * drop.to(p.dtype)
    sm = _scores(q.abs(), k.abs(), kpm, B, Lq, Lk, scale).clamp_min(0.0).amax(-1)
    return _rows(p @ _heads(v, B, Lk)), lse, sm


def attn_bwd_core(q, k, v, o, lse, dO, kpm, drop, B, Lq, Lk, scale, p_from_softmax=False):
    """The attention backward on saved q, k, v, o, lse -> (dq, dk, dv) and the sums of |terms| of dq and dk (see the module docstring).
    p = exp(s - lse) as the kernels recompute it (p_from_softmax: from the scores alone, for the exact tier)."""
    qh, kh, vh, oh, dOh = _heads(q, B, Lq), _heads(k, B, Lk), _heads(v, B, Lk), _heads(o, B, Lq), _heads(dO, B, Lq)
    s = _scores(q, k, kpm, B, Lq, Lk, scale)
    p = s.softmax(-1) if p_from_softmax else (s - lse[..., None]).exp()
    dp = dOh @ vh.transpose(-1, -2)
    pd = p
    if drop is not None:
        dp, pd = dp * drop.to(p.dtype), p * drop.to(p.dtype)
    delta = (oh * dOh).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dsm = p * (dp.abs() + delta.abs()) * scale
    dq, dk, dv = ds @ kh, ds.transpose(-1, -2) @ qh, pd.transpose(-1, -2) @ dOh
    return _rows(dq), _rows(dk), _rows(dv), _rows(dsm @ kh.abs()), _rows(dsm.transpose(-1, -2) @ qh.abs())


def pick(t, dtype, *names):
    return [t[n].to(dtype) for n in names]


def saved32(fwd, dtype, *names):
    """The float64 forward reference's tensors as the backward is handed them: rounded to float32 (fwd['unrounded']: as they are, for the CPU file's
    comparison with autograd)."""
    return [fwd[n].to(dtype) if fwd.get('unrounded') else fwd[n].float().to(dtype) for n in names]


def make_kpm(kind, B, Lk, seed):
    """bool [B, Lk] (True = masked key) or None.  'ragged': dropout_common.ragged_kpm;  'key0': ragged, and sample 1 % B keeps key 0 alone;
    'midtile': ragged, and sample 1 % B has keys 16..31 masked;  'full': ragged, and sample 1 has every key masked;  'pow2': sample b keeps
    max(1, P >> b) keys (P the largest power of two <= Lk), scattered."""
    if kind == 'none':
        return None
    kpm = DC.ragged_kpm(B, Lk)
    if kind == 'key0':
        kpm[1 % B, 1:] = True
        kpm[1 % B, 0] = False
    elif kind == 'midtile':
        kpm[1 % B, 16:32] = True
    elif kind == 'full':
        assert B >= 2
        kpm[1] = True
    elif kind == 'pow2':
        g = torch.Generator().manual_seed(777 + seed)
        kpm[:] = True
        P = 1 << (Lk.bit_length() - 1)
        for b in range(B):
            kpm[b, torch.randperm(Lk, generator=g)[:max(1, P >> b)]] = False
    else:
        assert kind == 'ragged', kind
    return kpm


def _gauss_or_dyadic(g, kind, shape, std=1.0, lim=4):
    if kind == 'gauss':
        return torch.randn(shape, generator=g) * std
    return torch.randint(-lim, lim + 1, shape, generator=g).float() / 4.0


def _ints(g, kind, shape, lim=2):
    return torch.randn(shape, generator=g) if kind == 'gauss' else torch.randint(-lim, lim + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------------------------------ mha_small
def self_case(name, B, L, kpm='none', pitched=False, p=0.0, kinds=('gauss', 'dyadic')):
    return dict(name=name, B=B, L=L, kpm=kpm, pitched=pitched, p=p, kinds=kinds)


# the smallest shapes that reach each path: L in {1, 9, 10, 15, 16}, B in {1, 3}, kpm NULL / ragged / one sample with key 0 alone, x packed and pitched
SELF_CASES = [
    self_case('L1-B1', 1, 1),
    self_case('L1-B3', 3, 1, 'ragged'),
    self_case('L9-B3-ragged', 3, 9, 'ragged'),
    self_case('L10-B3-key0', 3, 10, 'key0'),
    self_case('L15-B1-pitched', 1, 15, pitched=True),
    self_case('L16-B3-ragged-pitched', 3, 16, 'ragged', pitched=True),
    self_case('L16-B1', 1, 16),
    self_case('L9-B3-ragged-drop', 3, 9, 'ragged', p=0.15, kinds=('gauss',)),
    self_case('L10-B0', 0, 10, kinds=()),
    self_case('U-L16-B1', 1, 16, kinds=('uniform',)),
    self_case('U-L16-B3-pow2', 3, 16, 'pow2', kinds=('uniform',)),
    self_case('U-L9-B3-pow2-pitched', 3, 9, 'pow2', pitched=True, kinds=('uniform',)),
]
SELF_BY_NAME = {c['name']: c for c in SELF_CASES}
# n = 2 launches (first problem, second problem): different B and L, kpm on the second alone; B = 0 first (nb0 = 0) and second
SELF_GROUPS = [('L16-B1', 'L9-B3-ragged'), ('L10-B0', 'L15-B1-pitched'), ('L9-B3-ragged-drop', 'L10-B0'), ('L10-B3-key0', 'L1-B1')]
SELF_MASKED = self_case('L9-B3-full', 3, 9, 'full', kinds=('gauss',))        # one sample with every key masked: its own test
SELF_PATHS = ['pad_rows', 'full_tile', 'kpm_null', 'kpm', 'single_key_sample', 'B1', 'B3', 'x_packed', 'x_pitched', 'dropout', 'no_dropout',
              'dqkv', 'dqkv_null', 'B0_alone', 'group/second', 'group/nb0_zero', 'group/second_empty', 'group/kpm_second_only']


def self_paths(c, second=None):
    """mha_small_launch (csrc/mha_small.hip:840-854) and the two kernels.  One block per (sample, head) (:44, :358); rows / keys >= L of the 16-row tile
    are padding (:59, :84, :170, :379, :406, :537); kpm NULL or read (:84); the dropout branch (:143, :469, :499); dqkv optional (:480, :517; the GPU
    file runs every backward with and without it); B = 0 launches nothing (:849); a second problem's blocks follow the first's, nb0 = 8 B_first
    (:40-42, :354-356)."""
    names = set()
    for q in (c,) + ((second,) if second else ()):
        if q['B'] == 0:
            continue
        names |= {'pad_rows' if q['L'] < 16 else 'full_tile', 'kpm_null' if q['kpm'] == 'none' else 'kpm', f'B{q["B"]}',
                  'x_pitched' if q['pitched'] else 'x_packed', 'dropout' if q['p'] > 0 else 'no_dropout', 'dqkv', 'dqkv_null'}
        if q['kpm'] == 'key0':
            names.add('single_key_sample')
    if second is None:
        if c['B'] == 0:
            names.add('B0_alone')
        return names
    names.add('group/second')
    if c['B'] == 0:
        names.add('group/nb0_zero')
    if second['B'] == 0:
        names.add('group/second_empty')
    if c['kpm'] == 'none' and second['kpm'] != 'none' and c['B'] and second['B']:
        names.add('group/kpm_second_only')
    return names


def self_inputs(c, kind):
    """-> dict(x, w_in, b_in, w_out, dr) float32 and kpm (bool or None)."""
    g = torch.Generator().manual_seed(81000 + 7 * len(c['name']) + 131 * c['B'] + 17 * c['L'] + {'gauss': 0, 'dyadic': 1, 'uniform': 2}[kind])
    M = c['B'] * c['L']
    t = dict(x=_ints(g, kind, (M, D)), w_in=_gauss_or_dyadic(g, kind, (3 * D, D), 1.5 / 16), b_in=_gauss_or_dyadic(g, kind, (3 * D,), 0.2),
             w_out=_gauss_or_dyadic(g, kind, (D, D), 1.0 / 16), dr=_ints(g, kind, (M, D)))
    if kind == 'uniform':
        t['w_in'][:D] = 0.0
        t['b_in'][:D] = 0.0
    t['kpm'] = make_kpm(c['kpm'], c['B'], c['L'], c['L'])
    return t


def self_drop(c, masks, k):
    return masks.attention(host_seed(k), c['p'], c['B'], H, c['L'], c['L']) if c['p'] > 0 else None


def self_fwd_ref(t, c, drop=None, dtype=F64, scale=SCALE, kpm='own'):
    """qkv = x W_in^T + b_in (q unscaled); per (sample, head) S = scale q k^T, key mask, softmax, dropout, o = P V; ypart[h] (ldetr_hip.h:283-290)."""
    x, w_in, b_in, w_out = pick(t, dtype, 'x', 'w_in', 'b_in', 'w_out')
    kpm = t['kpm'] if isinstance(kpm, str) else kpm
    qkv = x @ w_in.t() + b_in
    o, lse, sm = attn_fwd_core(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], kpm, drop, c['B'], c['L'], c['L'], scale)
    return dict(qkv=qkv, o=o, lse=lse, ypart=head_out(o, w_out), mag_lse=sm)


def self_bwd_ref(t, fwd, c, drop=None, dtype=F64, scale=SCALE, exact=False):
    """dO_h = dr W_out[:, head]; attention backward on the saved qkv, o, lse; dqkv; dxpart[h] = dqkv_h W_in,h (ldetr_hip.h:291-294) -> (out, mag)."""
    w_in, w_out, dr = pick(t, dtype, 'w_in', 'w_out', 'dr')
    qkv, o, lse = saved32(fwd, dtype, 'qkv', 'o', 'lse')
    dq, dk, dv, mq, mk = attn_bwd_core(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, lse, dr @ w_out, t['kpm'], drop, c['B'], c['L'], c['L'], scale, exact)
    dqkv, mqkv = torch.cat([dq, dk, dv], 1), torch.cat([mq, mk, dv.abs()], 1)
    return dict(dqkv=dqkv, dxpart=head_in(dqkv, w_in, 3)), dict(dqkv=mqkv, dxpart=head_in(mqkv, w_in.abs(), 3))


@functools.lru_cache(maxsize=None)
def self_reference(name, kind, k):
    """float64 (fwd, bwd, mag) of a table case with the CPU's masks (k: the case's seed number); computed once, do not write to it."""
    c = SELF_BY_NAME.get(name, SELF_MASKED)
    t, drop = self_inputs(c, kind), self_drop(c, DC.Masks(WORD), k)
    fwd = self_fwd_ref(t, c, drop)
    return (fwd,) + self_bwd_ref(t, fwd, c, drop, exact=kind == 'uniform')


# ------------------------------------------------------------------------------------------------------------------------ mha_cross
def cross_case(name, B, Lq, Lk, kpm='none', pitched=False, p=0.0, kinds=('gauss', 'dyadic')):
    return dict(name=name, B=B, Lq=Lq, Lk=Lk, kpm=kpm, pitched=pitched, p=p, kinds=kinds)


# Lq in {1, 9, 16}; Lk in {1, 15, 16, 17, 33, 48, 64}: 1..4 key tiles, a ragged last tile, idle dK / dV waves; k / v / dk / dv packed and as views into one
# wider buffer; kpm NULL, ragged, and with the second of three key tiles fully masked
CROSS_CASES = [
    cross_case('Lq1-Lk1-B1', 1, 1, 1),
    cross_case('Lq9-Lk15-B3-ragged', 3, 9, 15, 'ragged'),
    cross_case('Lq16-Lk16-B1', 1, 16, 16),
    cross_case('Lq9-Lk17-B3-ragged-pitched', 3, 9, 17, 'ragged', pitched=True),
    cross_case('Lq16-Lk33-B1-pitched', 1, 16, 33, pitched=True),
    cross_case('Lq9-Lk48-B3-midtile', 3, 9, 48, 'midtile'),
    cross_case('Lq16-Lk64-B3-ragged-pitched', 3, 16, 64, 'ragged', pitched=True),
    cross_case('Lq1-Lk64-B1', 1, 1, 64),
    cross_case('Lq9-Lk33-B3-ragged-drop', 3, 9, 33, 'ragged', p=0.25, kinds=('gauss',)),
    cross_case('Lq9-Lk16-B3-key0', 3, 9, 16, 'key0'),
    cross_case('U-Lq16-Lk64-B1', 1, 16, 64, kinds=('uniform',)),
    cross_case('U-Lq9-Lk33-B3-pow2-pitched', 3, 9, 33, 'pow2', pitched=True, kinds=('uniform',)),
    cross_case('U-Lq1-Lk17-B3-pow2', 3, 1, 17, 'pow2', kinds=('uniform',)),
]
CROSS_BY_NAME = {c['name']: c for c in CROSS_CASES}
CROSS_MASKED = cross_case('Lq9-Lk33-B3-full', 3, 9, 33, 'full', kinds=('gauss',))
CROSS_PATHS = ['key_tiles1', 'key_tiles2', 'key_tiles3', 'key_tiles4', 'ragged_last_key_tile', 'full_last_key_tile', 'idle_dkdv_waves', 'kv_packed',
               'kv_pitched', 'kpm_null', 'kpm', 'masked_key_tile', 'single_key_sample', 'pad_queries', 'full_queries', 'dropout', 'no_dropout', 'B1', 'B3']


def cross_paths(c):
    """mha_cross_launch (csrc/mha_small.hip:877-887) and the two kernels.  One block per (sample, head); K_h / V_h rows >= Lk are zero-filled and
    masked (:219-223, :232, :582-586, :597); the backward's dQ wave loops over nkt = ceil(Lk / 16) key tiles (:555, :649), wave kt < nkt makes dK / dV of
    tile kt and the others idle (:679); rows of a ragged last tile are not stored (:712); dk / dv are written at pitches lddk / lddv (:713-714)."""
    nkt = (c['Lk'] + 15) // 16
    names = {f'key_tiles{nkt}', 'ragged_last_key_tile' if c['Lk'] % 16 else 'full_last_key_tile', 'kv_pitched' if c['pitched'] else 'kv_packed',
             'kpm_null' if c['kpm'] == 'none' else 'kpm', 'pad_queries' if c['Lq'] < 16 else 'full_queries', 'dropout' if c['p'] > 0 else 'no_dropout', f'B{c["B"]}'}
    if nkt < 4:
        names.add('idle_dkdv_waves')
    if c['kpm'] == 'midtile':
        names.add('masked_key_tile')
    if c['kpm'] == 'key0':
        names.add('single_key_sample')
    return names


def cross_inputs(c, kind):
    """-> dict(x, w_q, b_q, k, v, w_out, dr) float32 and kpm."""
    g = torch.Generator().manual_seed(82000 + 7 * len(c['name']) + 131 * c['B'] + 17 * c['Lq'] + 3 * c['Lk'] + {'gauss': 0, 'dyadic': 1, 'uniform': 2}[kind])
    Mq, Mk = c['B'] * c['Lq'], c['B'] * c['Lk']
    t = dict(x=_ints(g, kind, (Mq, D)), w_q=_gauss_or_dyadic(g, kind, (D, D), 1.5 / 16), b_q=_gauss_or_dyadic(g, kind, (D,), 0.2),
             k=_ints(g, kind, (Mk, D)) * (1.5 if kind == 'gauss' else 1.0), v=_ints(g, kind, (Mk, D), lim=8), w_out=_gauss_or_dyadic(g, kind, (D, D), 1.0 / 16),
             dr=_ints(g, kind, (Mq, D)))
    if kind == 'uniform':
        t['w_q'][:] = 0.0
        t['b_q'][:] = 0.0
    t['kpm'] = make_kpm(c['kpm'], c['B'], c['Lk'], c['Lk'])
    return t


def cross_drop(c, masks, k):
    return masks.attention(host_seed(k), c['p'], c['B'], H, c['Lq'], c['Lk']) if c['p'] > 0 else None


def cross_fwd_ref(t, c, drop=None, dtype=F64, scale=SCALE, kpm='own'):
    """q = x W_q^T + b_q; attention onto the given k, v; ypart[h] (ldetr_hip.h:309-314)."""
    x, w_q, b_q, k, v, w_out = pick(t, dtype, 'x', 'w_q', 'b_q', 'k', 'v', 'w_out')
    kpm = t['kpm'] if isinstance(kpm, str) else kpm
    q = x @ w_q.t() + b_q
    o, lse, sm = attn_fwd_core(q, k, v, kpm, drop, c['B'], c['Lq'], c['Lk'], scale)
    return dict(q=q, o=o, lse=lse, ypart=head_out(o, w_out), mag_lse=sm)


def cross_bwd_ref(t, fwd, c, drop=None, dtype=F64, scale=SCALE, exact=False):
    """dO_h = dr W_out[:, head]; attention backward on the saved q and the given k, v -> dq, dk, dv; dxpart[h] = dq_h W_q,h (ldetr_hip.h:315-317)."""
    w_q, k, v, w_out, dr = pick(t, dtype, 'w_q', 'k', 'v', 'w_out', 'dr')
    q, o, lse = saved32(fwd, dtype, 'q', 'o', 'lse')
    dq, dk, dv, mq, mk = attn_bwd_core(q, k, v, o, lse, dr @ w_out, t['kpm'], drop, c['B'], c['Lq'], c['Lk'], scale, exact)
    return dict(dq=dq, dk=dk, dv=dv, dxpart=head_in(dq, w_q, 1)), dict(dq=mq, dk=mk, dv=dv.abs(), dxpart=head_in(mq, w_q.abs(), 1))


@functools.lru_cache(maxsize=None)
def cross_reference(name, kind, k):
    c = CROSS_BY_NAME.get(name, CROSS_MASKED)
    t, drop = cross_inputs(c, kind), cross_drop(c, DC.Masks(WORD), k)
    fwd = cross_fwd_ref(t, c, drop)
    return (fwd,) + cross_bwd_ref(t, fwd, c, drop, exact=kind == 'uniform')


# ------------------------------------------------------------------------------------------------------------------------ feed-forward
def ffn_case(name, M, F, pitched=False, p=0.0, kinds=('gauss', 'dyadic')):
    return dict(name=name, M=M, F=F, pitched=pitched, p=p, kinds=kinds)


# M in {1, 31, 32, 33, 70}: a ragged and a full last row tile, one to three tiles; F in {64, 128, 320}: one, two and five slices; x packed and pitched
FFN_CASES = [
    ffn_case('M1-F64', 1, 64),
    ffn_case('M31-F128-pitched', 31, 128, pitched=True),
    ffn_case('M32-F320', 32, 320),
    ffn_case('M33-F64', 33, 64),
    ffn_case('M70-F320-pitched', 70, 320, pitched=True),
    ffn_case('M70-F128-drop', 70, 128, p=0.35, kinds=('gauss',)),
]
FFN_BY_NAME = {c['name']: c for c in FFN_CASES}
FFN_GROUPS = [('M31-F128-pitched', 'M70-F320-pitched'), ('M70-F128-drop', 'M1-F64'), ('M32-F320', 'M33-F64')]
FFN_PATHS = ['row_tiles1', 'row_tiles2', 'row_tiles3', 'ragged_last_row_tile', 'full_last_row_tile', 'slices1', 'slices2', 'slices5', 'x_packed', 'x_pitched',
             'dropout', 'no_dropout', 'dh', 'dh_null', 'group/second', 'group/different_M_and_F']


def ffn_paths(c, second=None):
    """ffn_launch (csrc/ffn_fused.hip:230-244) and the two kernels.  Block = (row tile bid % gx, hidden slice bid / gx), gx = ceil(M / 32) (:54-56,
    :133-135); rows >= M of the last tile are not loaded (:63, :143) and not stored (:97, :123, :180, :206); x is read at pitch ldx (:63); the dropout
    branch (:95) and 1 / keep (:138, :178); dh optional (:180; the GPU file runs every backward with and without it); a second problem's blocks follow
    the first's (:52-54, :131-133)."""
    names = set()
    for q in (c,) + ((second,) if second else ()):
        names |= {f'row_tiles{(q["M"] + 31) // 32}', 'ragged_last_row_tile' if q['M'] % 32 else 'full_last_row_tile', f'slices{q["F"] // FHS}',
                  'x_pitched' if q['pitched'] else 'x_packed', 'dropout' if q['p'] > 0 else 'no_dropout', 'dh', 'dh_null'}
    if second is not None:
        names.add('group/second')
        if c['M'] != second['M'] and c['F'] != second['F']:
            names.add('group/different_M_and_F')
    return names


def ffn_inputs(c, kind):
    g = torch.Generator().manual_seed(83000 + 7 * len(c['name']) + 3 * c['M'] + c['F'] + {'gauss': 0, 'dyadic': 1}[kind])
    M, F = c['M'], c['F']
    return dict(x=_ints(g, kind, (M, D)), w1=_gauss_or_dyadic(g, kind, (F, D), 1.0 / 16), b1=_gauss_or_dyadic(g, kind, (F,), 0.2),
                w2=_gauss_or_dyadic(g, kind, (D, F), 1.0 / 16), dy=_ints(g, kind, (M, D)))


def ffn_drop(c, masks, k):
    return masks.rows(host_seed(k), c['p'], c['M'], c['F']) if c['p'] > 0 else None


def ffn_fwd_ref(t, c, drop=None, dtype=F64, slice_shift=0):
    """h = dropout(relu(x W1^T + b1)); ypart[s] = h[:, 64s:64s+64] W2[:, 64s:64s+64]^T (ldetr_hip.h:262-263).  slice_shift: a WRONG reference whose
    slice 0 reads its hidden columns that far to the right (the CPU file's sensitivity proof)."""
    x, w1, b1, w2 = pick(t, dtype, 'x', 'w1', 'b1', 'w2')
    M, F = c['M'], c['F']
    h = torch.relu(x @ w1.t() + b1)
    if drop is not None:
        h = h * drop.to(dtype)
    hs = h.reshape(M, F // FHS, FHS)
    if slice_shift:
        hs = hs.clone()
        hs[:, 0] = h.roll(-slice_shift, 1)[:, :FHS]
    return dict(h=h, ypart=torch.einsum('msj,nsj->smn', hs, w2.reshape(D, F // FHS, FHS)))


def ffn_bwd_ref(t, fwd, c, dtype=F64, keep_scale=None):
    """dh = (dy W2)[h > 0] / keep on the saved h; dxpart[s] = dh[:, slice] W1[slice, :] (ldetr_hip.h:264-267).  keep_scale: override of 1 / keep."""
    w1, w2, dy = pick(t, dtype, 'w1', 'w2', 'dy')
    (h,) = saved32(fwd, dtype, 'h')
    M, F = c['M'], c['F']
    ks = (DC.DR.keep_scale(c['p']) if c['p'] > 0 else 1.0) if keep_scale is None else keep_scale
    dh = (dy @ w2) * (h > 0).to(dtype) * ks
    return dict(dh=dh, dxpart=torch.einsum('msj,sjn->smn', dh.reshape(M, F // FHS, FHS), w1.reshape(F // FHS, FHS, D)))


@functools.lru_cache(maxsize=None)
def ffn_reference(name, kind, k):
    c = FFN_BY_NAME[name]
    t = ffn_inputs(c, kind)
    fwd = ffn_fwd_ref(t, c, ffn_drop(c, DC.Masks(WORD), k))
    return fwd, ffn_bwd_ref(t, fwd, c)


# ------------------------------------------------------------------------------------------------------------------------ wgrad_multi
def wdesc(M, rows, cols, lda=None, a_col0=0, ldb=None, ldw=None, dw_off=0, db=True):
    """One descriptor: A is columns a_col0 .. a_col0 + rows of a [M, lda] buffer, B the first cols columns of [M, ldb], dW [rows, ldw] starting dw_off
    floats into its (16-byte aligned) buffer."""
    lda, ldb, ldw = lda or rows, ldb or cols, ldw or cols
    assert lda >= a_col0 + rows and ldb >= cols and ldw >= cols
    return dict(M=M, rows=rows, cols=cols, lda=lda, a_col0=a_col0, ldb=ldb, ldw=ldw, dw_off=dw_off, db=db)


# n in {1, 3, 8}; M in {0, 1, 15, 16, 17, 70}; rows / cols that are no multiple of 32, or of 4; ldw % 4 != 0 and a dW 4 bytes past a 16-byte boundary
# (scalar stores) against the vector path; db NULL and present; A as a column slice of a wider buffer (dqkv's q rows for ca_w_in)
WGRAD_GROUPS = {
    'n1': [wdesc(70, 96, 64)],
    'n3': [wdesc(17, 33, 30), wdesc(0, 32, 32), wdesc(16, 256, 64, lda=768, a_col0=0, db=False)],
    'n8': [wdesc(1, 5, 7, ldw=8), wdesc(15, 32, 32, dw_off=1), wdesc(16, 40, 36), wdesc(17, 31, 33), wdesc(70, 64, 96, ldb=100, ldw=100), wdesc(0, 8, 8),
           wdesc(70, 96, 30, lda=288, a_col0=64, ldw=32, db=False), wdesc(33, 1, 1)],
    'n2-M0-first': [wdesc(0, 64, 64), wdesc(16, 33, 65, ldw=68)],
}
WGRAD_PATHS = ['n1', 'n2', 'n3', 'n8', 'M0', 'M0_first', 'store/vector', 'store/scalar_ldw', 'store/scalar_misaligned', 'store/vector_tile_tail', 'rows_tail',
               'cols_tail', 'tiles>1', 'one_tile', 'db', 'db_null', 'A_column_slice', 'ldw_gt_cols', 'idle_waves', 'all_waves', 'ragged_last_unit', 'start_after_M0']


def wgrad_paths(group):
    """ldetr_wgrad_multi_f32 (csrc/mha_small.hip:892-909) and wgrad_multi_kernel.  A descriptor with M > 0 gets ceil(rows / 32) ceil(cols / 32) blocks
    from start[i] on, one with M = 0 none (:900-901); a block finds its descriptor by counting start[i] <= blockIdx (:751); the tokens are dealt to the
    four waves in units of 16 (:759); db is added by the blocks of column tile 0 (:769, :798); dW is added with float4 where ldw % 4 == 0, dW is
    16-byte aligned and the four columns exist, else element by element (:799-815)."""
    names = {f'n{len(group)}'}
    for i, d in enumerate(group):
        if d['M'] == 0:
            names |= {'M0'} | ({'M0_first'} if i == 0 else set()) | ({'start_after_M0'} if i + 1 < len(group) else set())
            continue
        vec = d['ldw'] % 4 == 0 and d['dw_off'] % 4 == 0
        names.add('store/vector' if vec else ('store/scalar_ldw' if d['ldw'] % 4 else 'store/scalar_misaligned'))
        if vec and d['cols'] % 4:
            names.add('store/vector_tile_tail')                     # :807, n0 + c4 + 3 >= cols
        units = (d['M'] + 15) // 16
        names |= {'tiles>1' if (d['rows'] > 32 or d['cols'] > 32) else 'one_tile', 'db' if d['db'] else 'db_null', 'idle_waves' if units < 4 else 'all_waves'}
        names |= ({'rows_tail'} if d['rows'] % 32 else set()) | ({'cols_tail'} if d['cols'] % 32 else set()) | ({'ragged_last_unit'} if d['M'] % 16 else set())
        names |= ({'A_column_slice'} if d['lda'] > d['rows'] else set()) | ({'ldw_gt_cols'} if d['ldw'] > d['cols'] else set())
    return names


def wgrad_inputs(d, kind, seed):
    """-> A [M, lda], B [M, ldb], dW0 [rows, ldw], db0 [rows]: the whole buffers, gaps included (the kernel must not read them into a result)."""
    g = torch.Generator().manual_seed(84000 + seed)
    return dict(A=_ints(g, kind, (d['M'], d['lda']), lim=3), B=_ints(g, kind, (d['M'], d['ldb']), lim=3), dW0=_ints(g, kind, (d['rows'], d['ldw']), lim=9),
                db0=_ints(g, kind, (d['rows'],), lim=9))


def wgrad_ref(t, d, dtype=F64):
    """dW[:, :cols] += A^T B, db += column sums of A (ldetr_hip.h:333-335); dW columns >= cols keep their content."""
    A, Bm, dW, db = [t[n].to(dtype).clone() for n in ('A', 'B', 'dW0', 'db0')]
    A = A[:, d['a_col0']:d['a_col0'] + d['rows']]
    dW[:, :d['cols']] += A.t() @ Bm[:, :d['cols']]
    return dict(dw=dW, db=db + A.sum(0))


# ------------------------------------------------------------------------------------------------------------------------ float32 yardstick
def case_numbers():
    """(family, case, seed number k) of every table case and the extra masked ones: k selects the host seed."""
    out, k = [], 0
    for fam, cases in (('self', SELF_CASES + [SELF_MASKED]), ('cross', CROSS_CASES + [CROSS_MASKED]), ('ffn', FFN_CASES)):
        for c in cases:
            out.append((fam, c, k))
            k += 1
    return out


SEED_NUMBER = {(fam, c['name']): k for fam, c, k in case_numbers()}


def self_figures(c, got_f, got_b, fwd, bwd, mag):
    """[(key, error)] of a self-attention case's buffers against the float64 reference."""
    B, L = c['B'], c['L']
    return [('self_qkv', block_err(got_f['qkv'], fwd['qkv'], blk_rows(B, L, 3))), ('self_o', block_err(got_f['o'], fwd['o'], blk_rows(B, L))),
            ('self_lse', block_err(got_f['lse'], fwd['lse'], blk_lse(B, L), fwd['mag_lse'])), ('self_ypart', block_err(got_f['ypart'], fwd['ypart'], blk_parts(B, L))),
            ('self_dqkv', block_err(got_b['dqkv'], bwd['dqkv'], blk_rows(B, L, 3), mag['dqkv'])),
            ('self_dxpart', block_err(got_b['dxpart'], bwd['dxpart'], blk_parts(B, L), mag['dxpart']))]


def cross_figures(c, got_f, got_b, fwd, bwd, mag):
    B, Lq, Lk = c['B'], c['Lq'], c['Lk']
    return [('cross_q', block_err(got_f['q'], fwd['q'], blk_rows(B, Lq))), ('cross_o', block_err(got_f['o'], fwd['o'], blk_rows(B, Lq))),
            ('cross_lse', block_err(got_f['lse'], fwd['lse'], blk_lse(B, Lq), fwd['mag_lse'])), ('cross_ypart', block_err(got_f['ypart'], fwd['ypart'], blk_parts(B, Lq))),
            ('cross_dq', block_err(got_b['dq'], bwd['dq'], blk_rows(B, Lq), mag['dq'])), ('cross_dk', block_err(got_b['dk'], bwd['dk'], blk_rows(B, Lk), mag['dk'])),
            ('cross_dv', block_err(got_b['dv'], bwd['dv'], blk_rows(B, Lk))),
            ('cross_dxpart', block_err(got_b['dxpart'], bwd['dxpart'], blk_parts(B, Lq), mag['dxpart']))]


def ffn_figures(c, got_f, got_b, fwd, bwd):
    M, F = c['M'], c['F']
    return [('ffn_h', block_err(got_f['h'], fwd['h'], blk_tiles(M, F))), ('ffn_ypart', block_err(got_f['ypart'], fwd['ypart'], blk_slices(M, F))),
            ('ffn_dh', block_err(got_b['dh'], bwd['dh'], blk_tiles(M, F))), ('ffn_dxpart', block_err(got_b['dxpart'], bwd['dxpart'], blk_slices(M, F)))]


def wgrad_figures(d, got, ref):
    return [('wgrad_dw', block_err(got['dw'][:, :d['cols']], ref['dw'][:, :d['cols']], blk_whole)), ('wgrad_db', block_err(got['db'], ref['db'], blk_whole))]


ROUNDING_KINDS = ('gauss', 'uniform')       # 'uniform' cases: lse, dq and dxpart are rounding-tier buffers, the others are (also) held to equality


def measure_fp32_baselines():
    """The float32 CPU evaluation of every reference against its float64 evaluation, worst case over the tables -> dict like FP32_BASELINE."""
    out = dict.fromkeys(FP32_BASELINE, 0.0)
    masks = DC.Masks(WORD)

    def worst(figs):
        for key, e in figs:
            out[key] = max(out[key], e)
    for fam, c, k in case_numbers():
        for kind in c['kinds']:
            if kind not in ROUNDING_KINDS or c.get('kpm') == 'full':          # (a fully masked sample: NaN on both sides)
                continue
            if fam == 'self':
                fwd, bwd, mag = self_reference(c['name'], kind, k)
                t, drop = self_inputs(c, kind), self_drop(c, masks, k)
                worst(self_figures(c, self_fwd_ref(t, c, drop, F32), self_bwd_ref(t, fwd, c, drop, F32)[0], fwd, bwd, mag))
            elif fam == 'cross':
                fwd, bwd, mag = cross_reference(c['name'], kind, k)
                t, drop = cross_inputs(c, kind), cross_drop(c, masks, k)
                worst(cross_figures(c, cross_fwd_ref(t, c, drop, F32), cross_bwd_ref(t, fwd, c, drop, F32)[0], fwd, bwd, mag))
            elif fam == 'ffn':
                fwd, bwd = ffn_reference(c['name'], kind, k)
                t = ffn_inputs(c, kind)
                worst(ffn_figures(c, ffn_fwd_ref(t, c, ffn_drop(c, masks, k), F32), ffn_bwd_ref(t, fwd, c, F32), fwd, bwd))
    for gi, (name, group) in enumerate(WGRAD_GROUPS.items()):
        for i, d in enumerate(group):
            if d['M']:
                t = wgrad_inputs(d, 'gauss', 16 * gi + i)
                worst(wgrad_figures(d, wgrad_ref(t, d, F32), wgrad_ref(t, d)))
    return out
