"""What tests/test_p3_engine_ref_cpu.py and tests/test_p3_engine_gpu.py share for the plane-format conv engine (csrc/p3_engine.hip behind
hip/p3.py): a Python port of the host-side launch policy, one list of path names, the case tables, the input classes, float64 references
written from the header's formulas, the measures and the float32 yardsticks.  Nothing here touches the GPU or the kernel library.

The policy model restates the host functions line by line (`# :N` = line N of csrc/p3_engine.hip).  For one entry point and one geometry it
returns the ten fields of ldetr_p3_last_launch and the path names the launch reaches; the GPU file asserts the ten fields for every case, which
is what makes the path list true, and the CPU file asserts that every name of P3_PATHS is reached by a table case.

Input classes (a case runs in each class that applies):
  select    the weights (forward, data gradient) hold ONE non-zero (tap, channel) = +-2^e per output channel, the weight gradient's dY one
            non-zero pixel per channel; the other operand is arbitrary fp32 (full 24-bit mantissas, wide exponents, values next to FLT_MAX).
            Every output is +-(one input element) x 2^e, or the epilogue of zero: the three planes of the element times a power of two are
            three exact products whose fp32 sum is the element again, so the kernel must equal float64 bit for bit, split-K and atomics
            included.  No tolerance for a wrong tap address, parity class, padding decision or plane.
  select_w  the mirror image for the gather and patch kernels: the ACTIVATIONS are non-zero (+-2^e, one channel) on a pixel lattice of period
            KH x KW, so that every window holds at most one of them, and the weights are arbitrary fp32: every output is one weight element
            times a power of two.  This is the class that sees the weights' mid and lo planes (the hi.lo product) without a tolerance.
  grid      both operands dense on the integers with at most 16 significant bits (values 256 + b, b odd, fill the hi and the mid plane; small
            integers fill hi only), sized so that every output's sum of |terms| stays below 2^24: every kept product and every partial sum is
            an fp32 number, the result does not depend on the order of summation and must equal float64 exactly.
  rounding  randn operands with a mild log-normal factor and mixed signs, held to FP32_FACTOR x the float32 yardstick in two measures.

An additive epilogue term (bias, one residual, the accumulated-onto dW) rounds once in fp32 and once in float64-then-fp32 alike as long as the
float64 sum is exact, which the narrow exponent range of those select cases ensures; two additive terms round twice in the kernel, so such
epilogues run in `grid` (integers: exact) and `rounding` only."""
import functools
import itertools
import math
import os
import zlib

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
FLT_MAX = float(torch.finfo(F32).max)


def limit_threads():
    """CPU references: more threads than this are slower on many-core hosts."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))


# ================================================================================================================ the launch policy, restated
WS_COUNTERS = 262144                     # csrc/gemm_conv.hip:1373
WS_BYTES_DEFAULT = 256 << 20             # hip/core.py:126 (LDETR_WORKSPACE_MIB)
C3_NGMAX = 13                            # :574
SMALL_FLOPS = 1.5e9                      # :1220


def cdiv(a, b):
    return (a + b - 1) // b


def ws_alloc(ws_bytes, tiles, nbytes):
    """ring_alloc (csrc/gemm_conv.hip:1386-1397): false when no workspace is registered or the request exceeds a whole ring."""
    need = (nbytes + 255) & ~255
    pbytes = ws_bytes - WS_COUNTERS * 4 if ws_bytes > WS_COUNTERS * 4 else 0
    return bool(ws_bytes) and need <= pbytes and tiles <= WS_COUNTERS


def choose_xcd_array(mtiles, ntiles, a_bytes, b_bytes):
    """:1162-1171 -> xm, xn, grid_x"""
    best, xm, xn = -1.0, 8, 1
    for n in (1, 2, 4, 8):
        m = 8 // n
        if (n > ntiles and n > 1) or (m > mtiles and m > 1):
            continue
        cost = a_bytes * n + b_bytes * m
        if best < 0 or cost < best:
            best, xm, xn = cost, m, n
    return xm, xn, 8 * cdiv(mtiles, xm) * cdiv(ntiles, xn)


def slot_target(flops, dflt):
    """:1219-1222"""
    return 256 if (flops < SMALL_FLOPS and dflt > 256) else dflt


def nt_splitk(M, N, nkt, bm, bn, slots):
    """:1227-1232"""
    nt = cdiv(M, bm) * cdiv(N, bn)
    sk = 1
    if nt < slots * 3 // 4:
        sk = max(1, min(slots // nt, nkt // 4, 16))
    return sk


def c3_geometry(N, H, W):
    """:1282-1296 -> (dict, None) or (None, reason)"""
    def lg(v):
        l = 0
        while (1 << l) < v:
            l += 1
        return l if (1 << l) == v else -1
    PW = W if W < 16 else 16
    if lg(PW) < 0 or W % PW:
        return None, 'W_not_multiple_of_PW'
    PH0 = min(128 // PW, H)
    PH = PH0
    while PH > 1 and (H % PH or lg(PH) < 0):
        PH >>= 1
    if lg(PH) < 0 or H % PH or 128 % (PW * PH):
        return None, 'H_not_divisible'                 # (not reachable: the loop ends on a power of two that divides H, 1 at the latest)
    NP = 128 // (PW * PH)
    NH = NP * (PH + 2) * (PW + 2)
    NG = (NH + 15) // 16
    if NG > C3_NGMAX:
        # the only way H decides: a first patch height that does not divide H is halved, and the tile then holds more, smaller patches
        return None, 'H_not_divisible' if (H % PH0 or lg(PH0) < 0) else 'NG_gt_13'
    ppr, ppi = W // PW, (H // PH) * (W // PW)
    return dict(PW=PW, PH=PH, NP=NP, NG=NG, ppr=ppr, ppi=ppi, mtiles=(N * ppi + NP - 1) // NP), None


def c3_accepted_geometries(limit=64):
    """Every (PW, PH, NP) c3_geometry accepts for H, W in 1..limit."""
    out = set()
    for H, W in itertools.product(range(1, limit + 1), repeat=2):
        g, _ = c3_geometry(1, H, W)
        if g:
            out.add((g['PW'], g['PH'], g['NP']))
    return sorted(out)


def c3_geometry_brute(H, W):
    """The patch conditions stated outright: the largest patch of PW x PH pixels (PW = min(W, 16) first, then the tallest PH) with PW | W, PH a
    power of two dividing H, PW * PH | 128 and the halo of the tile's NP patches within 13 groups of 16 pixels."""
    PW = min(W, 16)
    if W % PW or PW & (PW - 1):
        return None
    for PH in (128, 64, 32, 16, 8, 4, 2, 1):
        if PH * PW <= 128 and PH <= H and H % PH == 0 and 128 % (PW * PH) == 0:
            NP = 128 // (PW * PH)
            return (PW, PH, NP) if -(-NP * (PH + 2) * (PW + 2) // 16) <= 13 else None
    return None


def plan_nt(M, N, Kc, KH, KW, nkt, nclass, ngroups, bm, bn, sk, ws_bytes):
    """:1200-1214 -> dict(mtiles, ntiles, xm, xn, gx, sk, ncls, denied)"""
    mt, ntl = cdiv(M, bm), cdiv(N, bn)
    ncls = nclass if nclass > 1 else (ngroups if ngroups > 1 else 1)
    nt = mt * ntl
    xm, xn, gx = choose_xcd_array(mt, ntl, M * Kc * 6.0, N * KH * KW * Kc * 6.0)
    sk = max(1, min(sk, nkt))
    denied = False
    if sk > 1 and not ws_alloc(ws_bytes, nt * ncls, nt * ncls * sk * bm * bn * 4):
        sk, denied = 1, True
    return dict(mtiles=mt, ntiles=ntl, xm=xm, xn=xn, gx=gx, sk=sk, ncls=ncls, denied=denied)


def plan_c3(g, N, H, W, Kc, Nout, ngroups, ws_bytes):
    """:1299-1312"""
    ntl = cdiv(Nout, 64)
    nt = g['mtiles'] * ntl
    ncc = Kc // 32
    sk = 1
    slots = slot_target(2.0 * N * H * W * Nout * 9.0 * Kc, 512)
    if nt < slots * 3 // 4:
        sk = max(1, min(slots // nt, ncc // 2, 16))
    sk = min(sk, ncc)
    ng = ngroups if ngroups > 1 else 1
    denied = False
    if sk > 1 and not ws_alloc(ws_bytes, nt * ng, nt * ng * sk * 128 * 64 * 4):
        sk, denied = 1, True
    xm, xn, gx = choose_xcd_array(g['mtiles'], ntl, N * H * W * Kc * 6.0, Nout * 9 * Kc * 6.0)
    return dict(mtiles=g['mtiles'], ntiles=ntl, xm=xm, xn=xn, gx=gx, sk=sk, ncls=ng, denied=denied, ncc=ncc)


def plan_tn(Cout, Cin, KH, KW, npix):
    """:1334-1343 with launch_tn's / the pair's 64 x 64 tile and target (:1367, :1564)"""
    target = slot_target(2.0 * npix * Cout * float(Cin) * KH * KW, 512)
    mt, ntl = cdiv(Cout, 64), cdiv(Cin, 64)
    nt = mt * ntl * KH * KW
    nkt = (npix + 31) // 32
    sk = (target + nt - 1) // nt
    sk = min(sk, nkt // 4)
    if sk >= 8:
        sk = (sk + 4) // 8 * 8
    sk = max(sk, 1)
    return dict(mtiles=mt, ntiles=ntl, nt=nt, nkt=nkt, sk=sk)


def out_hw(H, W, KH, KW, s, pad):
    return (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1


def fields(kind, bm, bn, nw, splitk, xm, xn, ncls, tn_splitk, grid):
    return dict(kind=kind, bm=bm, bn=bn, nw=nw, splitk=splitk, xm=xm, xn=xn, ncls=ncls, tn_splitk=tn_splitk, grid=min(grid, 0x7fffffff))


def _xcd_paths(pl):
    out = ['xcd/%dx%d' % (pl['xm'], pl['xn'])]
    if pl['gx'] > pl['mtiles'] * pl['ntiles']:
        out.append('xcd/padding_blocks')
    if pl['mtiles'] < pl['xm'] or pl['ntiles'] < pl['xn']:
        out.append('xcd/mtiles_lt_xm')
    return out


def _splitk_paths(pl, nkt):
    if pl['denied']:
        return ['splitk/denied']
    if pl['sk'] == 1:
        return ['splitk/1']
    return ['splitk/even' if nkt % pl['sk'] == 0 else 'splitk/ragged_last_slice']


def dgrad_classes(KH, KW, s, pad, IH, IW, Kc):
    """The parity classes as p3_nt_body derives them (:393-406): [(py, px, nty, ntx, OHc, OWc, nkt)] in class order."""
    out = []
    for cls in range(s * s):
        py, px = cls // s, cls % s
        kh0, kw0 = (py + pad) % s, (px + pad) % s
        nty = (KH - kh0 + s - 1) // s if kh0 < KH else 0
        ntx = (KW - kw0 + s - 1) // s if kw0 < KW else 0
        out.append((py, px, nty, ntx, (IH - py + s - 1) // s, (IW - px + s - 1) // s, nty * ntx * Kc // 32))
    return out


def _nt_launch(M, N, Kc, KH, KW, s, pad, nkt, nclass, ngroups, forward, tap_mode, ws_bytes, paired=False):
    """launch_nt (:1260-1279), or the pair's fixed 64 x 64 plan (:1575) -> (plan, bm, bn, nw, one)"""
    cfg = 3
    if not paired and forward and nclass <= 1 and ((M >= 65536 and N >= 128) or (M >= 16384 and N >= 256 and nkt <= 16)):   # :1269
        cfg = 1
    bm, bn, nw = (128, 128, 8) if cfg == 1 else (64, 64, 4)
    flops = 2.0 * M * N * nkt * 32.0 * (nclass if nclass > 1 else 1)                                                       # :1223
    sk = nt_splitk(M, N, nkt, bm, bn, slot_target(flops, 512 if cfg == 3 else 256))                                        # :1272
    pl = plan_nt(M, N, Kc, KH, KW, nkt, nclass, ngroups, bm, bn, sk, ws_bytes)
    one = KH * KW == 1 and pad == 0 and nclass <= 1 and (tap_mode == 0 or s == 1)                                         # :1235
    return pl, bm, bn, nw, one


def _nt_paths(pl, M, N, nkt, bm, bn, nw, one):
    p = ['nt/%s%s' % ('128x128x8w' if bm == 128 else '64x64', '/ONE' if one else '')]
    if M % bm:
        p.append('nt/ragged_M')
    if N % 16:
        p.append('nt/ragged_N16')
    if N % bn:
        p.append('nt/ragged_N64')
    return p + _xcd_paths(pl) + _splitk_paths(pl, nkt)


def _fwd_tap_path(KH, KW, s, pad, patch):
    if (KH, KW) == (1, 1):
        return 'fwd/1x1s%d' % s
    if (KH, KW) == (3, 3):
        if s == 2:
            return 'fwd/3x3s2'
        return {0: 'fwd/3x3p0', 1: None if patch else 'fwd/3x3s1_nonpatch', 2: 'fwd/3x3p2'}[pad]
    return {(5, 5): 'fwd/5x5p2', (2, 2): 'fwd/2x2s2', (1, 3): 'fwd/1x3', (3, 1): 'fwd/3x1', (4, 8): 'fwd/4x8'}[(KH, KW)]


def _c3_paths(g, pl, N, Kc, Nout, flip, grouped):
    p = ['c3/geom/%dx%dx%d' % (g['PW'], g['PH'], g['NP'])]
    if (N * g['ppi']) % g['NP']:
        p.append('c3/half_empty_tile')
    if g['ppr'] > 1 and g['ppi'] > g['ppr']:
        p.append('c3/interior_halo')
    if Kc == 32:
        p.append('c3/ncc1')
    if Nout % 64:
        p.append('c3/ragged_Nout')
    if pl['sk'] > 1:
        p.append('c3/splitk')
    if flip:
        p.append('c3/flip')
    if grouped:
        p.append('c3/grouped')
    return p + _xcd_paths(pl) + (['splitk/denied'] if pl['denied'] else [])


def model_fwd(geom, dual=False, ws_bytes=WS_BYTES_DEFAULT):
    """p3_conv2d_fwd_impl (:1471-1508) -> (fields, paths)"""
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    ng = 2 if dual else 0
    if (KH, KW, s, pad) == (3, 3, 1, 1):
        g, why = c3_geometry(N, H, W)
        if g:
            pl = plan_c3(g, N, H, W, Ci, Co, ng, ws_bytes)
            paths = _c3_paths(g, pl, N, Ci, Co, False, dual) + (['dual/c3'] if dual else [])
            if dual and pl['sk'] > 1:
                paths.append('splitk/group2_slots')
            return fields(2, 128, 64, 4, pl['sk'], pl['xm'], pl['xn'], pl['ncls'], 0, pl['gx']), paths
        rej = ['c3/rejected/' + why] + (['c3/rejected/NG_gt_13'] if why == 'H_not_divisible' else [])
    else:
        rej = []
    M, nkt = N * OH * OW, KH * KW * Ci // 32
    pl, bm, bn, nw, one = _nt_launch(M, Co, Ci, KH, KW, s, pad, nkt, 0, ng, True, 0, ws_bytes)
    paths = rej + _nt_paths(pl, M, Co, nkt, bm, bn, nw, one) + [_fwd_tap_path(KH, KW, s, pad, False)]
    if dual:
        paths.append('dual/nt/128x128' if bm == 128 else ('dual/nt/ONE' if one else 'dual/nt'))
        if pl['sk'] > 1:
            paths.append('splitk/group2_slots')
    return fields(1, bm, bn, nw, pl['sk'], pl['xm'], pl['xn'], pl['ncls'], 0, pl['gx']), paths


def _dgrad_plan(geom, ws_bytes, paired):
    """setup_bwd_data (:1372-1408): the patch-or-gather choice and the class sizing.  geom is the FORWARD conv's: x [N,H,W,Ci] -> y [N,OH,OW,Co]."""
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    rej = []
    if (KH, KW, s, pad) == (3, 3, 1, 1) and OH == H and OW == W:
        g, why = c3_geometry(N, H, W)
        if g:
            return 'c3', g, plan_c3(g, N, H, W, Co, Ci, 0, ws_bytes), None, rej
        rej = ['c3/rejected/' + why] + (['c3/rejected/NG_gt_13'] if why == 'H_not_divisible' else [])
    if s == 1:
        M, nkt, nclass = N * H * W, KH * KW * Co // 32, 1                                       # :1399
    else:
        M = N * cdiv(H, s) * cdiv(W, s)                                                         # :1403
        nkt = max(1, cdiv(KH, s) * cdiv(KW, s) * Co // 32)                                     # :1404-1405
        nclass = s * s
    pl, bm, bn, nw, one = _nt_launch(M, Ci, Co, KH, KW, s, pad, nkt, nclass, 0, False, 1, ws_bytes, paired)
    return 'nt', None, pl, (M, nkt, nclass, one), rej


def _dgrad_paths(geom, kind, g, pl, extra, rej):
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    if kind == 'c3':
        return _c3_paths(g, pl, N, Co, Ci, True, False)
    M, nkt, nclass, one = extra
    p = rej + _nt_paths(pl, M, Ci, nkt, 64, 64, 4, one)
    if s == 1:
        p.append({(1, 1): 'dgrad/s1_1x1', (3, 3): 'dgrad/s1_3x3_nonpatch', (5, 5): 'dgrad/s1_5x5'}.get((KH, KW), 'dgrad/s1_other'))
    else:
        cl = dgrad_classes(KH, KW, s, pad, H, W, Co)
        if (KH, KW) == (1, 1):
            p.append('dgrad/s2_1x1')
        elif (KH, KW) == (2, 2):
            p.append('dgrad/s2_2x2')
        elif (KH, KW) == (3, 3):
            p.append('dgrad/s2_3x3p0' if pad == 0 else ('dgrad/s2_3x3_even' if H % 2 == 0 and W % 2 == 0 else 'dgrad/s2_3x3_odd'))
        else:
            p.append('dgrad/s2_other')
        if (OH - 1) * s - pad + KH < H or (OW - 1) * s - pad + KW < W:
            p.append('dgrad/s2_unused_border')
        if pl['sk'] > 1:
            if any(c[6] == 0 for c in cl):
                p.append('splitk/class_nkt_0')
            if any(0 < c[6] <= cdiv(c[6], pl['sk']) * (pl['sk'] - 1) for c in cl):
                p.append('splitk/class_shorter_than_slice')
    return p


def model_dgrad(geom, ws_bytes=WS_BYTES_DEFAULT):
    """ldetr_p3_conv2d_bwd_data (:1527-1536) -> (fields, paths)"""
    kind, g, pl, extra, rej = _dgrad_plan(geom, ws_bytes, False)
    paths = _dgrad_paths(geom, kind, g, pl, extra, rej)
    if kind == 'c3':
        return fields(2, 128, 64, 4, pl['sk'], pl['xm'], pl['xn'], 1, 0, pl['gx']), paths
    return fields(1, 64, 64, 4, pl['sk'], pl['xm'], pl['xn'], pl['ncls'], 0, pl['gx']), paths


def _wgrad_paths(geom, pt, row_scale, accumulate):
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    npix = N * OH * OW
    p = ['tn/splitk1' if pt['sk'] == 1 else ('tn/splitk_lt8' if pt['sk'] < 8 else 'tn/splitk_mult8')]
    if npix % 32:
        p.append('tn/ragged_pixel_tile')
    if Ci == 32 and Co == 32:
        p.append('tn/C32')
    if Ci % 64 == 32 and Ci > 64 or Co % 64 == 32 and Co > 64:
        p.append('tn/C96')
    if s == 2:
        p.append('tn/stride2')
    if pad > 0:
        p.append('tn/padded_taps')
    p.append('tn/row_scale' if row_scale else 'tn/no_row_scale')
    if accumulate:
        p.append('tn/accumulate')
    if npix > (1 << 20):
        p.append('tn/big_pixel_index')
    return p


def model_wgrad(geom, row_scale=False, accumulate=False):
    """ldetr_p3_conv2d_bwd_weight (:1538-1545), launch_tn (:1360-1369), launch_tn_cfg (:1346-1358)"""
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    pt = plan_tn(Co, Ci, KH, KW, N * OH * OW)
    return fields(3, 64, 64, 4, 0, 0, 0, 1, pt['sk'], pt['nt']), _wgrad_paths(geom, pt, row_scale, accumulate)


def model_pair(geom, ws_bytes=WS_BYTES_DEFAULT, row_scale=False, accumulate=False):
    """ldetr_p3_conv2d_bwd_pair (:1549-1595): one grid of n_tn weight-gradient blocks padded to a multiple of 8, then the data gradient's."""
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    kind, g, pl, extra, rej = _dgrad_plan(geom, ws_bytes, True)
    pt = plan_tn(Co, Ci, KH, KW, N * OH * OW)                                                   # :1564
    n_tn = pt['sk'] * pt['nt']                                                                  # :1565
    n_tn_pad = (n_tn + 7) // 8 * 8
    paths = _dgrad_paths(geom, kind, g, pl, extra, rej) + _wgrad_paths(geom, pt, row_scale, accumulate)
    if n_tn % 8:
        paths.append('pair/padding_blocks')
    if kind == 'c3':
        paths.append('pair/c3')
        return fields(5, 128, 64, 4, pl['sk'], pl['xm'], pl['xn'], 1, pt['sk'], n_tn_pad + pl['gx'] * pl['sk']), paths             # :1573
    paths.append('pair/nt/classes' if pl['ncls'] > 1 else ('pair/nt/ONE' if extra[3] else 'pair/nt'))
    return fields(4, 64, 64, 4, pl['sk'], pl['xm'], pl['xn'], pl['ncls'], pt['sk'], n_tn_pad + pl['gx'] * pl['sk'] * pl['ncls']), paths  # :1583


# ================================================================================================================ path names
C3_GEOMETRIES = [(4, 32, 1), (8, 8, 2), (8, 16, 1), (16, 8, 1)]      # what c3_accepted_geometries() finds (asserted by the CPU file)
EPI_NAMES = ['alpha', 'scale_only', 'bias_only', 'scale_bias', 'res_p3', 'res_f32', 'res_both', 'relu', 'mask', 'relu_mask', 'store/f32', 'store/p3',
             'store/both']
REJECTS = ['fwd/cin_multiple', 'fwd/cout_multiple', 'fwd/taps_gt_32', 'fwd/stride3', 'fwd/pad_ge_k', 'fwd/null_output', 'fwd/null_operand', 'fwd/31bit_x',
           'fwd/31bit_w', 'dual/null_second_set', 'dual/null_second_output', 'dgrad/cout_multiple', 'dgrad/cin_multiple', 'dgrad/taps_gt_32', 'dgrad/stride3',
           'dgrad/pad_ge_k', 'dgrad/null_output', 'dgrad/31bit_dy', 'dgrad/31bit_w', 'wgrad/cin_multiple', 'wgrad/cout_multiple', 'wgrad/stride3',
           'wgrad/pad_ge_k', 'wgrad/null_output', 'wgrad/31bit_x', 'wgrad/31bit_dy', 'pair/oh_mismatch', 'pair/null_dw', 'pair/cin_multiple']
P3_PATHS = (
    ['nt/64x64', 'nt/64x64/ONE', 'nt/128x128x8w', 'nt/128x128x8w/ONE', 'nt/ragged_M', 'nt/ragged_N16', 'nt/ragged_N64',
     'xcd/8x1', 'xcd/4x2', 'xcd/2x4', 'xcd/1x8', 'xcd/padding_blocks', 'xcd/mtiles_lt_xm',
     'splitk/1', 'splitk/even', 'splitk/ragged_last_slice', 'splitk/denied', 'splitk/class_nkt_0', 'splitk/class_shorter_than_slice', 'splitk/group2_slots',
     'fwd/1x1s1', 'fwd/1x1s2', 'fwd/3x3s1_nonpatch', 'fwd/3x3s2', 'fwd/3x3p0', 'fwd/3x3p2', 'fwd/5x5p2', 'fwd/2x2s2', 'fwd/1x3', 'fwd/3x1', 'fwd/4x8',
     'dgrad/s1_1x1', 'dgrad/s1_3x3_nonpatch', 'dgrad/s1_5x5', 'dgrad/s1_other', 'dgrad/s2_1x1', 'dgrad/s2_3x3_even', 'dgrad/s2_3x3_odd', 'dgrad/s2_2x2',
     'dgrad/s2_other', 'dgrad/s2_unused_border', 'dgrad/s2_3x3p0']
    + ['c3/geom/%dx%dx%d' % g for g in C3_GEOMETRIES]
    + ['c3/rejected/W_not_multiple_of_PW', 'c3/rejected/NG_gt_13', 'c3/rejected/H_not_divisible', 'c3/half_empty_tile', 'c3/interior_halo', 'c3/ncc1',
       'c3/ragged_Nout', 'c3/splitk', 'c3/flip', 'c3/grouped',
       'tn/splitk1', 'tn/splitk_lt8', 'tn/splitk_mult8', 'tn/ragged_pixel_tile', 'tn/C32', 'tn/C96', 'tn/stride2', 'tn/padded_taps', 'tn/row_scale',
       'tn/no_row_scale', 'tn/accumulate', 'tn/big_pixel_index',
       'pair/nt', 'pair/nt/ONE', 'pair/nt/classes', 'pair/c3', 'pair/padding_blocks',
       'dual/nt', 'dual/nt/ONE', 'dual/nt/128x128', 'dual/c3', 'dual/different_epilogues']
    + ['epi/%s@%s' % (e, k) for k in ('nt', 'c3') for e in EPI_NAMES]
    + ['cold/nt64', 'cold/nt128', 'cold/nt/ONE', 'cold/c3', 'cold/c3/flip', 'cold/tn', 'cold/pair', 'cold/dual']
    + ['reject/' + r for r in REJECTS])
# Reachable only through the development switches (LDETR_DEBUG="P3_TILE=2|4", "P3_WTILE=..", "P3_PAIR=0"): no table case may yield them.
P3_UNREACHABLE = ['nt/128x64x4w', 'nt/128x128x4w', 'tn/128x128', 'tn/128x64', 'pair/two_launches']


# ================================================================================================================ epilogues
def epi(alpha=False, scale=False, bias=False, res_p3=False, res_f32=False, relu=False, mask=False, store='both'):
    return dict(alpha=alpha, scale=scale, bias=bias, res_p3=res_p3, res_f32=res_f32, relu=relu, mask=mask, store=store)


EPI_NONE = epi()
EPIS = dict(
    none=EPI_NONE,
    alpha_f32=epi(alpha=True, store='f32'),
    scale_p3=epi(scale=True, store='p3'),
    bias_relu=epi(bias=True, relu=True),
    scale_bias_resp3=epi(scale=True, bias=True, res_p3=True),
    resf32_mask=epi(res_f32=True, mask=True, store='f32'),
    full=epi(alpha=True, scale=True, bias=True, res_p3=True, res_f32=True, relu=True, mask=True),
    resp3_mask=epi(res_p3=True, mask=True),                      # the trunk's data-gradient epilogue
    bn_res_relu=epi(scale=True, bias=True, res_p3=True, relu=True),     # the trunk's forward epilogue
)


def epi_paths(e, kernel):
    p = []
    if e['alpha']:
        p.append('alpha')
    if e['scale'] or e['bias']:
        p.append('scale_bias' if e['scale'] and e['bias'] else ('scale_only' if e['scale'] else 'bias_only'))
    if e['res_p3'] or e['res_f32']:
        p.append('res_both' if e['res_p3'] and e['res_f32'] else ('res_p3' if e['res_p3'] else 'res_f32'))
    if e['relu'] or e['mask']:
        p.append('relu_mask' if e['relu'] and e['mask'] else ('relu' if e['relu'] else 'mask'))
    p.append('store/' + e['store'])
    return ['epi/%s@%s' % (n, kernel) for n in p]


def additive_terms(e):
    return int(e['bias']) + int(e['res_p3']) + int(e['res_f32'])


# ================================================================================================================ case tables
def case(name, entry, geom, epi=EPI_NONE, classes=('select', 'select_w', 'grid', 'rounding'), ws=True, row_scale=False, accumulate=False, epi2=None,
         cold=False):
    """entry: fwd | dual | dgrad | wgrad | pair.  geom = (N, H, W, Cin, Cout, KH, KW, stride, pad) of the FORWARD convolution, whichever entry runs.
    ws=False: the split-K workspace is unregistered for the launch.  epi2: the second set's epilogue of a dual case."""
    if additive_terms(epi) > 1 or (epi2 is not None and additive_terms(epi2) > 1):
        classes = tuple(c for c in classes if c not in ('select', 'select_w'))
    if entry in ('wgrad', 'pair'):          # (the weight gradient has no second exact orientation: its dY is the one-hot operand of `select`)
        classes = tuple(c for c in classes if c != 'select_w')
    return dict(name=name, entry=entry, geom=tuple(geom), epi=epi, classes=tuple(classes), ws=ws, row_scale=row_scale, accumulate=accumulate, epi2=epi2, cold=cold)


E_NT = (2, 9, 9, 64, 72, 3, 3, 1, 1)           # gather kernel (9 is no patch width), three ragged row tiles, Cout = 72: ragged_N16 and ragged_N64
E_C3 = (3, 8, 8, 64, 72, 3, 3, 1, 1)           # patch kernel 8 x 8 x 2 with a half-empty last tile and a ragged channel tile
G128 = (19, 30, 30, 32, 256, 3, 3, 1, 1)       # M = 17100 >= 16384, N = 256, nkt = 9 <= 16: the 128x128 / 8-wave tile at its threshold, on the tap-walking loop
G128_ONE = (16, 32, 32, 32, 256, 1, 1, 1, 0)   # M = 16384 exactly: the same tile on the plain-GEMM loop

FWD_CASES = [
    case('f_1x1s1', 'fwd', (1, 8, 8, 32, 64, 1, 1, 1, 0)),
    case('f_1x1s2', 'fwd', (3, 9, 11, 64, 40, 1, 1, 2, 0), EPIS['bn_res_relu']),
    case('f_3x3_nonpatch', 'fwd', E_NT),
    case('f_3x3s2', 'fwd', (2, 14, 10, 64, 64, 3, 3, 2, 1)),
    case('f_3x3p0', 'fwd', (2, 7, 9, 32, 64, 3, 3, 1, 0)),
    case('f_3x3p2', 'fwd', (2, 6, 7, 32, 64, 3, 3, 1, 2)),
    case('f_5x5p2', 'fwd', (1, 9, 8, 32, 32, 5, 5, 1, 2)),
    case('f_2x2s2', 'fwd', (2, 8, 10, 64, 32, 2, 2, 2, 0)),
    case('f_1x3', 'fwd', (2, 6, 9, 32, 64, 1, 3, 1, 0)),
    case('f_3x1', 'fwd', (2, 9, 6, 32, 64, 3, 1, 1, 0)),
    case('f_4x8p3', 'fwd', (2, 7, 12, 32, 64, 4, 8, 1, 3)),             # 32 taps: the last bit of the tap mask
    case('f_4x8s2p1', 'fwd', (2, 9, 14, 32, 40, 4, 8, 2, 1)),
    case('f_longK', 'fwd', (2, 9, 9, 512, 64, 3, 3, 1, 1), classes=('select', 'grid', 'rounding')),     # K = 4608 on three tiles: 16 even slices
    case('f_K1024_1x1', 'fwd', (2, 8, 8, 1024, 128, 1, 1, 1, 0), classes=('select', 'grid', 'rounding')),
    case('f_wide_N', 'fwd', (1, 4, 4, 32, 1024, 1, 1, 1, 0)),            # one row tile, 16 channel tiles: the XCD array turned to 1 x 8
    case('f_4x2', 'fwd', (4, 10, 10, 32, 128, 1, 1, 1, 0)),
    case('f_denied', 'fwd', (2, 9, 9, 512, 64, 3, 3, 1, 1), ws=False, classes=('select', 'rounding')),
    case('f_128', 'fwd', G128, EPIS['bias_relu'], classes=('select', 'rounding')),
    case('f_128_one', 'fwd', G128_ONE, classes=('select', 'select_w')),
    # ---- patch kernel: every geometry c3_geometry accepts, and what it rejects
    case('c_16x8x1', 'fwd', (1, 8, 16, 32, 64, 3, 3, 1, 1)),
    case('c_8x16x1', 'fwd', (2, 16, 8, 64, 40, 3, 3, 1, 1)),
    case('c_8x8x2_half', 'fwd', E_C3),
    case('c_4x32x1', 'fwd', (2, 32, 4, 64, 64, 3, 3, 1, 1)),
    case('c_interior', 'fwd', (1, 16, 32, 128, 64, 3, 3, 1, 1)),         # 2 x 2 patches per image: halos that overlap the neighbouring patch on every side
    case('c_8x24', 'fwd', (1, 24, 8, 64, 64, 3, 3, 1, 1)),                # H = 24: the first patch height 16 does not divide, 8 does
    case('c_splitk', 'fwd', (2, 8, 8, 512, 64, 3, 3, 1, 1), classes=('select', 'grid', 'rounding')),
    case('c_denied', 'fwd', (2, 8, 8, 512, 64, 3, 3, 1, 1), ws=False, classes=('select',)),
    case('c_rej_NG', 'fwd', (2, 4, 4, 64, 64, 3, 3, 1, 1)),               # 4 x 4 images: NG = 18 > 13, the gather kernel
    case('c_rej_W12', 'fwd', (1, 8, 12, 32, 64, 3, 3, 1, 1)),
    case('c_rej_W24', 'fwd', (1, 8, 24, 32, 64, 3, 3, 1, 1), classes=('select',)),
    case('c_rej_H12', 'fwd', (1, 12, 16, 32, 64, 3, 3, 1, 1)),
]
EPI_CASES = ([case('e_nt_' + k, 'fwd', E_NT, EPIS[k]) for k in ('alpha_f32', 'scale_p3', 'bias_relu', 'scale_bias_resp3', 'resf32_mask', 'full')]
             + [case('e_c3_' + k, 'fwd', E_C3, EPIS[k]) for k in ('alpha_f32', 'scale_p3', 'bias_relu', 'scale_bias_resp3', 'resf32_mask', 'full')])
DGRAD_CASES = [
    case('d_s1_1x1', 'dgrad', (1, 8, 8, 32, 32, 1, 1, 1, 0)),
    case('d_s1_3x3_nonpatch', 'dgrad', (2, 9, 9, 40, 96, 3, 3, 1, 1), EPIS['resp3_mask']),
    case('d_s1_5x5', 'dgrad', (1, 9, 8, 32, 32, 5, 5, 1, 2)),
    case('d_s1_1x3', 'dgrad', (2, 6, 9, 32, 64, 1, 3, 1, 0)),
    case('d_s1_4x8p3', 'dgrad', (2, 7, 12, 32, 64, 4, 8, 1, 3)),
    case('d_s1_3x3p2', 'dgrad', (2, 6, 7, 32, 64, 3, 3, 1, 2)),
    case('d_s2_1x1', 'dgrad', (2, 9, 11, 64, 256, 1, 1, 2, 0), EPIS['resp3_mask']),     # three classes without taps, split-K 2: nkt = 0 slices
    case('d_s2_3x3_even', 'dgrad', (2, 16, 16, 64, 128, 3, 3, 2, 1)),
    case('d_s2_3x3_odd', 'dgrad', (2, 13, 9, 64, 64, 3, 3, 2, 1), EPIS['resp3_mask']),
    case('d_s2_2x2', 'dgrad', (2, 8, 10, 64, 32, 2, 2, 2, 0)),
    case('d_s2_2x2_border', 'dgrad', (2, 9, 11, 64, 32, 2, 2, 2, 0), EPIS['bias_relu']),  # row 8 and column 10 feed no output: dx there is the epilogue of zero
    case('d_s2_3x3p0', 'dgrad', (2, 9, 9, 32, 64, 3, 3, 2, 0)),
    case('d_s2_3x1', 'dgrad', (2, 9, 6, 32, 64, 3, 1, 2, 0)),
    case('d_s2_4x8p1', 'dgrad', (2, 9, 14, 32, 64, 4, 8, 2, 1)),
    case('d_s2_class_short', 'dgrad', (4, 30, 30, 256, 160, 3, 3, 2, 1), classes=('select', 'rounding')),   # split-K 4 over classes of 20 / 10 / 10 / 5 k-tiles
    case('d_c3_16x8', 'dgrad', (1, 8, 16, 64, 32, 3, 3, 1, 1)),
    case('d_c3_8x8x2', 'dgrad', (3, 8, 8, 40, 64, 3, 3, 1, 1), EPIS['resp3_mask']),
    case('d_c3_4x32', 'dgrad', (1, 32, 4, 64, 64, 3, 3, 1, 1)),
    case('d_c3_interior', 'dgrad', (1, 16, 32, 64, 128, 3, 3, 1, 1)),
]
BIG_PIX = (16645, 7, 9, 32, 32, 3, 3, 1, 1)     # npix = 1 048 635 > 2^20.  2^24 itself cannot be reached: the entry's 31-bit check on xbytes caps npix at
#                                                 11.1 M for 32 channels, and that case would need 2 GB of operands
WGRAD_CASES = [
    case('w_sk1_C32', 'wgrad', (1, 8, 8, 32, 32, 1, 1, 1, 0)),
    case('w_lt8_C96', 'wgrad', (3, 10, 11, 96, 64, 3, 3, 1, 1), row_scale=True),
    case('w_mult8', 'wgrad', (5, 15, 15, 32, 32, 1, 1, 1, 0), row_scale=True),
    case('w_stride2', 'wgrad', (2, 14, 10, 64, 64, 3, 3, 2, 1)),
    case('w_acc_4x8', 'wgrad', (2, 7, 12, 32, 64, 4, 8, 1, 3), accumulate=True, row_scale=True),
    case('w_s2_2x2_border', 'wgrad', (2, 9, 11, 64, 32, 2, 2, 2, 0)),
    case('w_big_pixel_index', 'wgrad', BIG_PIX, classes=('select',)),
]
PAIR_CASES = [
    case('p_nt', 'pair', (2, 9, 9, 64, 96, 3, 3, 1, 1), EPIS['resp3_mask'], row_scale=True, accumulate=True),
    case('p_nt_one', 'pair', (2, 8, 8, 64, 64, 1, 1, 1, 0)),
    case('p_classes', 'pair', (2, 13, 9, 64, 64, 3, 3, 2, 1), EPIS['resp3_mask'], row_scale=True),
    case('p_classes_1x1', 'pair', (2, 9, 11, 64, 256, 1, 1, 2, 0)),
    case('p_c3', 'pair', (3, 8, 8, 64, 64, 3, 3, 1, 1), EPIS['resp3_mask'], row_scale=True),
    case('p_c3_splitk', 'pair', (2, 16, 8, 64, 256, 3, 3, 1, 1)),
]
DUAL_CASES = [
    case('u_nt', 'dual', (2, 7, 9, 32, 64, 3, 3, 1, 0), EPIS['bias_relu'], epi2=EPIS['scale_p3']),
    case('u_nt_one', 'dual', (3, 9, 11, 64, 40, 1, 1, 2, 0), EPIS['alpha_f32'], epi2=EPIS['resf32_mask']),
    case('u_nt_splitk', 'dual', (2, 9, 9, 256, 64, 3, 3, 1, 1), EPIS['none'], epi2=EPIS['bias_relu'], classes=('select', 'grid', 'rounding')),
    case('u_nt_128', 'dual', G128, EPIS['none'], epi2=EPIS['bias_relu'], classes=('select',)),
    case('u_c3', 'dual', E_C3, EPIS['bn_res_relu'], epi2=EPIS['alpha_f32'], classes=('grid', 'rounding')),
    case('u_c3_splitk', 'dual', (2, 8, 8, 256, 64, 3, 3, 1, 1), EPIS['scale_p3'], epi2=EPIS['none'], classes=('select', 'rounding')),
]
# Non-finite operands (the cold path): criterion of test_p3_gpu.py::test_p3_non_finite_operands_give_the_fp32_convolutions_classes
COLD_CASES = [
    case('k_nt64', 'fwd', (2, 9, 9, 64, 64, 3, 3, 1, 1), cold=True, classes=('rounding',)),
    case('k_nt128', 'fwd', G128, cold=True, classes=('rounding',)),
    case('k_nt_one', 'fwd', (2, 8, 8, 64, 64, 1, 1, 1, 0), cold=True, classes=('rounding',)),
    case('k_c3', 'fwd', (3, 8, 8, 64, 64, 3, 3, 1, 1), cold=True, classes=('rounding',)),
    case('k_c3_flip', 'dgrad', (3, 8, 8, 64, 64, 3, 3, 1, 1), cold=True, classes=('rounding',)),
    case('k_tn', 'wgrad', (3, 10, 11, 64, 64, 3, 3, 1, 1), cold=True, classes=('rounding',)),
    case('k_pair', 'pair', (2, 9, 9, 64, 64, 3, 3, 1, 1), cold=True, classes=('rounding',)),
    case('k_dual', 'dual', (2, 9, 9, 64, 64, 3, 3, 1, 1), cold=True, classes=('rounding',), epi2=EPI_NONE),
]
VALUE_CASES = FWD_CASES + EPI_CASES + DGRAD_CASES + WGRAD_CASES + PAIR_CASES + DUAL_CASES
ALL_CASES = VALUE_CASES + COLD_CASES
BY_NAME = {c['name']: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def entry_accepts(entry, geom, null=(), oh_delta=0):
    """The LDETR_CHECKs of the five conv entries (:1374-1376, :1395, :1413-1417, :1475-1480, :1521, :1558), restated: True when the call would launch.
    Every check is on the host and precedes the launch; the host never reads through an operand pointer, so a rejected call touches no buffer."""
    N, H, W, Ci, Co, KH, KW, s, pad = geom
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    lim = 0x7fffffff
    def fwd_ok():
        if 'x' in null or 'w' in null or 'out' in null:
            return False
        if entry == 'dual' and ('x2' in null or 'w2' in null or 'out2' in null):
            return False
        if not (Ci % 32 == 0 and Co % 8 == 0 and KH * KW <= 32 and pad < KH and pad < KW and s in (1, 2)):
            return False
        return N * H * W * Ci * 6 + (pad * W + pad) * Ci * 6 < lim and Co * KH * KW * Ci * 6 < lim and N * OH * OW * Co * 6 < (1 << 40)
    def dgrad_ok():
        if 'dy' in null or 'w' in null or 'out' in null:
            return False
        if not (Co % 32 == 0 and Ci % 8 == 0 and KH * KW <= 32 and pad < KH and pad < KW and s in (1, 2)):
            return False
        dyb, wb = N * (OH + oh_delta) * OW * Co * 6, Ci * KH * KW * Co * 6
        if (KH, KW, s, pad) == (3, 3, 1, 1) and OH + oh_delta == H and OW == W and dyb < lim and wb < lim and c3_geometry(N, H, W)[0]:
            return True
        return dyb + ((KH - 1) * OW + KW - 1) * Co * 6 < lim and wb < lim
    def wgrad_ok():
        if 'x' in null or 'dy' in null or 'dw' in null:
            return False
        if not (Ci % 32 == 0 and Co % 32 == 0 and pad < KH and pad < KW and s in (1, 2)):
            return False
        # (N * OH * OW < 2^24 is implied by dybytes < 2^31 at Cout >= 32 -- 11.1 M pixels -- so that clause has no case of its own)
        return N * H * W * Ci * 6 + (pad * W + pad) * Ci * 6 < lim and N * OH * OW * Co * 6 < lim and N * OH * OW < (1 << 24)
    if entry in ('fwd', 'dual'):
        return fwd_ok()
    if entry == 'dgrad':
        return dgrad_ok()
    if entry == 'wgrad':
        return wgrad_ok()
    return dgrad_ok() and wgrad_ok() and oh_delta == 0


_RB = (1, 8, 8, 32, 32, 3, 3, 1, 1)


def _rg(**kw):
    g = dict(zip('N H W Ci Co KH KW s pad'.split(), _RB))
    g.update(kw)
    return tuple(g[k] for k in 'N H W Ci Co KH KW s pad'.split())


def reject(name, entry, geom=_RB, null=(), oh_delta=0):
    return dict(name=name, entry=entry, geom=geom, null=tuple(null), oh_delta=oh_delta)


# One case per LDETR_CHECK clause.  The size limits are passed as dimensions only: see entry_accepts.
REJECT_CASES = [
    reject('fwd/cin_multiple', 'fwd', _rg(Ci=40)), reject('fwd/cout_multiple', 'fwd', _rg(Co=36)), reject('fwd/taps_gt_32', 'fwd', _rg(KH=5, KW=7)),
    reject('fwd/stride3', 'fwd', _rg(s=3)), reject('fwd/pad_ge_k', 'fwd', _rg(pad=3)), reject('fwd/null_output', 'fwd', null=('out',)),
    reject('fwd/null_operand', 'fwd', null=('x',)), reject('fwd/31bit_x', 'fwd', _rg(N=4096, H=64, W=64)),
    reject('fwd/31bit_w', 'fwd', _rg(Co=1 << 20, Ci=1024, KH=1, KW=1, pad=0)),
    reject('dual/null_second_set', 'dual', null=('x2',)), reject('dual/null_second_output', 'dual', null=('out2',)),
    reject('dgrad/cout_multiple', 'dgrad', _rg(Co=40)), reject('dgrad/cin_multiple', 'dgrad', _rg(Ci=36)), reject('dgrad/taps_gt_32', 'dgrad', _rg(KH=5, KW=7)),
    reject('dgrad/stride3', 'dgrad', _rg(s=3)), reject('dgrad/pad_ge_k', 'dgrad', _rg(pad=3)), reject('dgrad/null_output', 'dgrad', null=('out',)),
    reject('dgrad/31bit_dy', 'dgrad', _rg(N=4096, H=64, W=64)), reject('dgrad/31bit_w', 'dgrad', _rg(Co=1 << 20, Ci=1024, KH=1, KW=1, pad=0)),
    reject('wgrad/cin_multiple', 'wgrad', _rg(Ci=40)), reject('wgrad/cout_multiple', 'wgrad', _rg(Co=40)), reject('wgrad/stride3', 'wgrad', _rg(s=3)),
    reject('wgrad/pad_ge_k', 'wgrad', _rg(pad=3)), reject('wgrad/null_output', 'wgrad', null=('dw',)), reject('wgrad/31bit_x', 'wgrad', _rg(N=4096, H=64, W=64)),
    reject('wgrad/31bit_dy', 'wgrad', _rg(N=64, Co=1 << 17)),
    reject('pair/oh_mismatch', 'pair', oh_delta=1), reject('pair/null_dw', 'pair', null=('dw',)), reject('pair/cin_multiple', 'pair', _rg(Ci=40)),
]
assert [r['name'] for r in REJECT_CASES] == REJECTS


def model(c, ws_bytes=WS_BYTES_DEFAULT):
    """-> (the ten fields of ldetr_p3_last_launch, path names) of a table case."""
    wsb = ws_bytes if c['ws'] else 0
    if c['entry'] in ('fwd', 'dual'):
        f, p = model_fwd(c['geom'], c['entry'] == 'dual', wsb)
    elif c['entry'] == 'dgrad':
        f, p = model_dgrad(c['geom'], wsb)
    elif c['entry'] == 'wgrad':
        f, p = model_wgrad(c['geom'], c['row_scale'], c['accumulate'])
    else:
        f, p = model_pair(c['geom'], wsb, c['row_scale'], c['accumulate'])
    p = list(p)
    if c['entry'] != 'wgrad':
        kern = 'c3' if f['kind'] in (2, 5) else 'nt'
        p += epi_paths(c['epi'], kern)
        if c['epi2'] is not None:
            p += epi_paths(c['epi2'], kern)
            if c['epi2'] != c['epi']:
                p.append('dual/different_epilogues')
    if c['cold']:
        if c['entry'] == 'dual':
            p.append('cold/dual')
        elif c['entry'] == 'pair':
            p += ['cold/pair', 'cold/tn']
        elif c['entry'] == 'wgrad':
            p.append('cold/tn')
        elif f['kind'] == 2:
            p.append('cold/c3/flip' if c['entry'] == 'dgrad' else 'cold/c3')
        else:
            p.append('cold/nt/ONE' if any(x.endswith('/ONE') and x.startswith('nt/') for x in p) else ('cold/nt128' if f['bm'] == 128 else 'cold/nt64'))
    return f, p


def reduction_length(c):
    """K of the case's contraction per output family -> dict(y= / dx= / dw=)."""
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    return dict(y=KH * KW * Ci, dx=KH * KW * Co, dw=N * OH * OW)


def k_bucket(K):
    return 256 if K <= 256 else (1024 if K <= 1024 else 4608)


# ================================================================================================================ inputs
def _gen(c, cls, salt=''):
    return torch.Generator().manual_seed(zlib.crc32(('%s/%s/%s' % (c['name'], cls, salt)).encode()))


def full_mantissa(g, shape, emin, emax):
    """fp32 values with random 24-bit mantissas, exponents uniform in [emin, emax], random signs."""
    m = (1.0 + torch.rand(shape, generator=g, dtype=F64)).to(F32)
    e = torch.randint(emin, emax + 1, shape, generator=g).to(F32)
    sgn = torch.randint(0, 2, shape, generator=g).to(F32) * 2 - 1
    return m * torch.exp2(e) * sgn


def _arbitrary(g, shape, wide):
    """The arbitrary operand of the select classes.  wide: exponents -60..60 and a few values at and next to FLT_MAX (the one-hot operand and the
    epilogue then only scale DOWN, so every product stays finite); narrow (an additive term follows): |v| in [2^-8, 2^9), so that the float64 sum with
    the term is exact."""
    if not wide:
        return full_mantissa(g, shape, -8, 8)
    v = full_mantissa(g, shape, -60, 60)
    flat = v.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:6]
    flat[idx] = torch.tensor([FLT_MAX, -FLT_MAX, FLT_MAX * (1 - 2.0 ** -9), -FLT_MAX * (1 - 2.0 ** -20), 3.3895e38, 2.0 ** 127], dtype=F32)[:idx.numel()]
    return v


def _pow2(g, shape, emin, emax):
    e = torch.randint(emin, emax + 1, shape, generator=g).to(F32)
    sgn = torch.randint(0, 2, shape, generator=g).to(F32) * 2 - 1
    return torch.exp2(e) * sgn


def _grid_values(g, shape, big_share):
    """Integers: mostly +-1..3 (hi plane only), a share of +-(256 + b), b odd in 1..7 (9 significant bits: hi and mid plane)."""
    small = torch.randint(1, 4, shape, generator=g).to(F32)
    big = 256.0 + (torch.randint(0, 4, shape, generator=g).to(F32) * 2 + 1)
    sgn = torch.randint(0, 2, shape, generator=g).to(F32) * 2 - 1
    return torch.where(torch.rand(shape, generator=g) < big_share, big, small) * sgn


def _rounding(g, shape, sigma=0.5):
    return (torch.randn(shape, generator=g, dtype=F32) * torch.exp(sigma * torch.randn(shape, generator=g, dtype=F32))).contiguous()


def _grid_shares(K):
    """Shares of 9-bit values on either side such that sum |terms| stays below 2^21 (a factor 8 is left for the epilogue: |alpha * scale| <= 4, bias,
    residuals): K x (9 + 2 x 3 x 263 x p + 263^2 x p^2) < 2^21."""
    p = 1.0
    while K * (9 + 1578 * p + 69169 * p * p) * 1.3 > 2 ** 21 and p > 1e-4:
        p *= 0.5
    return p


def make_inputs(c, cls, which=0):
    """-> dict of fp32 CPU tensors: x [N,H,W,Ci], w [Co,KH,KW,Ci], dy [N,OH,OW,Co], and the epilogue / scale operands of the case.  which = 1: the second
    operand set of a dual case.  Deterministic in (case, class, which)."""
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    g = _gen(c, cls, str(which))
    e = c['epi2'] if (which == 1 and c['epi2'] is not None) else c['epi']
    entry = c['entry']
    t = {}
    grad = entry in ('dgrad', 'wgrad', 'pair')
    wide = additive_terms(e) == 0 and not c['accumulate']
    K = reduction_length(c)
    if cls == 'select':
        if entry in ('fwd', 'dual'):
            t['x'] = _arbitrary(g, (N, H, W, Ci), wide)
            w = torch.zeros(Co, KH * KW, Ci)
            co = torch.arange(Co)
            w[co, (co * 5 + 1) % (KH * KW), (co * 7 + 3) % Ci] = _pow2(g, (Co,), -3, -1)
            t['w'] = w.reshape(Co, KH, KW, Ci)
        else:
            if entry in ('dgrad', 'pair'):      # one (co, tap) per INPUT channel: the rows of the data gradient's weight image
                w = torch.zeros(Co, KH * KW, Ci)
                ci = torch.arange(Ci)
                w[(ci * 7 + 3) % Co, (ci * 5 + 1) % (KH * KW), ci] = _pow2(g, (Ci,), -3, -1)
                t['w'] = w.reshape(Co, KH, KW, Ci)
            if entry == 'pair':
                # the pair shares dy: arbitrary for the data gradient, so the weight gradient's exact operand is X -- one non-zero pixel per INPUT channel
                t['dy'] = _arbitrary(g, (N, OH, OW, Co), wide)
                x = torch.zeros(N * H * W, Ci)
                pix = _select_pixels(N * H * W, Ci, g, H * W)
                x[pix, torch.arange(Ci)] = _pow2(g, (Ci,), -3, -1)
                t['x'] = x.reshape(N, H, W, Ci)
            elif entry == 'dgrad':
                t['dy'] = _arbitrary(g, (N, OH, OW, Co), wide)
            else:                               # wgrad: one non-zero pixel of dY per output channel
                dy = torch.zeros(N * OH * OW, Co)
                pix = _select_pixels(N * OH * OW, Co, g, OH * OW)
                dy[pix, torch.arange(Co)] = _pow2(g, (Co,), -3, -1)
                t['dy'] = dy.reshape(N, OH, OW, Co)
                t['x'] = _arbitrary(g, (N, H, W, Ci), wide)
    elif cls == 'select_w':
        # activations on a lattice of period KH x KW (every window holds at most one), one channel each; arbitrary weights
        if entry in ('fwd', 'dual'):
            x = torch.zeros(N, H, W, Ci)
            yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
            on = ((yy % KH) == (KH // 2)) & ((xx % KW) == (KW // 2))
            ch = (yy * 5 + xx * 3) % Ci
            for n in range(N):
                vals = _pow2(g, (H, W), -3, -1)
                x[n].scatter_(2, ((ch + n) % Ci)[..., None].expand(H, W, 1), torch.where(on, vals, torch.zeros(()))[..., None])
            t['x'] = x
            t['w'] = _arbitrary(g, (Co, KH, KW, Ci), wide)
        else:
            dy = torch.zeros(N, OH, OW, Co)
            yy, xx = torch.arange(OH)[:, None], torch.arange(OW)[None, :]
            on = ((yy % KH) == (KH // 2)) & ((xx % KW) == (KW // 2))
            ch = (yy * 5 + xx * 3) % Co
            for n in range(N):
                vals = _pow2(g, (OH, OW), -3, -1)
                dy[n].scatter_(2, ((ch + n) % Co)[..., None].expand(OH, OW, 1), torch.where(on, vals, torch.zeros(()))[..., None])
            t['dy'] = dy
            t['w'] = _arbitrary(g, (Co, KH, KW, Ci), wide)
    elif cls == 'grid':
        if entry in ('fwd', 'dual'):
            p = _grid_shares(K['y'])
            t['x'], t['w'] = _grid_values(g, (N, H, W, Ci), p), _grid_values(g, (Co, KH, KW, Ci), p)
        else:
            p = _grid_shares(max(K['dx'] if entry != 'wgrad' else 0, K['dw'] if entry != 'dgrad' else 0))
            t['dy'] = _grid_values(g, (N, OH, OW, Co), p)
            if entry != 'wgrad':
                t['w'] = _grid_values(g, (Co, KH, KW, Ci), p)
            if entry != 'dgrad':
                t['x'] = _grid_values(g, (N, H, W, Ci), p)
    else:
        if entry in ('fwd', 'dual'):
            t['x'] = _rounding(g, (N, H, W, Ci))
            t['w'] = _rounding(g, (Co, KH, KW, Ci), 0.25) / math.sqrt(KH * KW * Ci)
        else:
            t['dy'] = _rounding(g, (N, OH, OW, Co))
            if entry != 'wgrad':
                t['w'] = _rounding(g, (Co, KH, KW, Ci), 0.25) / math.sqrt(KH * KW * Co)
            if entry != 'dgrad':
                t['x'] = _rounding(g, (N, H, W, Ci))
    # ---- epilogue operands (output of the fwd / data-gradient launch: rows x ch)
    oshape = (N, H, W, Ci) if grad else (N, OH, OW, Co)
    ch = oshape[-1]
    exact = cls != 'rounding'
    if entry != 'wgrad':
        if e['alpha']:
            t['alpha'] = {'select': -0.5, 'select_w': -0.5, 'grid': -2.0, 'rounding': -0.75}[cls]
        if e['scale']:
            t['scale'] = (_pow2(g, (ch,), -2, 0).abs() if cls in ('select', 'select_w') else _pow2(g, (ch,), 0, 1).abs()) if exact else torch.rand(ch, generator=g) + 0.5
        for k in ('bias', 'res_p3', 'res_f32'):
            if e[k]:
                shp = (ch,) if k == 'bias' else oshape
                if cls in ('select', 'select_w'):
                    t[k] = full_mantissa(g, shp, -4, 4)
                elif cls == 'grid':
                    t[k] = torch.randint(-1023, 1024, shp, generator=g).to(F32)
                else:
                    t[k] = torch.randn(shp, generator=g, dtype=F32)
        if e['mask']:
            m = torch.randn(oshape, generator=g, dtype=F32)
            m.view(-1)[:8] = torch.tensor([-0.0, 0.0, 0.0, -0.0, 1e-30, -1e-30, -1e-30, 1e-30])      # +-0 and the smallest magnitudes on even and odd channels
            t['mask'] = m
    if c['row_scale']:
        t['row_scale'] = (_pow2(g, (Co,), -1, 1).abs() if cls != 'grid' else _pow2(g, (Co,), 0, 1).abs()) if exact else torch.rand(Co, generator=g) + 0.5
    if c['accumulate']:
        shp = (Co, KH, KW, Ci)
        t['dw0'] = full_mantissa(g, shp, -4, 4) if cls in ('select', 'select_w') else (torch.randint(-1023, 1024, shp, generator=g).to(F32) if cls == 'grid'
                                                                                       else torch.randn(shp, generator=g, dtype=F32))
    return t


def _select_pixels(npix, nch, g, ohw=63):
    """One pixel per channel: pixels at which a float quotient pix * (1 / ohw) truncates to the wrong image index (fastdivmod's correction step, :791-796),
    the first, the last, the pixels around the 2^k boundaries that fit, the rest random."""
    pix = torch.arange(npix)
    q = (pix.to(F32) * torch.tensor(1.0 / ohw, dtype=F32)).to(torch.int64)
    off = pix[(q * ohw > pix) | (pix - q * ohw >= ohw)]
    fixed = off[:: max(1, off.numel() // 6)][:6].tolist() + [0, npix - 1, npix // 2, 31, 32, 33, npix - 32, npix - 33, 62, 63, 64, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 65535, 65536, 65537, 999999, 1000000,
             1048575 - 63, 1048576 + 63]
    fixed = list(dict.fromkeys(p for p in fixed if 0 <= p < npix))[:nch]
    rest = torch.randint(0, npix, (nch - len(fixed),), generator=g).tolist()
    return torch.tensor(fixed + rest)


# ================================================================================================================ references
def conv_fwd_ref(x, w, s, pad, dtype=F64, mut=None):
    """y[n][oy][ox][co] = sum x[n][oy*s - pad + kh][ox*s - pad + kw][ci] * w[co][kh][kw][ci] (include/ldetr_hip.h:707) as a tap loop over shifted
    slices -> (y, sum of |terms|).  mut: a deliberately wrong variant (the CPU file's sensitivity checks)."""
    x, w = x.to(dtype), w.to(dtype)
    N, H, W, Ci = x.shape
    Co, KH, KW, _ = w.shape
    OH, OW = out_hw(H, W, KH, KW, s, pad)
    P = max(KH, KW) + 1       # zero border wide enough for every variant
    xp = torch.zeros(N, H + 2 * P + s * 2, W + 2 * P + s * 2, Ci, dtype=dtype)
    xp[:, P:P + H, P:P + W] = x
    y = torch.zeros(N, OH, OW, Co, dtype=dtype)
    S = torch.zeros(N, OH, OW, Co, dtype=dtype)
    pd = pad - 1 if mut == 'pad_minus_1' else pad
    for kh in range(KH):
        for kw in range(KW):
            y0, x0 = (P - pd + kw, P - pd + kh) if mut == 'swap_khkw' else (P - pd + kh, P - pd + kw)
            xs = xp[:, y0:y0 + (OH - 1) * s + 1:s, x0:x0 + (OW - 1) * s + 1:s]
            t = xs @ w[:, kh, kw].t()
            if mut == 'drop_tap_at_border' and kh == KH - 1 and kw == 0:        # (a tap that is inside the image at the right border)
                t = t.clone()
                t[:, :, OW - 1] = 0
            y += t
            S += xs.abs() @ w[:, kh, kw].abs().t()
    return y, S


def conv_dgrad_ref(dy, w, s, pad, IH, IW, dtype=F64, mut=None):
    """dx[n][iy][ix][ci] = sum dy[n][(iy + pad - kh) / s][(ix + pad - kw) / s][co] * w[co][kh][kw][ci] over the taps that divide (csrc/p3_engine.hip:1525),
    parity class by parity class -> (dx, sum of |terms|)."""
    dy, w = dy.to(dtype), w.to(dtype)
    N, OH, OW, Co = dy.shape
    _, KH, KW, Ci = w.shape
    dx = torch.zeros(N, IH, IW, Ci, dtype=dtype)
    S = torch.zeros(N, IH, IW, Ci, dtype=dtype)
    for py in range(s):
        for px in range(s):
            qy, qx = (px, py) if mut == 'swap_parity' else (py, px)
            iy, ix = torch.arange(py, IH, s), torch.arange(px, IW, s)
            for kh in range(KH):
                if (qy + pad - kh) % s:
                    continue
                for kw in range(KW):
                    if (qx + pad - kw) % s:
                        continue
                    oy, ox = torch.div(iy + pad - kh, s, rounding_mode='floor'), torch.div(ix + pad - kw, s, rounding_mode='floor')
                    vy, vx = (oy >= 0) & (oy < OH), (ox >= 0) & (ox < OW)
                    if not (vy.any() and vx.any()):
                        continue
                    src = dy[:, oy[vy]][:, :, ox[vx]]
                    t = src @ w[:, kh, kw]
                    ta = src.abs() @ w[:, kh, kw].abs()
                    rows, cols = iy[vy][:, None], ix[vx][None, :]
                    dx[:, rows, cols] += t
                    S[:, rows, cols] += ta
    if mut == 'unused_row_copies_neighbour':
        OHf, OWf = out_hw(IH, IW, KH, KW, s, pad)
        last = (OHf - 1) * s - pad + KH          # first input row no output reads
        assert last < IH
        dx[:, last:] = dx[:, last - 1:last]
    return dx, S


def conv_wgrad_ref(x, dy, KH, KW, s, pad, dtype=F64, mut=None):
    """dW[co][kh][kw][ci] = sum_pix dY[pix][co] * X[src(pix, kh, kw)][ci] (csrc/p3_engine.hip:771) -> (dW, sum of |terms|)"""
    N, H, W, Ci = x.shape
    _, OH, OW, Co = dy.shape
    d2 = dy.reshape(-1, Co)
    if mut == 'last_pixel_tile_missing':
        d2 = d2.clone()
        d2[(d2.shape[0] - 1) // 32 * 32:] = 0
    pix = (d2 != 0).any(1).nonzero()[:, 0]          # pixels whose dY row is zero add nothing (the select inputs: a handful of a million)
    d2 = d2[pix].to(dtype)
    n, rem = torch.div(pix, OH * OW, rounding_mode='floor'), pix % (OH * OW)
    oy, ox = torch.div(rem, OW, rounding_mode='floor'), rem % OW
    dw = torch.zeros(Co, KH, KW, Ci, dtype=dtype)
    S = torch.zeros(Co, KH, KW, Ci, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            sy, sx = oy * s - pad + kh, ox * s - pad + kw
            v = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
            xs = x[n[v], sy[v], sx[v]].to(dtype)
            dw[:, kh, kw] = d2[v].t() @ xs
            S[:, kh, kw] = d2[v].double().abs().t() @ xs.double().abs()
    return dw, S


def apply_epilogue(acc, S, t, e, dtype=F64, mut=None):
    """include/ldetr_hip.h:696: v = acc * alpha * col_scale[n] + col_bias[n] + residual[m][n]; relu; v = relu_mask[m][n] > 0 ? v : 0, in the kernel's order of
    operations (which matters for the float32 yardstick only) -> (v, pre-activation, sum of |terms| with the epilogue's)."""
    alpha = torch.tensor(t.get('alpha', 1.0), dtype=dtype)
    if mut == 'alpha_omitted':
        alpha = torch.tensor(1.0, dtype=dtype)
    cs = alpha * (t['scale'].to(dtype) if e['scale'] else torch.ones((), dtype=dtype))
    if mut == 'scale_8_channels_off' and e['scale']:
        cs = alpha * t['scale'].to(dtype).roll(8)
    v = acc.to(dtype) * cs
    Sv = S.to(F64) * cs.to(F64).abs()
    if mut == 'relu_before_residual' and e['relu']:
        v = torch.where(v < 0, torch.zeros_like(v), v)
    for k in ('bias', 'res_p3', 'res_f32'):
        if e[k]:
            v = v + t[k].to(dtype)
            Sv = Sv + t[k].to(F64).abs()
    pre = v
    if e['relu'] and mut != 'relu_before_residual':
        v = torch.where(v < 0, torch.zeros_like(v), v)
    if e['mask']:
        keep = (v > 0) if mut == 'mask_from_y' else (t['mask'] > 0)
        v = torch.where(keep, v, torch.zeros_like(v))
    return v, pre, Sv


def bf16_planes(v):
    """The three-way split of a (moderate) fp32 tensor as float64 planes: hi = bf16(v), mid = bf16(v - hi), lo = the rest."""
    v = v.to(F32)
    hi = v.bfloat16().to(F32)
    over = torch.isinf(hi) & torch.isfinite(v)          # next to FLT_MAX the leading part is truncated (ldetr_common.hpp: split2_bf16_exact)
    hi = torch.where(over, (v.view(torch.int32) & -65536).view(F32), hi)
    mid = (v - hi).bfloat16().to(F32)
    lo = v - hi - mid
    assert torch.equal(lo.bfloat16().to(F32), lo), 'more than three planes'
    return hi.double(), mid.double(), lo.double()


def case_outputs(c, t, dtype=F64, mut=None, which=0):
    """The outputs of a case from inputs `t` in `dtype` -> dict family -> (value, pre-activation or None, sum of |terms|).  Families: y | dx | dw."""
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    e = c['epi2'] if (which == 1 and c['epi2'] is not None) else c['epi']
    out = {}
    conv_m = mut if mut in ('swap_khkw', 'pad_minus_1', 'drop_tap_at_border') else None
    epi_m = mut if mut in ('alpha_omitted', 'scale_8_channels_off', 'relu_before_residual', 'mask_from_y') else None
    if c['entry'] in ('fwd', 'dual'):
        acc, S = conv_fwd_ref(t['x'], t['w'], s, pad, dtype, conv_m)
        if mut in ('no_mid_mid', 'no_hi_lo'):
            xh, xm, xl = bf16_planes(t['x'])
            wh, wm, wl = bf16_planes(t['w'])
            acc = acc - (conv_fwd_ref(xm, wm, s, pad)[0] if mut == 'no_mid_mid' else conv_fwd_ref(xh, wl, s, pad)[0]).to(dtype)
        out['y'] = apply_epilogue(acc, S, t, e, dtype, epi_m)
    if c['entry'] in ('dgrad', 'pair'):
        w = t['w'].to(dtype)
        if c['row_scale']:
            w = (t['w'].to(dtype) * t['row_scale'].to(dtype)[:, None, None, None])       # FrozenBN's factor rides on the weight image (ldetr_p3_weight_bwd)
            if dtype == F64:
                w = w.to(F32).to(F64)                                                 # the image holds float32(w * scale): an INPUT of the contraction
        acc, S = conv_dgrad_ref(t['dy'], w, s, pad, H, W, dtype, mut if mut in ('swap_parity', 'unused_row_copies_neighbour') else None)
        out['dx'] = apply_epilogue(acc, S, t, e, dtype, epi_m)
    if c['entry'] in ('wgrad', 'pair'):
        dw, S = conv_wgrad_ref(t['x'], t['dy'], KH, KW, s, pad, dtype, mut if mut == 'last_pixel_tile_missing' else None)
        if c['row_scale']:
            dw = dw * t['row_scale'].to(dtype)[:, None, None, None]
            S = S * t['row_scale'].to(F64).abs()[:, None, None, None]
        if c['accumulate']:
            dw = dw + t['dw0'].to(dtype)
            S = S + t['dw0'].to(F64).abs()
        out['dw'] = (dw, None, S)
    return out


def case_outputs_f32(c, t, which=0):
    """The float32 yardstick: F.conv2d in fp32 and its autograd on the host, then the epilogue in fp32."""
    N, H, W, Ci, Co, KH, KW, s, pad = c['geom']
    e = c['epi2'] if (which == 1 and c['epi2'] is not None) else c['epi']
    ref = case_outputs(c, t, F64, which=which)
    out = {}
    nchw = lambda v: v.permute(0, 3, 1, 2)
    if c['entry'] in ('fwd', 'dual'):
        acc = F.conv2d(nchw(t['x']), nchw(t['w']), stride=s, padding=pad).permute(0, 2, 3, 1)
        out['y'] = apply_epilogue(acc, ref['y'][2], t, e, F32)[0]
    else:
        xd = nchw(t['x'] if 'x' in t else torch.zeros(N, H, W, Ci)).clone().requires_grad_(True)
        w = t['w'] if 'w' in t else torch.zeros(Co, KH, KW, Ci)
        wd = nchw(w).clone().requires_grad_(True)
        wsd = wd * t['row_scale'][:, None, None, None] if c['row_scale'] else wd
        gx, = torch.autograd.grad(F.conv2d(xd, wsd.detach(), stride=s, padding=pad), xd, nchw(t['dy']))
        gw, = torch.autograd.grad(F.conv2d(xd.detach(), wd, stride=s, padding=pad), wd, nchw(t['dy']))
        if c['entry'] in ('dgrad', 'pair'):
            out['dx'] = apply_epilogue(gx.permute(0, 2, 3, 1), ref['dx'][2], t, e, F32)[0]
        if c['entry'] in ('wgrad', 'pair'):
            dw = gw.permute(0, 2, 3, 1)
            if c['row_scale']:
                dw = dw * t['row_scale'][:, None, None, None]
            if c['accumulate']:
                dw = dw + t['dw0']
            out['dw'] = dw
    return out


@functools.lru_cache(maxsize=None)
def inputs(name, cls, which=0):
    return make_inputs(BY_NAME[name], cls, which)


@functools.lru_cache(maxsize=None)
def reference(name, cls, which=0):
    """float64 outputs of a table case; computed once, shared, never modified."""
    return case_outputs(BY_NAME[name], inputs(name, cls, which), F64, which=which)


# ================================================================================================================ measures and bounds
CANCELLED = 1.0 / 32


def rel_err(got, ref, S):
    """max |got - ref| / max |ref|; a block whose reference lost five or more bits to cancellation is measured against its sum of |terms|."""
    got, ref = got.detach().double().cpu(), ref.double()
    d = ref.abs().max()
    if d < CANCELLED * S.max():
        d = S.max()
    return ((got - ref).abs().max() / d.clamp_min(1e-300)).item()


def elem_rel_err(got, ref, S):
    """max over elements of |got - ref| / (that element's sum of |terms|, epilogue terms included); an element without terms must be exactly 0."""
    got, ref = got.detach().double().cpu(), ref.double()
    zero = S == 0
    if not bool((got[zero] == 0).all()):
        return float('inf')
    if bool(zero.all()):
        return 0.0
    return ((got - ref).abs()[~zero] / S[~zero]).max().item()


def bit_equal(got, ref64):
    """got (fp32) == float32(ref64) element for element; NaNs by position, -0 == +0.  -> number of elements that differ."""
    got, ref = got.detach().cpu().to(F32), ref64.to(F32)
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    return int((~same).sum())


def near_zero_share(pre, S, bound):
    """Share of elements whose pre-activation lies within the bound of zero (there a ReLU may cut on one side and not on the other; ReLU being
    1-Lipschitz, the element's error is still at most the pre-activation's, so it is compared like every other element, and counted)."""
    if pre is None:
        return 0.0
    return float(((pre.abs() <= bound * S) & (S > 0)).double().mean())


# Bounds the project already has, in rel_err's measure (tests/test_p3_gpu.py: 2e-6 forward, 3e-6 gradients)
PROJECT_BOUND = dict(y=2e-6, dx=3e-6, dw=3e-6)
FP32_FACTOR = 4.0
# float32 on the host (F.conv2d, its autograd, the epilogue in fp32) against the float64 reference: worst rounding-class case of the tables per output
# family and reduction-length bucket (K <= 256, <= 1024, <= 4608; dw: K = pixels), in rel_err's and in elem_rel_err's measure.
# measure_fp32_baselines() re-measures them; the GPU file allows FP32_FACTOR x these.
FP32_BASELINE = {'y/256': 3.32e-07, 'y/1024': 1.91e-06, 'y/4608': 2.56e-06, 'y_elem/256': 3.09e-07, 'y_elem/1024': 3.98e-07, 'y_elem/4608': 3.32e-07,
                 'dx/256': 6.77e-07, 'dx/1024': 1.14e-06, 'dx/4608': 1.43e-06, 'dx_elem/256': 2.56e-07, 'dx_elem/1024': 2.93e-07, 'dx_elem/4608': 3.41e-07,
                 'dw/256': 4.21e-07, 'dw/1024': 2.28e-07, 'dw/4608': 2.76e-07, 'dw_elem/256': 3.68e-07, 'dw_elem/1024': 1.21e-07, 'dw_elem/4608': 6.09e-08}
# Buckets whose FP32_FACTOR x yardstick lies ABOVE the project's ceiling in rel_err's measure (the host's fp32 convolution sums a long mixed-sign reduction
# in one chain; its error is a few 1e-7 of the sum of |terms|, which is several times max |y|): there the ceiling is the bound, the tighter of the two.
YARDSTICK_ABOVE_CEILING = ['y/1024', 'y/4608', 'dx/1024', 'dx/4608']


def bound(family, K, elem=False):
    b = FP32_FACTOR * FP32_BASELINE['%s%s/%d' % (family, '_elem' if elem else '', k_bucket(K))]
    return b if elem else min(b, PROJECT_BOUND[family])


def rounding_cases():
    return [c for c in VALUE_CASES if 'rounding' in c['classes']]


def measure_fp32_baselines():
    out = {}
    for c in rounding_cases():
        for which in ((0, 1) if c['entry'] == 'dual' else (0,)):
            t = inputs(c['name'], 'rounding', which)
            ref = reference(c['name'], 'rounding', which)
            y32 = case_outputs_f32(c, t, which)
            K = reduction_length(c)
            for fam, v in y32.items():
                kb = k_bucket(K[fam])
                for key, f in (('%s/%d' % (fam, kb), rel_err), ('%s_elem/%d' % (fam, kb), elem_rel_err)):
                    out[key] = max(out.get(key, 0.0), f(v, ref[fam][0], ref[fam][2]))
    return out
