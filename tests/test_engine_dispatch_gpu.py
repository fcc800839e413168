"""Every `return launch_*` statement of the fp32-operand engine's C entry points (host part of csrc/gemm_conv.hip), driven through the Python
wrappers at the smallest shapes that reach it.  Each case pins two things: the sequence of (entry, kernel template) the launch policy chose
(ldetr_engine_last_launch; the table below was recorded on an MI355X BEFORE the host side was restructured, so a change of the host code that
moves a shape onto another template -- or another workspace slice, fix-up vs atomics -- shows here) and the result against a float64 evaluation
at <= 2e-5, the bar of test_engine_bench_shapes_gpu.py.  The comment on each case names the statement it reaches."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from engine_launches import SWEEP_FORCED, Launches
from oracle import ops_ref

pytestmark = pytest.mark.gpu


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _operands(M, N, K, ta, tb):
    """A, B as ldetr_gemm_f32 stores them (ta: A is [K, M]; tb: B is [K, N], else [N, K]) and op(A) @ op(B) in float64."""
    A = torch.randn(K, M) if ta else torch.randn(M, K)
    B = torch.randn(K, N) if tb else torch.randn(N, K)
    ref = (A.double().t() if ta else A.double()) @ (B.double() if tb else B.double().t())
    return A, B, ref


def dense(M, N, K, ta, tb):
    def run(dev):
        from layoutdetr_amd.hip import core
        torch.manual_seed(M + N + K + 2 * ta + tb)
        A, B, ref = _operands(M, N, K, ta, tb)
        with Launches() as L:
            C = core.gemm(A.to(dev), B.to(dev), ta, tb, M, N, K)
        return L.seen, dict(c=rel(C, ref))
    return run


def dense_splitk_epilogue(registered):
    """(300, 200, 1024) with splitk = 8 and alpha / bias / residual / lrelu: in-kernel fix-up through a workspace slice, or (workspace
    unregistered) zero fill + fp32 atomics + the epilogue pass."""
    def run(dev):
        from layoutdetr_amd.hip import core
        M, N, K = 300, 200, 1024
        torch.manual_seed(41)
        A = torch.randn(M, K); W = torch.randn(N, K); b = torch.randn(N); R = torch.randn(M, N)
        ref = F.leaky_relu(0.5 * (A.double() @ W.double().t()) + b.double() + R.double(), 0.2) * math.sqrt(2)
        Ad, Wd, bd, Rd = [t.to(dev) for t in (A, W, b, R)]
        ep = core.epilogue(alpha=0.5, col_bias=bd, residual=Rd, act=core.ACT_LRELU, act_alpha=0.2, act_gain=math.sqrt(2))
        lib = core.lib()
        ws = core._workspace[torch.cuda.current_device()]
        try:
            if not registered:
                core.check(lib.ldetr_set_workspace(None, 0), 'unregister')
            with Launches() as L:
                C = core.gemm(Ad, Wd, 0, 0, M, N, K, splitk=8, ep=ep)
            torch.cuda.synchronize()
        finally:
            if not registered:
                core.check(lib.ldetr_set_workspace(ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4), 're-register')
        return L.seen, dict(c=rel(C, ref))
    return run


def dense_rowsum_accumulate(dev):
    from layoutdetr_amd.hip import core
    M, N, K = 1024, 512, 4096
    torch.manual_seed(43)
    A, B, ref = _operands(M, N, K, 1, 1)
    C0 = torch.randn(M, N)
    out = C0.to(dev); rs = torch.zeros(M, device=dev)
    with Launches() as L:
        core.gemm(A.to(dev), B.to(dev), 1, 1, M, N, K, out=out, ep=core.epilogue(accumulate=True, a_rowsum=rs))
    return L.seen, dict(c=rel(out, C0.double() + ref), rowsum=rel(rs, A.double().sum(0)))


def pair(p0, p1):
    """p = (M, N, K, ta, tb): both problems through ONE ldetr_gemm_pair_f32 call."""
    def run(dev):
        from layoutdetr_amd.hip import core
        torch.manual_seed(sum(p0[:3]) + sum(p1[:3]))
        gs, refs = [], []
        for M, N, K, ta, tb in (p0, p1):
            A, B, ref = _operands(M, N, K, ta, tb)
            gs.append(dict(A=A.to(dev), B=B.to(dev), ta=ta, tb=tb, M=M, N=N, K=K, out=torch.empty(M, N, device=dev), ep=None))
            refs.append(ref)
        with Launches() as L:
            core.gemm_pair(gs[0], gs[1])
        return L.seen, dict(c0=rel(gs[0]['out'], refs[0]), c1=rel(gs[1]['out'], refs[1]))
    return run


def conv2d(N, H, W, Ci, Co, k, s, p):
    """y = conv(x, w) * scale + shift (FrozenBN folded into the epilogue, as the trunk calls it), then dx and dw."""
    def run(dev):
        from layoutdetr_amd.hip import conv
        torch.manual_seed(6 + H + Ci)
        x = torch.randn(N, Ci, H, W); w = torch.randn(Co, Ci, k, k) / math.sqrt(Ci * k * k)
        scale = torch.rand(Co) + 0.5; shift = torch.randn(Co)
        xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True)
        yr = F.conv2d(xr, wr, stride=s, padding=p) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        g = torch.randn(yr.shape); yr.backward(g.double())
        xg = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
        wg = w.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with Launches() as L:
            y = conv.conv2d_nhwc(xg, wg, scale.to(dev), shift.to(dev), None, stride=s, pad=p)
            y.backward(g.permute(0, 2, 3, 1).contiguous().to(dev))
        return L.seen, dict(y=rel(y.permute(0, 3, 1, 2), yr), dx=rel(xg.grad.permute(0, 3, 1, 2), xr.grad), dw=rel(wg.grad, wr.grad))
    return run


def conv2d_stem(dev):
    """The smallest case of test_conv2d_stem_nchw: 7x7 / 2 on a 3-channel NCHW image with FrozenBN + ReLU (a shift of +12 keeps every
    pre-activation, sigma ~ 2, on the ReLU's linear branch: no mask to disagree about with float64)."""
    from layoutdetr_amd.hip import conv
    N, H, W = 2, 32, 32
    torch.manual_seed(7)
    x = torch.randn(N, 3, H, W); w = torch.randn(64, 3, 7, 7) * 0.1
    scale = torch.rand(64) + 0.5; shift = torch.randn(64) + 12.0
    wr = w.double().requires_grad_(True)
    yr = F.relu(F.conv2d(x.double(), wr, stride=2, padding=3) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    g = torch.randn(yr.shape); yr.backward(g.double())
    wg = w.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with Launches() as L:
        y = conv.conv2d_nhwc(x.to(dev), wg, scale.to(dev), shift.to(dev), None, stride=2, pad=3, relu=True, x_is_nchw=True)
        y.backward(g.permute(0, 2, 3, 1).contiguous().to(dev))
    return L.seen, dict(y=rel(y.permute(0, 3, 1, 2), yr), dw=rel(wg.grad, wr.grad))


def conv_transpose2d(N, H, W, Ci, Co):
    """3x3 / stride 2, the weight given un-transposed (OHWI)."""
    def run(dev):
        from layoutdetr_amd.hip import conv
        torch.manual_seed(11 + Co)
        x = torch.randn(N, Ci, H, W); w = torch.randn(Co, Ci, 3, 3) / math.sqrt(Ci * 9)
        xr = x.double().requires_grad_(True); wr = w.double().requires_grad_(True)
        yr = F.conv_transpose2d(xr, wr.permute(1, 0, 2, 3), stride=2)
        g = torch.randn(yr.shape); yr.backward(g.double())
        xg = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
        wg = w.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
        with Launches() as L:
            y = conv.conv_transpose2d_nhwc(xg, wg, stride=2, pad=0)
            y.backward(g.permute(0, 2, 3, 1).contiguous().to(dev))
        return L.seen, dict(y=rel(y.permute(0, 3, 1, 2), yr), dx=rel(xg.grad.permute(0, 3, 1, 2), xr.grad), dw=rel(wg.grad.permute(0, 3, 1, 2), wr.grad))
    return run


def modconv(B, R, Ci, Co, up):
    """One StyleGAN2 synthesis layer as test_engine_bench_shapes_gpu.py evaluates it (bias of +8 sigma: the lrelu stays on one branch)."""
    def run(dev):
        from layoutdetr_amd.hip import modconv as mc
        torch.manual_seed(300 + B + R + up)
        x = torch.randn(B, Ci, R, R); w = torch.randn(Co, Ci, 3, 3) / math.sqrt(Ci * 9); s = torch.randn(B, Ci) * 0.5 + 1.0
        b = torch.randn(Co) * 0.1 + 8.0
        f = ops_ref.setup_filter([1, 3, 3, 1])
        xr, wr, sr, br = [t.double().clone().requires_grad_(True) for t in (x, w, s, b)]
        y = ops_ref.modulated_conv2d(xr, wr, sr, up=up, padding=1, resample_filter=f.double(), demodulate=True, flip_weight=(up == 1))
        y = ops_ref.bias_act(y, br, act='lrelu', gain=math.sqrt(2))
        g = torch.randn(y.shape)
        y.backward(g.double())
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
        wd = w.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        sd = s.to(dev).requires_grad_(True); bd = b.to(dev).requires_grad_(True)
        with Launches() as L:
            out = mc.modconv3x3(xd, wd, sd, bd) if up == 1 else mc.modconv3x3_up2(xd, wd, sd, bd, f.to(dev))
            out.backward(g.permute(0, 2, 3, 1).contiguous().to(dev))
        return L.seen, dict(y=rel(out.permute(0, 3, 1, 2), y), dx=rel(xd.grad.permute(0, 3, 1, 2), xr.grad), dw=rel(wd.grad, wr.grad),
                            dstyles=rel(sd.grad, sr.grad), dbias=rel(bd.grad, br.grad))
    return run


CASES = {
    # ---- ldetr_gemm_f32
    'gemm_nt_70x36x52': dense(70, 36, 52, 0, 0),                 # launch_small<0, 0>, generic loads (K % 32 != 0)
    'gemm_nn_70x36x52': dense(70, 36, 52, 0, 1),                 # launch_small<0, 1>, generic loads
    'gemm_tn_70x36x52': dense(70, 36, 52, 1, 1),                 # launch_small<1, 1>, generic loads
    'gemm_nt_144x256x256': dense(144, 256, 256, 0, 0),           # launch_small<0, 0>, FAST
    'gemm_nt_144x256x2048': dense(144, 256, 2048, 0, 0),         # launch_small<0, 0> with small_plan_rule's in-kernel split-K (workspace slice)
    'gemm_nt_4096x256x64': dense(4096, 256, 64, 0, 0),           # launch_gemm<OP_KC_DENSE, OP_KC_DENSE>: exactly SMALL_GEMM_TILES tiles
    'gemm_nn_4096x256x64': dense(4096, 256, 64, 0, 1),           # launch_gemm<OP_KC_DENSE, OP_RC_DENSE>
    'gemm_splitk8_epilogue_workspace': dense_splitk_epilogue(True),        # launch_gemm: fix-up slice from the ring
    'gemm_splitk8_epilogue_no_workspace': dense_splitk_epilogue(False),    # launch_gemm: zero_fill + atomics + gemm_epilogue_kernel
    'gemm_tn_rowsum_accumulate_1024x512x4096': dense_rowsum_accumulate,    # ldetr_colsum_f32 pass, then launch_gemm<OP_RC_DENSE, OP_RC_DENSE>
    # ---- ldetr_gemm_pair_f32
    'pair_nn_tn_144_256_256': pair((144, 256, 256, 0, 1), (256, 256, 144, 1, 1)),       # the NN + TN single launch (dX + dW of a linear layer)
    'pair_tn_tn_144_256_2048': pair((2048, 256, 144, 1, 1), (256, 2048, 144, 1, 1)),    # the TN + TN single launch (the feed-forward block's two dW)
    'pair_fallback_two_calls': pair((144, 256, 256, 0, 1), (4096, 1024, 512, 1, 1)),    # second problem not small: two ldetr_gemm_f32 calls
    # ---- ldetr_conv2d_{fwd, bwd_data, bwd_weight}_f32
    'conv_2x16x16_64_64_k1': conv2d(2, 16, 16, 64, 64, 1, 1, 0),        # packed 1x1: launch_small<0, 0> | launch_small<0, 1> | launch_small<1, 1>
    'conv_4x32x32_64_256_k1': conv2d(4, 32, 32, 64, 256, 1, 1, 0),      # packed 1x1, 256 tiles: launch_gemm<OP_KC_DENSE, OP_KC_DENSE> forward
    'conv_1x96x96_8_8_k1': conv2d(1, 96, 96, 8, 8, 1, 1, 0),            # packed 1x1, > 8192 pixels: launch_gemm<OP_RC_DENSE, OP_RC_DENSE> weight gradient
    'conv_2x16x16_64_128_k3': conv2d(2, 16, 16, 64, 128, 3, 1, 1),      # launch_gemm<OP_KC_CONV, OP_KC_DENSE> | <OP_KC_CONVT, OP_RC_WT> | <OP_RC_DENSE, OP_RC_PIX>
    'conv_2x17x15_32_64_k3s2': conv2d(2, 17, 15, 32, 64, 3, 2, 1),      # the same three with stride 2: parity classes of the data gradient
    'conv_3x9x9_8_12_k3': conv2d(3, 9, 9, 8, 12, 3, 1, 1),              # the same three, generic loads
    'conv_1x16x16_64_64_k7': conv2d(1, 16, 16, 64, 64, 7, 1, 3),        # 49 taps: no FAST
    'conv_2x256x257_32_32_k3': conv2d(2, 256, 257, 32, 32, 3, 1, 1),    # launch_gemm's 256 x 32 tile (forward and data gradient)
    'conv_stem_2x32x32_nchw': conv2d_stem,                              # stem kernel forward; launch_gemm<OP_RC_DENSE, OP_RC_CONVK> weight gradient
    # ---- ldetr_conv_transpose2d_{fwd, bwd_data, bwd_weight}_f32
    'convT_2x8x8_64_64': conv_transpose2d(2, 8, 8, 64, 64),     # launch_gemm<OP_KC_CONVT, OP_KC_WTAP> | <OP_KC_CONV, OP_RC_WT> | <OP_RC_PIX, OP_RC_DENSE>
    'convT_2x8x8_64_32': conv_transpose2d(2, 8, 8, 64, 32),
    # ---- modulated layers: per-sample operand scales in the weight gradients
    'modconv_b2_r8': modconv(2, 8, 64, 64, 1),                  # set_sample_slices, then launch_gemm<OP_RC_DENSE, OP_RC_PIX>
    'modconv_up_b2_r8': modconv(2, 8, 64, 64, 2),               # set_sample_slices, then launch_gemm<OP_RC_PIX, OP_RC_DENSE>
    'modconv_b8_r8': modconv(8, 8, 64, 64, 1),                  # operands scaled by the caller: no scales reach the launch
    'modconv_up_b8_r8': modconv(8, 8, 64, 64, 2),
    'modconv_b2_r4': modconv(2, 4, 64, 64, 1),                  # < 64 pixels per sample: scales stay in the loaders, launch_gemm<OP_RC_PIX, OP_RC_PIX> (conv2d)
    'modconv_up_b2_r4': modconv(2, 4, 64, 64, 2),               # the same in ldetr_conv_transpose2d_bwd_weight_f32: launch_gemm<OP_RC_PIX, OP_RC_PIX>
}

# (entry, kernel template) of every engine call of a case, in order: recorded on an MI355X at the commit before the host side of gemm_conv.hip was
# restructured.  A policy change must update this table AND keep the parity green.
EXPECT = {
    'gemm_nt_70x36x52': [('gemm', 'gemm_small_kernel<4w>')],
    'gemm_nn_70x36x52': [('gemm', 'gemm_small_kernel<4w>')],
    'gemm_tn_70x36x52': [('gemm', 'gemm_small_kernel<4w>')],
    'gemm_nt_144x256x256': [('gemm', 'gemm_small_kernel<4w,FAST>')],
    'gemm_nt_144x256x2048': [('gemm', 'gemm_small_kernel<4w,FAST>')],
    'gemm_nt_4096x256x64': [('gemm', 'gemm_f32_kernel<64,64,32,4w,FAST>')],
    'gemm_nn_4096x256x64': [('gemm', 'gemm_f32_kernel<64,64,32,4w,FAST>')],
    'gemm_splitk8_epilogue_workspace': [('gemm', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=8')],
    'gemm_splitk8_epilogue_no_workspace': [('gemm', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=8')],
    'gemm_tn_rowsum_accumulate_1024x512x4096': [('gemm', 'gemm_f32_kernel<128,64,32,4w,FAST,SPLIT> splitK=8')],
    'pair_nn_tn_144_256_256': [('gemm', 'gemm_small_pair_kernel<4w>')],
    'pair_tn_tn_144_256_2048': [('gemm', 'gemm_small_pair_kernel<4w>')],
    'pair_fallback_two_calls': [('gemm', 'gemm_f32_kernel<128,64,32,4w,FAST,SPLIT>')],
    'conv_2x16x16_64_64_k1': [('conv2d_fwd', 'gemm_small_kernel<4w,FAST>'), ('conv2d_bwd_data', 'gemm_small_kernel<4w,FAST>'), ('conv2d_bwd_weight', 'gemm_small_kernel<8w,FAST>')],
    'conv_4x32x32_64_256_k1': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST>'), ('conv2d_bwd_data', 'gemm_small_kernel<4w,FAST>'), ('conv2d_bwd_weight', 'gemm_small_kernel<8w,FAST>')],
    'conv_1x96x96_8_8_k1': [('conv2d_fwd', 'gemm_small_kernel<4w>'), ('conv2d_bwd_data', 'gemm_small_kernel<4w>'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=72')],
    'conv_2x16x16_64_128_k3': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=9'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4')],
    'conv_2x17x15_32_64_k3s2': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w> splitK=2'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w>')],
    'conv_3x9x9_8_12_k3': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w>'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w>'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w>')],
    'conv_1x16x16_64_64_k7': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w> splitK=24'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w> splitK=24'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=2')],
    'conv_2x256x257_32_32_k3': [('conv2d_fwd', 'gemm_f32_kernel<256,32,32,4w,FAST,SPLIT>'), ('conv2d_bwd_data', 'gemm_f32_kernel<256,32,32,4w,FAST,SPLIT>'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w> splitK=86')],
    'conv_stem_2x32x32_nchw': [('conv2d_fwd', 'stem_conv7x7_kernel'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4')],
    'convT_2x8x8_64_64': [('conv_transpose2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>'), ('conv_transpose2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv_transpose2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>')],
    'convT_2x8x8_64_32': [('conv_transpose2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>'), ('conv_transpose2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w> splitK=2'), ('conv_transpose2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>')],
    'modconv_b2_r8': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST> splitK=2')],
    'modconv_up_b2_r8': [('conv_transpose2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>'), ('conv_transpose2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv_transpose2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST> splitK=2')],
    'modconv_b8_r8': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4')],
    'modconv_up_b8_r8': [('conv_transpose2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>'), ('conv_transpose2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv_transpose2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4')],
    'modconv_b2_r4': [('conv2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w>')],
    'modconv_up_b2_r4': [('conv_transpose2d_fwd', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT>'), ('conv_transpose2d_bwd_data', 'gemm_f32_kernel<64,64,32,4w,FAST,SPLIT> splitK=4'), ('conv_transpose2d_bwd_weight', 'gemm_f32_kernel<64,64,32,4w>')],
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_entry_points_launch_the_recorded_kernels_and_match_float64(dev, case):
    seen, errs = CASES[case](dev)
    torch.cuda.synchronize()
    print(f'  {case}: {seen}')
    print('   ', {k: f'{v:.1e}' for k, v in errs.items()})
    if not SWEEP_FORCED:       # (the development sweeps' forcing switches change the policy on purpose: values only)
        assert seen == EXPECT[case], f'{case}: launched {seen}, recorded {EXPECT[case]}'
    for k, v in errs.items():
        assert v <= 2e-5, f'{case}: {k} is {v:.2e} from float64'
