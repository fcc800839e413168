"""The StyleGAN2 synthesis network as one autograd node (hip/sg2_chain.py) against the per-layer path (LDETR_DEBUG="SG2_CHAIN=0") and the
oracle's float64 evaluation; the up layer's demodulation gradient from the saved output instead of a pass over the saved `ud`."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops_ref, stylegan2_ref  # noqa: E402

B, RES = 3, 32
CFG = dict(z_dim=32, w_dim=32, img_resolution=RES, img_channels=3, use_noise=False, channel_base=1024, channel_max=64,
           num_fp16_res=0, conv_clamp=None, fused_modconv_default=False)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def assert_close(a, b, tol, what=''):
    e = rel_err(a, b)
    assert e <= tol, f'{what}: rel err {e:.3e} > {tol:.1e}'


def _model(dev):
    from layoutdetr_amd.training.networks_stylegan2 import Decoder
    torch.manual_seed(11)
    m = Decoder(**CFG).train()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') and 'affine' not in n and 'mapping' not in n:
                p.normal_(0, 0.1)          # (the layers' biases start at zero: give the bias term of the demodulation sum something to do)
    return m.to(dev)


def _run(m, z, g, chain):
    """-> (img, d_z, {name: grad}) of one forward + backward on the chosen path."""
    from layoutdetr_amd.hip import sg2_chain
    old = sg2_chain.ENABLED
    sg2_chain.ENABLED = chain
    try:
        runs = sg2_chain.NODE_RUNS[0]
        m.zero_grad(set_to_none=True)
        zz = z.clone().requires_grad_(True)
        img = m(zz)
        assert (sg2_chain.NODE_RUNS[0] - runs) == (1 if chain else 0), 'the path under test did not run'
        (img * g).sum().backward()
        return img.detach().clone(), zz.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}
    finally:
        sg2_chain.ENABLED = old


@pytest.fixture(scope='module')
def case(dev):
    """Model, inputs, both paths' results and the float64 oracle, computed once and left unchanged."""
    m = _model(dev)
    gen = torch.Generator().manual_seed(12)
    z = torch.randn(B, 32, generator=gen); g = torch.randn(B, 3, RES, RES, generator=gen)
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    z64 = z.double().requires_grad_(True)
    img64 = stylegan2_ref.decoder(sd, '', z64, RES)
    (img64 * g.double()).sum().backward()
    ref = (img64.detach(), z64.grad, {k: v.grad for k, v in sd.items()})
    zd, gd = z.to(dev), g.to(dev)
    return dict(m=m, z=zd, g=gd, ref=ref, node=_run(m, zd, gd, True), layers=_run(m, zd, gd, False))


def test_node_matches_per_layer_path(case):
    """Both paths read the same saved outputs for the lrelu mask and run the same contraction launches: only summation order differs."""
    (img_a, dz_a, gr_a), (img_b, dz_b, gr_b) = case['node'], case['layers']
    assert torch.equal(img_a, img_b), 'the node\'s forward issues the per-layer launches: bit-equal image'
    assert_close(dz_a, dz_b, 2e-5, 'd_z')
    assert set(gr_a) == set(gr_b)
    for k in gr_b:
        assert_close(gr_a[k], gr_b[k], 2e-5, 'grad ' + k)


@pytest.mark.parametrize('path', ['node', 'layers'])
def test_each_path_matches_float64_oracle(case, path):
    """Bounds of test_stylegan2_decoder_matches_reference_golden."""
    img, dz, gr = case[path]
    img64, dz64, gr64 = case['ref']
    assert_close(img, img64, 2e-5, 'img')
    assert_close(dz, dz64, 2e-4, 'd_z')
    n = 0
    for k, v in gr.items():
        assert_close(v, gr64[k], 5e-4, 'grad ' + k); n += 1
    assert n > 40


def test_no_grad_output_is_bit_equal_and_nothing_is_kept(case):
    m, z = case['m'], case['z']
    from layoutdetr_amd.hip import sg2_chain
    runs = sg2_chain.NODE_RUNS[0]
    with torch.no_grad():
        img = m(z)
    assert sg2_chain.NODE_RUNS[0] == runs + 1
    assert img.grad_fn is None and not img.requires_grad
    assert torch.equal(img, case['node'][0])


def test_ud_is_not_saved(case):
    """The transposed convolutions' outputs ([B, 2r+1, 2r+1, C]) are not among the node's saved tensors; the layers' outputs are."""
    m, z = case['m'], case['z']
    img = m(z.clone().requires_grad_(True))
    fn = img.grad_fn
    while fn is not None and '_SynthesisFn' not in type(fn).__name__:
        fn = fn.next_functions[0][0]
    assert fn is not None, 'no synthesis node in the graph'
    shapes = [tuple(t.shape) for t in fn.saved_tensors if t.ndim == 4]
    assert not [s for s in shapes if s[0] == B and s[1] == s[2] and s[1] % 2 == 1], f'an odd-sized [B, 2r+1, 2r+1, C] tensor is saved: {shapes}'
    for r in (4, 8, 16, 32):
        assert any(s[1] == r and s[2] == r for s in shapes), f'the {r}x{r} outputs must be saved'


def test_node_in_captured_graph_replays_its_eager_run(case, dev):
    """Forward + backward of the node captured once and replayed.  The image is bit-equal; the gradients are held to the bound between the two
    paths (2e-5) because the weight gradients and the row sums add with fp32 atomics, whose order no two runs share."""
    m, z, g = case['m'], case['z'], case['g']
    params = list(m.parameters())
    zs = z.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):          # allocations and one-time setup outside the capture
            torch.autograd.grad((m(zs) * g).sum(), [zs] + params)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        img = m(zs)
        grads = torch.autograd.grad((img * g).sum(), [zs] + params)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    img_e, dz_e, gr_e = case['node']
    assert torch.equal(img, img_e)
    assert_close(grads[0], dz_e, 2e-5, 'd_z')
    for (k, _), v in zip(m.named_parameters(), grads[1:]):
        assert_close(v, gr_e[k], 2e-5, 'grad ' + k)


@pytest.mark.parametrize('Bn,R,Ci,Co', [(2, 8, 128, 64), (3, 4, 32, 32)])
def test_up_layer_demod_gradient_from_saved_output(dev, Bn, R, Ci, Co):
    """_ModConvUpFn's gradient for the demodulation coefficients: <dud, ud> / d = <dv, pre(y) - bias> / d, formed by the lrelu backward from the
    saved output -- against float64 autograd with the coefficients as an independent input."""
    from layoutdetr_amd.hip.modconv import _ModConvUpFn
    torch.manual_seed(300 + R)
    x = torch.randn(Bn, Ci, R, R); w = torch.randn(Co, Ci, 3, 3) / math.sqrt(Ci * 9); s = torch.randn(Bn, Ci) * 0.5 + 1.0
    b = torch.randn(Co) * 0.1; d = torch.rand(Bn, Co) + 0.5
    f = ops_ref.setup_filter([1, 3, 3, 1])
    xr, wr, sr, br, dr = [t.double().requires_grad_(True) for t in (x, w, s, b, d)]
    y = ops_ref.modulated_conv2d(xr, wr, sr, up=2, padding=1, resample_filter=f.double(), demodulate=False, flip_weight=False)
    y = ops_ref.bias_act(y * dr[:, :, None, None], br, act='lrelu', gain=math.sqrt(2))
    g = torch.randn(y.shape, dtype=torch.float64)
    y.backward(g)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    wd = w.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sd, bd, dd = [t.to(dev).requires_grad_(True) for t in (s, b, d)]
    out = _ModConvUpFn.apply(xd, wd, sd, dd, bd, f.to(dev), 0.2, math.sqrt(2))
    assert not [t for t in out.grad_fn.saved_tensors if t.ndim == 4 and t.shape[1] == 2 * R + 1], 'ud is still saved'
    out.backward(g.float().permute(0, 2, 3, 1).contiguous().to(dev))
    assert_close(out.permute(0, 3, 1, 2), y.detach(), 2e-5, 'y')
    assert_close(dd.grad, dr.grad, 1e-4, 'ddemod')
    assert_close(xd.grad.permute(0, 3, 1, 2), xr.grad, 5e-5, 'dx')
    assert_close(wd.grad, wr.grad, 5e-5, 'dw')
    assert_close(sd.grad, sr.grad, 1e-4, 'dstyles')
    assert_close(bd.grad, br.grad, 5e-5, 'dbias')
