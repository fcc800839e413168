"""The synthesis node with the side chain inside (hip/sg2_chain.py: grouped styles, grouped demodulation coefficients, their backward and the
affines' backward) against the same node with the side chain as autograd nodes in front of it (LDETR_DEBUG="SG2_SIDE=0") and the oracle's
float64 evaluation.  The model of tests/test_sg2_chain_gpu.py: B = 3, 32 x 32, channel_max 64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import stylegan2_ref  # noqa: E402

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
                p.normal_(0, 0.1)
    return m.to(dev)


class _Side(object):
    """sg2_chain.SIDE set for a block, and the number of grouped style launches issued inside it."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from layoutdetr_amd.hip import sg2_chain
        self.old, self.old_fn, self.calls = sg2_chain.SIDE, sg2_chain.side_styles, 0

        def counted(*a, **k):
            self.calls += 1
            return self.old_fn(*a, **k)
        sg2_chain.SIDE, sg2_chain.side_styles = self.on, counted
        return self

    def __exit__(self, *exc):
        from layoutdetr_amd.hip import sg2_chain
        sg2_chain.SIDE, sg2_chain.side_styles = self.old, self.old_fn


def _run(m, z, g, side):
    """-> (img, d_z, {name: grad}) of one forward + backward with the side chain inside the node or in front of it."""
    from layoutdetr_amd.hip import sg2_chain
    with _Side(side) as sw:
        runs = sg2_chain.NODE_RUNS[0]
        m.zero_grad(set_to_none=True)
        zz = z.clone().requires_grad_(True)
        img = m(zz)
        assert sg2_chain.NODE_RUNS[0] == runs + 1 and sw.calls == (1 if side else 0), 'the path under test did not run'
        (img * g).sum().backward()
        return img.detach().clone(), zz.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.fixture(scope='module')
def case(dev):
    """Model, inputs, both routes' results and the float64 oracle, computed once and left unchanged."""
    m = _model(dev)
    gen = torch.Generator().manual_seed(12)
    z = torch.randn(B, 32, generator=gen); g = torch.randn(B, 3, RES, RES, generator=gen)
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    z64 = z.double().requires_grad_(True)
    img64 = stylegan2_ref.decoder(sd, '', z64, RES)
    (img64 * g.double()).sum().backward()
    ref = (img64.detach(), z64.grad, {k: v.grad for k, v in sd.items()})
    zd, gd = z.to(dev), g.to(dev)
    return dict(m=m, z=zd, g=gd, ref=ref, inside=_run(m, zd, gd, True), front=_run(m, zd, gd, False))


def test_side_chain_inside_matches_side_chain_in_front(case):
    """The grouped forward launches run the single launches' bodies: bit-equal image.  The gradients differ by summation order only (the latent's
    gradient as one product over all layers, the demodulation's style share added by the kernel): test_sg2_chain_gpu's bound between two orders."""
    (img_a, dz_a, gr_a), (img_b, dz_b, gr_b) = case['inside'], case['front']
    assert torch.equal(img_a, img_b)
    assert_close(dz_a, dz_b, 2e-5, 'd_z')
    assert set(gr_a) == set(gr_b) and any('affine.weight' in k for k in gr_a) and any('mapping' in k for k in gr_a)
    for k in gr_b:
        assert_close(gr_a[k], gr_b[k], 2e-5, 'grad ' + k)


@pytest.mark.parametrize('route', ['inside', 'front'])
def test_each_route_matches_float64_oracle(case, route):
    """Bounds of test_sg2_chain_gpu.test_each_path_matches_float64_oracle."""
    img, dz, gr = case[route]
    img64, dz64, gr64 = case['ref']
    assert_close(img, img64, 2e-5, 'img')
    assert_close(dz, dz64, 2e-4, 'd_z')
    n = 0
    for k, v in gr.items():
        assert_close(v, gr64[k], 5e-4, 'grad ' + k); n += 1
    assert n > 40


def test_captured_forward_and_backward_replay_the_eager_run(case, dev):
    """Forward + backward captured once and replayed: the image bit-equal, the gradients at the bound between two runs of the atomics."""
    m, z, g = case['m'], case['z'], case['g']
    params = list(m.parameters())
    zs = z.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with _Side(True) as sw:
        with torch.cuda.stream(side):
            for _ in range(2):          # allocations and one-time setup outside the capture
                torch.autograd.grad((m(zs) * g).sum(), [zs] + params)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            img = m(zs)
            grads = torch.autograd.grad((img * g).sum(), [zs] + params)
        assert sw.calls == 3
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    img_e, dz_e, gr_e = case['inside']
    assert torch.equal(img, img_e)
    assert_close(grads[0], dz_e, 2e-5, 'd_z')
    for (k, _), v in zip(m.named_parameters(), grads[1:]):
        assert_close(v, gr_e[k], 2e-5, 'grad ' + k)


def test_per_layer_latents_take_the_route_in_front(case):
    """ws [B, num_ws, w_dim]: the affines run per layer in front of the node; same image, gradients at the bound between two orders."""
    m, z, g = case['m'], case['z'], case['g']
    with _Side(True) as sw:
        m.zero_grad(set_to_none=True)
        zz = z.clone().requires_grad_(True)
        w = m.mapping(zz, broadcast=False)
        img = m.synthesis(w.unsqueeze(1).repeat([1, m.num_ws, 1]))
        assert sw.calls == 0
        (img * g).sum().backward()
    img_e, dz_e, gr_e = case['inside']
    assert torch.equal(img, img_e)
    assert_close(zz.grad, dz_e, 2e-5, 'd_z')
    for k, p in m.named_parameters():
        assert_close(p.grad, gr_e[k], 2e-5, 'grad ' + k)


def test_no_grad_saves_nothing(case):
    m, z = case['m'], case['z']
    with _Side(True) as sw, torch.no_grad():
        img = m(z)
        assert sw.calls == 1
    assert img.grad_fn is None and not img.requires_grad
    assert torch.equal(img, case['inside'][0])
