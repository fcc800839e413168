"""Generates tests/golden/layoutnet_train.npz by driving the REFERENCE (salesforce/LayoutDETR) on the CPU: data only.

Run where the reference tree is available:  python tools/gen_layoutnet_train_golden.py [path to the reference]
Weights and inputs are not stored: tests/layoutnet_train_common.py rebuilds them from names and seeds on both sides.  Stored per case (A, B, C of
layoutnet_train_common.CASES): the three outputs of the reference's LayoutNet.forward in float32 and float64 and the three terms of the detector's
loss (float64).  Stored once: a trajectory of the reference module under torch.optim.Adam on layoutnet_train_common.trajectory_batches() (eval
mode: no dropout) -- the float64 per-step losses and the float32 run's deviation from them -- and the first perturbed batch.  Printed: how far the
reference in float32 is from its float64 run on outputs, parameter gradients and per-step losses (the figures the test bounds are argued from)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (the one place that names where the reference tree lies)

REF = sys.argv[1] if len(sys.argv) > 1 else _DEFAULT_REF
OUT = os.path.join(ROOT, 'tests', 'golden', 'layoutnet_train.npz')


def _setup():
    sys.path.insert(0, REF)
    sys.path.insert(1, ROOT)
    sys.path.insert(2, os.path.join(ROOT, 'tests'))
    from oracle.gen_golden import _stub_modules
    _stub_modules()


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def main():
    _setup()
    import layout_eval_common as C
    import layoutnet_train_common as T
    from training.networks_layoutnet import LayoutNet

    def module(num_label, dtype):
        net = LayoutNet(num_label)
        net.load_state_dict(C.seeded_layoutnet_state(net))
        return net.to(dtype).eval()

    def loss_of(net, bbox, label, pad, is_real):
        disc, cls, box = net(bbox.to(next(net.parameters()).dtype), label.clone(), pad)
        return T.loss_terms(disc, cls, box, bbox, label, pad, is_real) + ((disc, cls, box),)

    d = {}
    worst_out = worst_grad = 0.0
    for tag, c in T.CASES.items():
        bbox, label, pad, is_real = T.case_inputs(tag)
        res = {}
        for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            net = module(c['num_label'], dtype)
            *terms, total, outs = loss_of(net, bbox, label, pad, is_real)
            total.backward()
            res[name] = (outs, terms, {n: p.grad.clone() for n, p in net.named_parameters()})
            for key, v in zip(('disc', 'cls', 'box'), outs):
                d[f'{tag}_{key}_{name}'] = v.detach().numpy()
        d[f'{tag}_loss_terms'] = np.array([t.item() for t in res['f64'][1]], dtype=np.float64)
        e_out = max(rel(a, b) for a, b in zip(res['f32'][0], res['f64'][0]))
        e_grad = max(rel(res['f32'][2][n], g) for n, g in res['f64'][2].items())
        worst_out, worst_grad = max(worst_out, e_out), max(worst_grad, e_grad)
        print(f'case {tag}: M = {int((~pad).sum())}, loss terms {d[f"{tag}_loss_terms"]}, fp32 vs fp64: outputs {e_out:.2e}, parameter gradients {e_grad:.2e}')
        # the restatement the tests differentiate must be the reference's function
        sd = T.to_dtype(C.seeded_layoutnet_state(LayoutNet(c['num_label'])), torch.float64)
        mine = T.forward_ref(sd, bbox.double(), label, pad)[:3]
        e = max(rel(a, b) for a, b in zip(mine, res['f64'][0]))
        assert e <= 1e-10, (tag, e)

    t = T.TRAJ
    batches = T.trajectory_batches()
    d['traj_batch0_bbox'] = batches[0][0].numpy()
    d['traj_batch0_is_real'] = batches[0][3].numpy()
    runs = {}
    for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        net = module(t['num_label'], dtype)
        opt = torch.optim.Adam(net.parameters(), lr=t['lr'], betas=t['betas'], eps=t['eps'])
        rows = []
        for bbox, label, pad, is_real in batches:
            opt.zero_grad()
            l_disc, l_cls, l_bbox, total, _ = loss_of(net, bbox, label, pad, is_real)
            total.backward()
            opt.step()
            rows.append([l_disc.item(), l_cls.item(), l_bbox.item(), total.item()])
        runs[name] = np.array(rows, dtype=np.float64)
    d['traj_losses_f64'] = runs['f64']                                   # [steps][L_disc, L_cls, L_bbox, total]
    d['traj_f32_deviation'] = np.abs(runs['f32'] - runs['f64']) / np.abs(runs['f64'])
    first, last = runs['f64'][0, 3], runs['f64'][-1, 3]
    print(f'trajectory: fp64 total loss {first:.4f} -> {last:.4f}; fp32 run deviates by at most {d["traj_f32_deviation"][:, 3].max():.2e} (total), '
          f'{d["traj_f32_deviation"].max():.2e} (any term)')
    assert last < first, 'the reference trajectory must reduce its loss'
    print(f'fp32 vs fp64 over the cases: outputs {worst_out:.2e}, parameter gradients {worst_grad:.2e}')
    np.savez_compressed(OUT, **d)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
