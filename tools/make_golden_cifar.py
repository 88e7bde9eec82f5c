"""Golden fixtures for the CIFAR ResNets (tests/test_resnet_cifar.py) from the unmodified reference `resnet(dataset=...)`
and its Trainer on CPU, with the recipe of oracle/make_golden.py (imported as a module: the reference and its shim on
sys.path, the seeded batches, tensor_sums, the warm BatchNorm state and the gradient sampling are that file's).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_cifar.py

Writes under tests/golden/ (data only):
  structure_cifar.json   keys / shapes / parameter counts / regime of cifar10 depth 8, 20, 44 and cifar100 depth 20, the
                         initial tensor sums of the seeded depth-8 and depth-20 builds, the wide-resnet regime
  traj_c8                cifar10 depth 8, B = 8, 32 x 32, 3 steps
  traj_c20               cifar100 depth 20, B = 8, 3 steps (the 100-way ragged head)
  traj_c8_wide_drop      depth 8, width [32, 64, 128], dropout 0.3, regime 'wide-resnet' (the Dropout masks come from torch's
                         seeded CPU generator, drawn behind the model's construction)
  traj_c20_warm          cifar10 depth 20 in float64, every BatchNorm seeded non-trivial (make_golden.warm_bn_state), the
                         step-0 gradient of every parameter recorded (norm + sampled values)
Each trajectory records per-step loss / prec1 / prec5 / grad, init and final tensor sums, a few final tensors, `validate`
and the input sums.  No recorded prec value may hang on a near-tie: the smallest gap between neighbours among the six
largest logits, over every training and validation sample, must exceed 1e-4 - otherwise the next seed is taken."""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as mg  # noqa: E402  (puts the reference and its shim on sys.path)
import torch  # noqa: E402

KEEP = ['conv1.weight', 'bn1.running_mean', 'bn1.running_var', 'layer1.0.conv1.weight', 'layer2.0.downsample.0.weight',
        'layer3.0.bn2.weight', 'fc.weight', 'fc.bias']
MIN_GAP = 1e-4


def float_sums(sd):
    return mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point})


def top_gap(logits):
    top = logits.detach().double().sort(dim=1, descending=True).values[:, :6]
    return float((top[:, :-1] - top[:, 1:]).min())


def structure():
    out = {}
    for name, kw in [('cifar10_d8', dict(dataset='cifar10', depth=8)), ('cifar10_d20', dict(dataset='cifar10', depth=20)),
                     ('cifar10_d44', dict(dataset='cifar10')), ('cifar100_d20', dict(dataset='cifar100', depth=20))]:
        torch.manual_seed(123)
        m = mg.ref_models.resnet(**kw)
        sd = m.state_dict()
        out[name] = {'model_kw': kw, 'params': sum(p.numel() for p in m.parameters()), 'keys': list(sd.keys()),
                     'shapes': [list(v.shape) for v in sd.values()],
                     'regime': [{k: v for k, v in r.items() if k != 'regularizer'} for r in m.regime],
                     'weight_decay': m.regime[0]['regularizer']['value']}
        if kw.get('depth') in (8, 20):
            out[name]['init_sums'] = float_sums(sd)
    m = mg.ref_models.resnet(dataset='cifar10', depth=8, regime='wide-resnet')
    out['wide_regime'] = {'regime': [{k: v for k, v in r.items() if k != 'regularizer'} for r in m.regime],
                          'weight_decay': m.regime[0]['regularizer']['value']}
    with open(os.path.join(mg.OUT, 'structure_cifar.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('structure_cifar.json', {k: v.get('params') for k, v in out.items()})


def run(tag, dataset, model_kw, B, classes, steps, seed, dtype=torch.float, warm=False):
    """One attempt with `seed`; returns None when a recorded prec value hangs on a logit gap below MIN_GAP."""
    import copy
    torch.manual_seed(123)
    model = mg.ref_models.resnet(dataset=dataset, **model_kw)
    names = [k for k, _ in model.named_parameters()]
    ac_grads = None
    data = mg.batches(steps, B, 32, classes, seed)
    if warm:
        mg.warm_bn_state(model)
        mb = copy.deepcopy(model).float()       # PyTorch's own bf16 (autocast) on the same start state, batch 0: the yardstick
        mb.train()
        with torch.autocast('cpu', dtype=torch.bfloat16):
            out_b = mb(data[0][0])
        torch.nn.functional.cross_entropy(out_b.float(), data[0][1]).backward()
        ac_grads = {k: p.grad.detach().clone() for k, p in mb.named_parameters()}
        model.to(dtype)
    init_sums = float_sums(model.state_dict())
    opt = mg.OptimRegime(model, model.regime)
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=dtype, distributed=False,
                       loss_scale=1.0, grad_clip=1e9, print_freq=10 ** 9)
    gaps, raw, handles = [], {}, []
    hook = model.fc.register_forward_hook(lambda mod, inp, out: gaps.append(top_gap(out)))
    if warm:
        params = dict(model.named_parameters())
        for k in names:   # raw autograd gradients (the regulariser adds wd * p to p.grad in place before the step)
            handles.append(params[k].register_hook(lambda g, k=k: raw.__setitem__(k, g.detach().clone())))
    recs, grads0, autocast_err = [], None, None
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if warm and i == 0:
            grads0 = {k: mg.sample_tensor(raw[k], k) for k in names}
            autocast_err = {k: [mg.rel_l2(ac_grads[k], raw[k]), float(ac_grads[k].double().norm())] for k in names}
            for h in handles:
                h.remove()
    val = tr.validate(data[:2])
    hook.remove()
    if min(gaps) <= MIN_GAP:
        print(tag, 'seed', seed, 'rejected: logit gap', min(gaps))
        return None
    sd = model.state_dict()
    out = {'tag': tag, 'dataset': dataset, 'model_kw': model_kw, 'B': B, 'size': 32, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0, 'records': recs,
           'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')}, 'min_logit_gap': min(gaps),
           'reference_dtype': str(dtype).replace('torch.', ''),
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in data],
           'init_sums': init_sums, 'final_sums': float_sums(sd),
           'num_batches_tracked': int(sd['bn1.num_batches_tracked'])}
    if warm:
        out.update({'warm_seed': mg.WARM_SEED, 'warm_last_gamma': list(mg.WARM_LAST_GAMMA),
                    'grad0_norms': {k: v['norm'] for k, v in grads0.items()}, 'autocast_err': autocast_err})
        final = {k: mg.sample_tensor(sd[k], k) for k in names}
        torch.save({'grad0': grads0, 'final': final}, os.path.join(mg.OUT, 'traj_%s_tensors.pt' % tag))
    else:
        torch.save({k: sd[k].float().clone() for k in KEEP}, os.path.join(mg.OUT, 'traj_%s_final.pt' % tag))
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(tag, 'seed', seed, recs, 'val', out['validate'], 'gap', min(gaps))
    return out


def trajectory(tag, dataset, model_kw, B, classes, steps, seed, **kw):
    for s in range(seed, seed + 20):
        if run(tag, dataset, model_kw, B, classes, steps, s, **kw) is not None:
            return
    raise SystemExit('%s: no seed without a near-tie' % tag)


if __name__ == '__main__':
    structure()
    trajectory('c8', 'cifar10', dict(depth=8), B=8, classes=10, steps=3, seed=71)
    trajectory('c20', 'cifar100', dict(depth=20), B=8, classes=100, steps=3, seed=72)
    trajectory('c8_wide_drop', 'cifar10', dict(depth=8, width=[32, 64, 128], dropout=0.3, regime='wide-resnet'), B=8,
               classes=10, steps=3, seed=73)
    trajectory('c20_warm', 'cifar10', dict(depth=20), B=8, classes=10, steps=3, seed=74, dtype=torch.double, warm=True)
    mg.assert_no_new_bytecode()
