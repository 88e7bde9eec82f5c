"""Golden fixtures for MobileNet (tests/test_mobilenet.py) from the unmodified reference on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mobilenet.py

oracle/make_golden.py is imported unchanged.  torchvision is not installed and the oracle's torchvision.transforms shim
raises when a transform is constructed (the reference's MobileNet builds its data_regime in __init__), so the names of the
already-imported shim module are replaced FROM HERE by a recorder class before the model is built; nothing under oracle/
changes.

This architecture is badly conditioned at fixture sizes (BatchNorm over a few dozen values per channel, channels dying
behind ReLU): the reference's own fp32 run leaves its float64 run after a few steps.  So every trajectory is the FLOAT64
reference at a small learning rate (stored in the fixture), the fp32 reference is run beside it, and each json carries a
`ref_self` block - the fp32 reference's deviation from the float64 one per step, per final tensor and per step-0 gradient -
and `checked_steps`: the longest prefix on which the fp32 reference is within ONE TENTH of every bound the test applies
(loss abs 1e-4, grad-norm rel 1e-3, prec identical, final tensors rel-L2 1e-4, validate loss rel 1e-3).  The final tensors
and the validate record are those after `checked_steps` steps.  The tool fails if checked_steps < 2.

Writes under tests/golden/:
  structure_mobilenet.json      keys, shapes, parameter counts, seeded init sums and the recorded data_regime of
                                (width 1, deep), (width 0.5, deep), (width 0.25, shallow)
  traj_mbs                      width 0.25 deep, B = 16, 64 px, lr 0.01, 2 steps, validate on the first two batches
  traj_mbs_shallow (+_final.pt) width 0.25 shallow, B = 16, 32 px, lr 0.01, 3 steps, ALL floating tensors
  traj_mbs_grad0 (.json, .pt)   step-0 gradient of every parameter of the mbs model: norm + helpers.sample_tensor samples"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as mg  # noqa: E402  (puts the reference and its shim on sys.path)
import torch  # noqa: E402
import torchvision.transforms as shim_transforms  # noqa: E402  (the oracle's stub)


class Recorded(object):
    """Stands in for a torchvision transform: remembers its class name and constructor arguments."""
    name = '?'

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs

    def describe(self):
        d = lambda v: v.describe() if isinstance(v, Recorded) else [d(u) for u in v] if isinstance(v, (list, tuple)) else v  # noqa: E731
        return {'name': self.name, 'args': d(self.args), 'kwargs': {k: d(v) for k, v in self.kwargs.items()}}


for _n in ('Compose', 'Normalize', 'ToTensor', 'Resize', 'CenterCrop', 'RandomCrop', 'RandomHorizontalFlip',
           'RandomResizedCrop', 'ColorJitter', 'Lambda', 'Pad'):
    setattr(shim_transforms, _n, type(_n, (Recorded,), {'name': _n}))

CLASSES = 16
MBS = dict(width=0.25, num_classes=CLASSES)
MBS_SHALLOW = dict(width=0.25, shallow=True, num_classes=CLASSES)
# the test's fp32 bounds; the fp32 reference must be within a tenth of each on the checked steps
BOUNDS = {'loss_abs': 1e-4, 'grad_rel': 1e-3, 'final_rel_l2': 1e-4, 'validate_loss_rel': 1e-3}
GRAD0_FLOOR, GRAD0_FACTOR, GRAD0_MAX_SELF = 2.5e-4, 4.0, 1e-2


def build(kw):
    torch.manual_seed(123)
    return mg.ref_models.mobilenet(**kw)


def describe_regime(regime):
    out = []
    for r in regime:
        out.append({k: (v.describe() if isinstance(v, Recorded) else v) for k, v in r.items() if k != 'regularizer'})
    return out


def structure():
    out = {}
    for tag, kw in (('w1.0', dict()), ('w0.5', dict(width=0.5)), ('w0.25_shallow', dict(width=0.25, shallow=True))):
        m = build(kw)
        sd = m.state_dict()
        wd = m.regime[0]['regularizer']['filter']
        decayed = [n + '.' + pn for n, mod in m.named_modules() for pn, _ in mod.named_parameters(recurse=False)
                   if wd['module'](mod) and wd['parameter_name'](pn)]
        out[tag] = {'model_kw': kw, 'keys': list(sd.keys()), 'shapes': [list(v.shape) for v in sd.values()],
                    'n_params': sum(p.numel() for p in m.parameters()),
                    'n_depthwise': sum(1 for x in m.modules() if isinstance(x, torch.nn.Conv2d) and x.groups > 1),
                    'decayed': decayed,
                    'regime': describe_regime(m.regime), 'data_regime': describe_regime(m.data_regime)}
        if tag == 'w0.25_shallow':
            out[tag]['init_sums'] = mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point})
        ms = mg.ref_models.mobilenet(regime='small', **kw)
        out[tag]['small'] = {'regime': describe_regime(ms.regime), 'data_regime': describe_regime(ms.data_regime),
                             'data_eval_regime': describe_regime(ms.data_eval_regime),
                             'wd_value': ms.regime[0]['regularizer']['value']}
    assert len(out['w1.0']['keys']) == 177 and out['w1.0']['n_params'] == 4236936, (len(out['w1.0']['keys']),
                                                                                   out['w1.0']['n_params'])
    with open(os.path.join(mg.OUT, 'structure_mobilenet.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print({t: (len(v['keys']), v['n_params'], v['n_depthwise']) for t, v in out.items()})


def run_reference(kw, B, size, lr, steps, seed, dtype):
    """`steps` steps of the reference Trainer in `dtype`; per step: the meter record, the raw step-0 gradients (tensor
    hooks: the regulariser adds wd*p to p.grad before the optimizer step), the state dict and the validate record."""
    model = build(kw)
    init = {k: v.clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    model.to(dtype)
    opt = mg.OptimRegime(model, [dict(model.regime[0], lr=lr)])
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=dtype, distributed=False,
                       loss_scale=1.0, grad_clip=1e9, print_freq=10 ** 9)
    data = mg.batches(steps, B, size, CLASSES, seed)
    raw, handles = {}, []
    for k, p in model.named_parameters():
        handles.append(p.register_hook(lambda g, k=k: raw.__setitem__(k, g.detach().clone())))
    recs, states, vals, grads0 = [], [], [], None
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if i == 0:
            grads0 = dict(raw)
            for h in handles:
                h.remove()
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        v = tr.validate(data[:2])
        vals.append({k: float(v[k]) for k in ('loss', 'prec1', 'prec5')})
    return {'init': init, 'recs': recs, 'states': states, 'vals': vals, 'grads0': grads0, 'data': data}


def self_deviation(r64, r32):
    """fp32 reference against float64 reference: per step, and per tensor of the state after each step."""
    steps = []
    for i, (a, b) in enumerate(zip(r32['recs'], r64['recs'])):
        fin = {k: mg.rel_l2(r32['states'][i][k], v) for k, v in r64['states'][i].items() if v.dtype.is_floating_point}
        steps.append({'loss_abs': abs(a['loss'] - b['loss']), 'grad_rel': abs(a['grad'] - b['grad']) / b['grad'],
                      'prec_same': a['prec1'] == b['prec1'] and a['prec5'] == b['prec5'],
                      'final_rel_l2_max': max(fin.values()),
                      'validate_loss_rel': abs(r32['vals'][i]['loss'] - r64['vals'][i]['loss']) / r64['vals'][i]['loss'],
                      'validate_prec_same': all(r32['vals'][i][k] == r64['vals'][i][k] for k in ('prec1', 'prec5')),
                      'final_rel_l2': fin})
    return steps


def checked_prefix(dev, check_final):
    """Longest prefix k: every step < k within a tenth of the per-step bounds, and the state / validate record after step
    k - 1 (what the test compares at the end of its run) within a tenth of theirs."""
    best = 0
    for k in range(1, len(dev) + 1):
        ok = all(d['loss_abs'] <= BOUNDS['loss_abs'] / 10 and d['grad_rel'] <= BOUNDS['grad_rel'] / 10 and d['prec_same']
                 for d in dev[:k])
        last = dev[k - 1]
        ok = ok and (not check_final or last['final_rel_l2_max'] <= BOUNDS['final_rel_l2'] / 10) \
            and last['validate_loss_rel'] <= BOUNDS['validate_loss_rel'] / 10 and last['validate_prec_same']
        if ok:
            best = k
    return best


def trajectory(tag, kw, B, size, lr, steps, seed, all_tensors, grad0):
    r64 = run_reference(kw, B, size, lr, steps, seed, torch.double)
    r32 = run_reference(kw, B, size, lr, steps, seed, torch.float)
    dev = self_deviation(r64, r32)
    k = checked_prefix(dev, all_tensors)     # (final tensors are compared where the fixture stores them)
    print(tag, 'fp32 reference vs float64 reference per step:',
          [{n: (v if isinstance(v, bool) else float('%.3g' % v)) for n, v in d.items() if n != 'final_rel_l2'} for d in dev],
          'checked_steps', k)
    assert k >= 2, '%s: the fp32 reference leaves the float64 one within %d step(s)' % (tag, k)
    sd = r64['states'][k - 1]
    out = {'tag': tag, 'model_kw': kw, 'B': B, 'size': size, 'classes': CLASSES, 'steps': steps, 'seed': seed, 'lr': lr,
           'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0, 'reference_dtype': 'float64',
           'records': r64['recs'], 'checked_steps': k, 'validate': r64['vals'][k - 1], 'bounds': BOUNDS,
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in r64['data']],
           'init_sums': mg.tensor_sums(r64['init']),
           'final_sums': mg.tensor_sums({n: v for n, v in sd.items() if v.dtype.is_floating_point}),
           'num_batches_tracked': int(sd['features.1.num_batches_tracked']),
           'ref_self': {'steps': dev}}
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    if all_tensors:
        torch.save({n: v.float().clone() for n, v in sd.items() if v.dtype.is_floating_point},
                   os.path.join(mg.OUT, 'traj_%s_final.pt' % tag))
    if grad0:
        g64, g32 = r64['grads0'], r32['grads0']
        tens, meta = {}, {}
        for n, g in g64.items():
            s = mg.sample_tensor(g, n)
            s32 = mg.sample_tensor(g32[n], n)
            tens[n] = {'norm': s['norm'], 'val': s['val']}
            meta[n] = {'norm': s['norm'], 'numel': s['numel'],
                       'self_norm_rel': abs(s32['norm'] - s['norm']) / max(s['norm'], 1e-300),
                       'self_rel_l2': mg.rel_l2(s32['val'], s['val'])}
        dw_bias = [n for n in meta if n.endswith('components.0.bias')]
        worst = max(max(v['self_norm_rel'], v['self_rel_l2']) for n, v in meta.items() if n not in dw_bias)
        print('  step-0 gradients: worst fp32-reference deviation (depthwise biases aside) %.3g' % worst,
              '; depthwise bias / weight gradient norms',
              [(float('%.2g' % meta[n]['norm']), float('%.2g' % meta[n[:-4] + 'weight']['norm'])) for n in dw_bias[:3]])
        assert worst <= GRAD0_MAX_SELF, worst
        with open(os.path.join(mg.OUT, 'traj_%s_grad0.json' % tag), 'w') as f:
            json.dump({'tag': tag, 'params': meta, 'depthwise_biases': dw_bias, 'floor': GRAD0_FLOOR,
                       'factor': GRAD0_FACTOR, 'worst_self': worst}, f, indent=1, sort_keys=True)
        torch.save(tens, os.path.join(mg.OUT, 'traj_%s_grad0.pt' % tag))


if __name__ == '__main__':
    which = sys.argv[1:] or ['structure', 'mbs', 'mbs_shallow']
    if 'structure' in which:
        structure()
    if 'mbs' in which:
        trajectory('mbs', MBS, B=16, size=64, lr=0.01, steps=2, seed=5, all_tensors=False, grad0=True)
    if 'mbs_shallow' in which:
        trajectory('mbs_shallow', MBS_SHALLOW, B=16, size=32, lr=0.01, steps=3, seed=5, all_tensors=True, grad0=False)
    mg.assert_no_new_bytecode()
