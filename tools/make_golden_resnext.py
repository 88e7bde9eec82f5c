"""Golden fixtures for ResNeXt (tests/test_resnext.py) from the unmodified reference on CPU, with the recipes of
oracle/make_golden.py: the reference's resnet(...) builds a ResNeXt when given groups / width / expansion.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_resnext.py

Writes under tests/golden/:
  structure_resnext.json        keys, shapes, parameter counts of resnext(depth=d), d = 18 / 34 / 50 / 101 / 152
  traj_rx50s                    small ResNeXt-50 (grouped shapes (4, 4), (8, 8) s1 / s2, (16, 16) s1 / s2), 4 steps
  traj_rx18s                    small BasicBlock model (conv1 AND conv2 grouped; the reference's resnet() builds depth 18
                                with expansion 1: per-group widths (2, 4), (4, 8), (4, 4), (8, 8)), 4 steps
  traj_rx50s_warm               rx50s with the warm BatchNorm recipe, reference run in float64 (step-0 gradients of the
                                grouped filters are non-zero: cold init zeroes the last gamma of every block)
  traj_rx50_full                resnext(depth=50) defaults, B = 4, 224x224, 2 steps, reference run in float64"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as mg  # noqa: E402  (puts the reference and its shim on sys.path)
import torch  # noqa: E402

RX50S = dict(depth=50, inplanes=8, width=[16, 32, 64, 128], groups=[4, 4, 8, 8], num_classes=16)
RX18S = dict(depth=18, expansion=2, inplanes=8, width=[16, 32, 64, 64], groups=[4, 4, 8, 8], num_classes=16)
RX50_FULL = dict(depth=50, width=[128, 256, 512, 1024], groups=[32, 32, 32, 32], expansion=2)


def trajectory_f64(tag, model_kw, B, size, classes, steps, seed):
    """oracle/make_golden.py's `trajectory` recipe with the reference run in float64 (the same seeded model and batches,
    the reference Trainer with dtype=torch.double).  At 224x224 the reference's own fp32 run is 1.0e-3 off the float64
    gradient norm at step 0 - PyTorch's CPU grouped convolution sums 9 * C/g products per output in an order of its
    own - which is the whole fp32 tolerance; a float64 fixture measures the engine against the truth instead."""
    torch.manual_seed(123)
    model = mg.ref_models.resnet(dataset='imagenet', **model_kw)
    init_sums = mg.tensor_sums({k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point})
    model.double()
    opt = mg.OptimRegime(model, model.regime)
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=torch.double,
                       distributed=False, loss_scale=1.0, grad_clip=1e9, print_freq=10 ** 9)
    data = mg.batches(steps, B, size, classes, seed)
    recs = []
    for x, t in data:
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
    val = tr.validate(data[:2])
    sd = model.state_dict()
    out = {'tag': tag, 'model_kw': model_kw, 'B': B, 'size': size, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0,
           'reference_dtype': 'float64', 'records': recs,
           'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')},
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in data],
           'init_sums': init_sums,
           'final_sums': mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point}),
           'num_batches_tracked': int(sd['bn1.num_batches_tracked'])}
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    keep = ['conv1.weight', 'bn1.running_mean', 'bn1.running_var', 'layer1.0.conv1.weight', 'layer1.0.conv2.weight',
            'fc.bias']
    torch.save({k: sd[k].float().clone() for k in keep}, os.path.join(mg.OUT, 'traj_%s_final.pt' % tag))
    print(tag, recs, 'val', out['validate'])


def structure():
    """Keys, shapes and parameter counts of the reference's resnext(depth=d) defaults."""
    out = {}
    for depth in (18, 34, 50, 101, 152):
        torch.manual_seed(0)
        m = mg.ref_models.resnext(depth=depth)
        sd = m.state_dict()
        out[str(depth)] = {'keys': list(sd.keys()), 'shapes': [list(v.shape) for v in sd.values()],
                           'n_params': sum(p.numel() for p in m.parameters()),
                           'n_grouped': sum(1 for x in m.modules() if isinstance(x, torch.nn.Conv2d) and x.groups > 1)}
    with open(os.path.join(mg.OUT, 'structure_resnext.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print({d: (v['n_params'], v['n_grouped']) for d, v in out.items()})


if __name__ == '__main__':
    which = sys.argv[1:] or ['structure', 'rx50s', 'rx18s', 'rx50s_warm', 'rx50_full']
    if 'structure' in which:
        structure()
    if 'rx50s' in which:
        mg.trajectory('rx50s', RX50S, B=8, size=32, classes=16, steps=4, seed=41)
    if 'rx18s' in which:
        mg.trajectory('rx18s', RX18S, B=8, size=32, classes=16, steps=4, seed=42)
    if 'rx50s_warm' in which:
        mg.warm_trajectory('rx50s_warm', RX50S, B=8, size=32, classes=16, steps=3, seed=43, dtype=torch.double)
    if 'rx50_full' in which:
        trajectory_f64('rx50_full', RX50_FULL, B=4, size=224, classes=1000, steps=2, seed=44)
    mg.assert_no_new_bytecode()
