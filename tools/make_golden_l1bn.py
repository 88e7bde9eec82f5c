"""Golden fixtures for L1 batch norm (tests/test_l1bn.py, tests/test_resnet_l1.py) from the unmodified reference on CPU,
with the recipes of oracle/make_golden.py: the reference's resnet(bn_norm='L1') rebinds torch.nn.BatchNorm2d to its
models/modules/lp_norm.py L1BatchNorm2d before it builds the model.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_l1bn.py

Writes under tests/golden/:
  l1bn_ops.pt            records of the reference MODULE (L1BatchNorm2d, float64) at the operator-test shapes: the seed of the
                         inputs, the z / dy / dgamma / dbeta / dres it returned, both running buffers after one training
                         call, the eval-mode output
  structure_l1.json      keys in order, shapes and parameter count of resnet(depth=d, bn_norm='L1'), d = 18 / 50
  traj_r50s_l1           make_golden.SMALL + bn_norm='L1', depth 50, 4 steps (fp32 reference)
  traj_r18s_l1           the same, depth 18
  traj_rx18s_l1          make_golden_resnext.RX18S + bn_norm='L1' (grouped 3x3 convolutions), 2 steps
  traj_r50s_l1_warm      the small ResNet-50 with a seeded non-trivial state of every L1 norm, reference in float64, 3 steps;
                         step-0 gradient of EVERY parameter as norm + sample

The rebinding is process-global: every model build here is followed by restoring torch.nn.BatchNorm2d, and that is
asserted."""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import make_golden as mg  # noqa: E402  (puts the reference and its shim on sys.path)
import torch  # noqa: E402
from make_golden_resnext import RX18S  # noqa: E402

REAL_BN = torch.nn.BatchNorm2d
assert REAL_BN.__module__.startswith('torch.nn')

# (N, H, W, C) of the operator tests and the (relu, residual) combinations recorded for each
OP_SHAPES = [(2, 1, 1, 8), (3, 7, 5, 24), (2, 9, 9, 64), (1, 37, 1, 1040), (4, 28, 28, 16), (2, 56, 56, 8)]
WARM_SEED = 977


def build(model_kw):
    """The reference's resnet(bn_norm='L1', ...); torch.nn.BatchNorm2d restored afterwards."""
    from models.modules.lp_norm import L1BatchNorm2d
    try:
        model = mg.ref_models.resnet(dataset='imagenet', **model_kw)
        assert torch.nn.BatchNorm2d is L1BatchNorm2d
    finally:
        torch.nn.BatchNorm2d = REAL_BN
    assert torch.nn.BatchNorm2d is REAL_BN
    assert any(isinstance(m, L1BatchNorm2d) for m in model.modules())
    assert not any(isinstance(m, REAL_BN) for m in model.modules())
    return model


def op_inputs(shape, has_res, seed):
    """Seeded inputs of one operator record in the reference's NCHW layout, rounded to bf16 (8 mantissa bits, modest
    range: exact in f16 and fp32 too, so every compute dtype sees the same values).  tests/test_l1bn.py restates this."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(seed)

    def draw(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).bfloat16().double()
    y = (draw(N, C, H, W, scale=1.5) + draw(1, C, 1, 1, scale=0.5)).bfloat16().double()
    gamma = (torch.rand(C, generator=g) + 0.5).bfloat16().double()
    beta = draw(C, scale=0.3)
    res = draw(N, C, H, W) if has_res else None
    dz = draw(N, C, H, W)
    return y, gamma, beta, res, dz


def op_records():
    """The inputs are not stored (seed + sums: op_inputs regenerates them); every returned tensor goes through
    make_golden.sample_tensor (norm, sum, up to 2048 seeded samples - the whole tensor below that), per-channel vectors
    whole."""
    from models.modules.lp_norm import L1BatchNorm2d
    recs = []
    for shape in OP_SHAPES:
        N, H, W, C = shape
        small = N * H * W * C <= 4096
        combos = [(0, 0), (1, 0), (1, 1)] if small else [(1, 1) if C == 16 else ((0, 0) if C == 64 else (1, 0))]
        for relu, has_res in combos:
            seed = 2024 + len(recs)
            y, gamma, beta, res, dz = op_inputs(shape, has_res, seed)
            bn = L1BatchNorm2d(C).double()
            with torch.no_grad():
                bn.weight.copy_(gamma)
                bn.bias.copy_(beta)
            bn.train()
            yr = y.clone().requires_grad_(True)
            rr = res.clone().requires_grad_(True) if has_res else None
            out = bn(yr)
            if has_res:
                out = out + rr
            if relu:
                out = torch.relu(out)
            out.backward(dz)
            rm, rv = bn.running_mean.clone(), bn.running_var.clone()
            bn.eval()
            with torch.no_grad():
                ev = bn(y)
                if has_res:
                    ev = ev + res
                if relu:
                    ev = torch.relu(ev)
            recs.append({'shape': list(shape), 'relu': relu, 'has_res': has_res, 'seed': seed,
                         'input_sums': [float(t.sum()) for t in (y, gamma, beta, dz)] + ([float(res.sum())] if has_res else []),
                         'z': mg.sample_tensor(out, 'z'), 'dy': mg.sample_tensor(yr.grad, 'dy'),
                         'dres': mg.sample_tensor(rr.grad, 'dres') if has_res else None,
                         'z_eval': mg.sample_tensor(ev, 'z_eval'),
                         'dgamma': bn.weight.grad.float(), 'dbeta': bn.bias.grad.float(),
                         'running_mean': rm.float(), 'running_var': rv.float()})
    keys = list(L1BatchNorm2d(8).state_dict().keys())
    torch.save({'records': recs, 'state_dict_keys': keys}, os.path.join(mg.OUT, 'l1bn_ops.pt'))
    print('l1bn_ops.pt', len(recs), 'records', keys, os.path.getsize(os.path.join(mg.OUT, 'l1bn_ops.pt')), 'bytes')


def structure():
    out = {}
    for depth in (18, 50):
        torch.manual_seed(0)
        m = build(dict(depth=depth, bn_norm='L1'))
        sd = m.state_dict()
        out[str(depth)] = {'keys': list(sd.keys()), 'shapes': [list(v.shape) for v in sd.values()],
                           'n_params': sum(p.numel() for p in m.parameters())}
    with open(os.path.join(mg.OUT, 'structure_l1.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print({d: (v['n_params'], len(v['keys'])) for d, v in out.items()})


def trajectory(tag, model_kw, B, size, classes, steps, seed):
    """make_golden.trajectory's recipe and fields, minus num_batches_tracked (this norm has none)."""
    torch.manual_seed(123)
    model = build(model_kw)
    init_sums = mg.tensor_sums({k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point})
    opt = mg.OptimRegime(model, model.regime)
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=torch.float,
                       distributed=False, loss_scale=1.0, grad_clip=1e9, print_freq=10 ** 9)
    data = mg.batches(steps, B, size, classes, seed)
    recs = []
    for x, t in data:
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
    val = tr.validate(data[:2])
    sd = model.state_dict()
    assert not any(k.endswith('num_batches_tracked') for k in sd)
    out = {'tag': tag, 'model_kw': model_kw, 'B': B, 'size': size, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0, 'records': recs,
           'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')},
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in data],
           'init_sums': init_sums,
           'final_sums': mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point})}
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    keep = ['conv1.weight', 'bn1.running_mean', 'bn1.running_var', 'layer1.0.conv1.weight',
            'layer2.0.downsample.0.weight', 'layer4.1.bn2.weight', 'fc.weight', 'fc.bias']
    torch.save({k: sd[k].clone() for k in keep if k in sd}, os.path.join(mg.OUT, 'traj_%s_final.pt' % tag))
    print(tag, recs[0], recs[-1], 'val', out['validate'])


def warm_l1_state(model, seed=WARM_SEED):
    """Seeded non-trivial state of every L1 norm (module order, one generator): gamma ~ U(0.5, 1.5) - the last gamma of
    every block included -, beta ~ N(0, 0.1).  tests/test_resnet_l1.py applies the same recipe to the engine's model;
    the running buffers then come from one seeded training-mode forward (warm_running)."""
    from models.modules.lp_norm import L1BatchNorm2d
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, m in model.named_modules():
            if isinstance(m, L1BatchNorm2d):
                C = m.weight.numel()
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_mean.zero_()
                m.running_var.zero_()


def warm_batch(B, size, seed=WARM_SEED + 1):
    return torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(seed))


def warm_trajectory(tag, model_kw, B, size, classes, steps, seed):
    """make_golden.warm_trajectory's recipe with the reference in float64 and the L1 warm state; the raw autograd gradient
    of step 0 is recorded for EVERY parameter (tensor hooks: the regulariser adds wd*p to p.grad in place)."""
    torch.manual_seed(123)
    model = build(model_kw)
    warm_l1_state(model)
    model.double()
    model.train()
    with torch.no_grad():
        model(warm_batch(B, size).double())        # running buffers: 0.9 x the statistics of this batch
    data = mg.batches(steps, B, size, classes, seed)
    start_sums = mg.tensor_sums({k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point})
    opt = mg.OptimRegime(model, model.regime)
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=torch.double,
                       distributed=False, grad_clip=1e9, print_freq=10 ** 9)
    params = dict(model.named_parameters())
    raw, handles = {}, []
    for k, p in params.items():
        handles.append(p.register_hook(lambda g, k=k: raw.__setitem__(k, g.detach().clone())))
    recs, grads0 = [], None
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if i == 0:
            assert set(raw) == set(params)
            grads0 = {k: mg.sample_tensor(raw[k], k) for k in params}
            for h in handles:
                h.remove()
            raw.clear()
    val = tr.validate(data[:2])
    sd = model.state_dict()
    out = {'tag': tag, 'model_kw': model_kw, 'B': B, 'size': size, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0,
           'l1_warm_seed': WARM_SEED, 'reference_dtype': 'float64', 'records': recs,
           'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')},
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in data],
           'start_sums': start_sums,
           'final_sums': mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point}),
           'grad0_norms': {k: v['norm'] for k, v in grads0.items()}}
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    torch.save({'grad0': grads0}, os.path.join(mg.OUT, 'traj_%s_tensors.pt' % tag))
    print(tag, recs, 'val', out['validate'])
    n = sorted(out['grad0_norms'].items(), key=lambda kv: kv[1])
    print('  smallest / largest recorded step-0 gradient norms:', n[:3], n[-3:])


if __name__ == '__main__':
    which = sys.argv[1:] or ['ops', 'structure', 'r50s_l1', 'r18s_l1', 'rx18s_l1', 'r50s_l1_warm']
    if 'ops' in which:
        op_records()
    if 'structure' in which:
        structure()
    if 'r50s_l1' in which:
        trajectory('r50s_l1', dict(depth=50, bn_norm='L1', **mg.SMALL), B=8, size=32, classes=16, steps=4, seed=41)
    if 'r18s_l1' in which:
        trajectory('r18s_l1', dict(depth=18, bn_norm='L1', **mg.SMALL), B=8, size=32, classes=16, steps=4, seed=42)
    if 'rx18s_l1' in which:
        trajectory('rx18s_l1', dict(RX18S, bn_norm='L1'), B=8, size=32, classes=16, steps=2, seed=43)
    if 'r50s_l1_warm' in which:
        warm_trajectory('r50s_l1_warm', dict(depth=50, bn_norm='L1', **mg.SMALL), B=8, size=32, classes=16, steps=3,
                        seed=44)
    assert torch.nn.BatchNorm2d is REAL_BN
    mg.assert_no_new_bytecode()
