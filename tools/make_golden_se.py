"""Golden fixtures for the squeeze-excite ResNet (tests/test_se.py, tests/test_resnet_se.py) from the unmodified reference
on CPU, with the recipes of oracle/make_golden.py: the reference's resnet_se(**config) is resnet(residual_block=SEBlock,
**config), ONE SEBlock per stage shared by every block of the stage, applied to the SHORTCUT.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_se.py

Writes under tests/golden/:
  structure_se.json      state_dict keys in order (alias keys included), shapes, parameter count and the named_parameters()
                         names of resnet_se(depth=d), d = 18 / 50
  se_ops.pt              records of the reference MODULE (models/modules/se.py SEBlock, float64) at the operator-test shapes:
                         the seed of the inputs, and out / dr / the four parameter gradients / the gate m it returned
  traj_r50s_se           make_golden.SMALL, depth 50, 4 steps (fp32 reference)
  traj_r18s_se           depth 18 at width 16 .. 128 (hidden widths 1, 2, 4, 8), 4 steps
  traj_rx18s_se          the same with groups=[2, 2, 2, 2], 2 steps
  traj_r50s_se_warm      the small ResNet-50 with make_golden.warm_bn_state (last gammas non-zero), reference in float64,
                         3 steps; step-0 gradient of EVERY unique parameter as norm + sample"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as mg  # noqa: E402  (puts the reference and its shim on sys.path)
import torch  # noqa: E402

# (N, H, W, C, C // ratio) of the operator tests; the last two are the GPU-only real widths
OP_SHAPES = [(2, 1, 1, 16, 1), (3, 7, 5, 32, 2), (2, 9, 9, 64, 4), (1, 37, 1, 1040, 65), (4, 28, 28, 16, 1),
             (2, 56, 56, 8, 2), (2, 56, 56, 256, 16), (2, 7, 7, 2048, 128)]
R18S = dict(depth=18, width=[16, 32, 64, 128], inplanes=16, num_classes=16)
SE_KEEP = ['layer1.0.residual_block.transform.0.weight', 'layer1.0.residual_block.transform.2.bias',
           'layer3.0.residual_block.transform.0.bias', 'layer4.0.residual_block.transform.2.weight']


def build(model_kw):
    model = mg.ref_models.resnet_se(dataset='imagenet', **model_kw)
    from models.modules.se import SEBlock
    for s in (1, 2, 3, 4):
        stage = getattr(model, 'layer%d' % s)
        assert isinstance(stage[0].residual_block, SEBlock)
        assert all(b.residual_block is stage[0].residual_block for b in stage)
    return model


def op_inputs(shape, signed, seed):
    """Seeded inputs of one operator record in the reference's layouts, rounded to bf16 (exact in f16 - but for the few
    values below 2^-14 - and in fp32).  signed: the shortcut BatchNorm's output (first block of a stage); otherwise a
    post-ReLU block input.  tests/test_se.py restates this."""
    N, H, W, C, Cr = shape
    g = torch.Generator().manual_seed(seed)

    def draw(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).bfloat16().double()
    r = (draw(N, C, H, W) + draw(N, C, 1, 1, scale=0.7) + draw(1, C, 1, 1, scale=0.5)).bfloat16().double()
    if not signed:
        r = r.clamp_min(0)
    w1, b1 = draw(Cr, C, scale=2.0 / C ** 0.5), draw(Cr, scale=0.3)
    w2, b2 = draw(C, Cr, scale=1.5 / Cr ** 0.5), draw(C, scale=0.5)
    dout = draw(N, C, H, W)
    return r, w1, b1, w2, b2, dout


def op_records():
    """The inputs are not stored (seed + sums: op_inputs regenerates them); every returned tensor goes through
    make_golden.sample_tensor (norm, sum, up to 2048 seeded samples - the whole tensor below that)."""
    from models.modules.se import SEBlock
    recs = []
    for shape in OP_SHAPES:
        N, H, W, C, Cr = shape
        small = N * H * W * C <= 16384
        for signed in ((1, 0) if small else ((1,) if C in (8, 256) else (0,))):
            seed = 4100 + len(recs)
            r, w1, b1, w2, b2, dout = op_inputs(shape, signed, seed)
            assert C % Cr == 0
            se = SEBlock(C, ratio=C // Cr).double()
            with torch.no_grad():
                se.transform[0].weight.copy_(w1)
                se.transform[0].bias.copy_(b1)
                se.transform[2].weight.copy_(w2)
                se.transform[2].bias.copy_(b2)
            rr = r.clone().requires_grad_(True)
            out = se(rr)
            out.backward(dout)
            with torch.no_grad():
                m = se.transform(r.mean((2, 3)))
            recs.append({'shape': list(shape), 'signed': signed, 'seed': seed,
                         'input_sums': [float(t.sum()) for t in (r, w1, b1, w2, b2, dout)],
                         'out': mg.sample_tensor(out, 'out'), 'dr': mg.sample_tensor(rr.grad, 'dr'),
                         'dw1': mg.sample_tensor(se.transform[0].weight.grad, 'dw1'),
                         'db1': mg.sample_tensor(se.transform[0].bias.grad, 'db1'),
                         'dw2': mg.sample_tensor(se.transform[2].weight.grad, 'dw2'),
                         'db2': mg.sample_tensor(se.transform[2].bias.grad, 'db2'),
                         'm': mg.sample_tensor(m, 'm')})
    keys = list(SEBlock(32).state_dict().keys())
    torch.save({'records': recs, 'state_dict_keys': keys}, os.path.join(mg.OUT, 'se_ops.pt'))
    print('se_ops.pt', len(recs), 'records', keys, os.path.getsize(os.path.join(mg.OUT, 'se_ops.pt')), 'bytes')


def structure():
    out = {}
    for depth in (18, 50):
        torch.manual_seed(0)
        m = build(dict(depth=depth))
        sd = m.state_dict()
        out[str(depth)] = {'keys': list(sd.keys()), 'shapes': [list(v.shape) for v in sd.values()],
                           'n_params': sum(p.numel() for p in m.parameters()),
                           'named_parameters': [k for k, _ in m.named_parameters()]}
    with open(os.path.join(mg.OUT, 'structure_se.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print({d: (v['n_params'], len(v['keys']), len(v['named_parameters'])) for d, v in out.items()})


def trajectory(tag, model_kw, B, size, classes, steps, seed):
    """make_golden.trajectory's recipe and fields on resnet_se; a few SE tensors among the kept final tensors."""
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
    out = {'tag': tag, 'model_kw': model_kw, 'B': B, 'size': size, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0, 'records': recs,
           'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')},
           'input_sums': [[float(x.double().sum()), float(t.sum())] for x, t in data],
           'init_sums': init_sums,
           'final_sums': mg.tensor_sums({k: v for k, v in sd.items() if v.dtype.is_floating_point}),
           'n_params': sum(p.numel() for p in model.parameters()), 'n_keys': len(sd),
           'num_batches_tracked': int(sd['bn1.num_batches_tracked'])}
    with open(os.path.join(mg.OUT, 'traj_%s.json' % tag), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    keep = ['conv1.weight', 'bn1.running_mean', 'bn1.running_var', 'layer1.0.conv1.weight',
            'layer2.0.downsample.0.weight', 'layer4.1.bn2.weight', 'fc.weight', 'fc.bias'] + SE_KEEP
    torch.save({k: sd[k].clone() for k in keep if k in sd}, os.path.join(mg.OUT, 'traj_%s_final.pt' % tag))
    print(tag, recs[0], recs[-1], 'val', out['validate'], out['n_params'], out['n_keys'])


def warm_trajectory(tag, model_kw, B, size, classes, steps, seed):
    """make_golden.warm_trajectory's recipe (warm_bn_state: every BatchNorm with a seeded non-trivial state, the last gamma
    of every block in [0.03, 0.1)) with the reference in float64; the raw autograd gradient of step 0 is recorded for
    EVERY unique parameter (tensor hooks: the regulariser adds wd*p to p.grad in place).  A shared SE parameter's hook sees
    the sum over the blocks of its stage."""
    torch.manual_seed(123)
    model = build(model_kw)
    mg.warm_bn_state(model)
    model.double()
    data = mg.batches(steps, B, size, classes, seed)
    start_sums = mg.tensor_sums({k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point})
    opt = mg.OptimRegime(model, model.regime)
    tr = mg.RefTrainer(model, mg.CrossEntropyLoss(), opt, device_ids=None, device='cpu', dtype=torch.double,
                       distributed=False, grad_clip=1e9, print_freq=10 ** 9)
    params = dict(model.named_parameters())
    raw, calls, handles = {}, {}, []

    def hook(g, k):
        calls[k] = calls.get(k, 0) + 1
        raw[k] = g.detach().clone()
    for k, p in params.items():
        handles.append(p.register_hook(lambda g, k=k: hook(g, k)))
    recs, grads0 = [], None
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if i == 0:
            assert set(raw) == set(params) and set(calls.values()) == {1}
            grads0 = {k: mg.sample_tensor(raw[k], k) for k in params}
            for h in handles:
                h.remove()
            raw.clear()
    val = tr.validate(data[:2])
    sd = model.state_dict()
    out = {'tag': tag, 'model_kw': model_kw, 'B': B, 'size': size, 'classes': classes, 'steps': steps,
           'seed': seed, 'loss_scale': 1.0, 'grad_clip': 1e9, 'chunk_batch': 1, 'smooth_eps': 0.0,
           'warm_seed': mg.WARM_SEED, 'warm_last_gamma': list(mg.WARM_LAST_GAMMA), 'reference_dtype': 'float64',
           'records': recs, 'validate': {k: float(val[k]) for k in ('loss', 'prec1', 'prec5')},
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
    print('  SE:', {k: v for k, v in out['grad0_norms'].items() if 'residual_block' in k and k.startswith('layer1')})


if __name__ == '__main__':
    which = sys.argv[1:] or ['ops', 'structure', 'r50s_se', 'r18s_se', 'rx18s_se', 'r50s_se_warm']
    if 'ops' in which:
        op_records()
    if 'structure' in which:
        structure()
    if 'r50s_se' in which:
        trajectory('r50s_se', dict(depth=50, **mg.SMALL), B=8, size=32, classes=16, steps=4, seed=51)
    if 'r18s_se' in which:
        trajectory('r18s_se', dict(R18S), B=8, size=32, classes=16, steps=4, seed=52)
    if 'rx18s_se' in which:
        trajectory('rx18s_se', dict(R18S, groups=[2, 2, 2, 2]), B=8, size=32, classes=16, steps=2, seed=53)
    if 'r50s_se_warm' in which:
        warm_trajectory('r50s_se_warm', dict(depth=50, **mg.SMALL), B=8, size=32, classes=16, steps=3, seed=54)
    mg.assert_no_new_bytecode()
