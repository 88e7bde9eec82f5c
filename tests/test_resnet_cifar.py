"""resnet(dataset='cifar10' | 'cifar100') (models/resnet.py: ResNetCifar) against the reference's ResNet_cifar.

  * structure / seeded construction / regimes: tests/golden/structure_cifar.json (tools/make_golden_cifar.py, from the reference);
  * strict load of a reference-layout state dict, the weight-decay filter, the refusals;
  * trajectories traj_c8 / traj_c20 (cifar100: the ragged 100-way head) / traj_c8_wide_drop (widths 32-128, Dropout(0.3) with
    the reference's host draws, the wide-resnet regime) with test_resnext.py's bounds (fp32: loss abs 1e-4, grad-norm rel 1e-3,
    prec identical, final tensors rel-L2 1e-4, validate loss rel 1e-3; bf16 / f16: _check_bf16's bounds on the first two steps;
    the emulator, which runs one lane at a time, needed 33 minutes on 8 cores for every step of every case of this file, so
    there the depth-8 fixtures run every step (c8, fp32) or the first two (c8_wide_drop; both in 16 bit) and the depth-20
    fixtures one step - the GPU runs all of them);
  * warm start traj_c20_warm (reference in float64, every BatchNorm non-trivial): step-0 gradient of EVERY parameter, norm rel
    5e-3 and sampled rel-L2 5e-3;
  * GPU: the plan is bit-identical to eager launches; the CLI on cifar10-synthetic (emulator: depth 8)."""
import json
import os

import pytest
import torch

from conftest import HAS_GPU
from helpers import GOLDEN, golden_batches, load_traj, load_warm, rel_l2, sample_tensor, warm_bn_state

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _structure():
    with open(os.path.join(GOLDEN, 'structure_cifar.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', ['cifar10_d8', 'cifar10_d20', 'cifar10_d44', 'cifar100_d20'])
def test_structure_and_seeded_construction_match_reference(name):
    import convnet_amd as ca
    ref = _structure()[name]
    torch.manual_seed(123)
    m = ca.models.resnet(**ref['model_kw'])
    sd = m.state_dict()
    assert list(sd.keys()) == ref['keys']
    assert [list(v.shape) for v in sd.values()] == ref['shapes']
    assert sum(p.numel() for p in m.parameters()) == ref['params']
    assert 'bn1.num_batches_tracked' in sd and not hasattr(m, 'layer4') and not hasattr(m, 'maxpool')
    assert [{k: v for k, v in r.items() if k != 'regularizer'} for r in m.regime] == ref['regime']
    assert m.regime[0]['regularizer']['value'] == ref['weight_decay'] == 1e-4
    if 'init_sums' in ref:
        for k, (s, a) in ref['init_sums'].items():
            v = sd[k].double()
            assert float(v.sum()) == pytest.approx(s, rel=1e-12, abs=1e-12), k
            assert float(v.abs().sum()) == pytest.approx(a, rel=1e-12, abs=1e-12), k


def test_defaults_and_wide_regime():
    import convnet_amd as ca
    m = ca.models.resnet(dataset='cifar10')
    assert m.fc.out_features == 10 and len(m.layer1) == len(m.layer2) == len(m.layer3) == 7      # depth 44
    assert m.conv1.kernel_size == (3, 3) and m.conv1.stride == (1, 1) and m.conv1.padding == (1, 1)
    assert m.layer1[0].downsample is None and m.layer2[0].downsample is not None and m.layer3[0].downsample is not None
    assert ca.models.resnet(dataset='cifar100', depth=8).fc.out_features == 100
    assert ca.models.resnet(dataset='cifar10', depth=8, inplanes=8).layer1[0].downsample is not None      # inplanes != width[0]
    w = ca.models.resnet(dataset='cifar10', depth=8, regime='wide-resnet')
    ref = _structure()['wide_regime']
    assert [{k: v for k, v in r.items() if k != 'regularizer'} for r in w.regime] == ref['regime']
    assert w.regime[0]['regularizer']['value'] == ref['weight_decay'] == 5e-4
    for blk in m.layer2:        # init_model: the last gamma of every block is zero
        assert float(blk.bn2.weight.detach().abs().sum()) == 0.0
    assert float(m.fc.bias.detach().abs().sum()) == 0.0


def test_dropout_sits_behind_the_first_relu_and_turns_that_blocks_fusions_off():
    import convnet_amd as ca
    plain = ca.models.resnet(dataset='cifar10', depth=8)
    drop = ca.models.resnet(dataset='cifar10', depth=8, dropout=0.3)
    assert list(plain.state_dict()) == list(drop.state_dict())
    for blk in drop.layer1:
        assert blk.dropout.p == 0.3 and 'input_bn' not in blk.conv2.__dict__ and 'inner_consumer_conv' not in blk.bn1.__dict__
        assert blk.conv1.__dict__['stats_bn'] is blk.bn1 and blk.conv2.__dict__['stats_bn'] is blk.bn2
    for blk in plain.layer1:
        assert blk.dropout.p == 0 and blk.conv2.__dict__['input_bn'] is blk.bn1
        assert blk.bn1.__dict__['inner_consumer_conv'] is blk.conv2
    assert plain.layer2[0].conv1.__dict__['input_bn'] is plain.layer1[0].bn2


def test_strict_load_of_a_reference_layout_state_dict():
    import convnet_amd as ca
    ref = _structure()['cifar10_d20']
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.tensor(7) if k.endswith('num_batches_tracked') else torch.randn(shape, generator=g))
          for k, shape in zip(ref['keys'], ref['shapes'])}
    m = ca.models.resnet(dataset='cifar10', depth=20)
    m.load_state_dict(sd, strict=True)
    out = m.state_dict()
    for k in sd:
        assert torch.equal(out[k], sd[k]), k


def test_weight_decay_filter():
    import convnet_amd as ca
    m = ca.models.resnet(dataset='cifar10', depth=8)
    f = m.regime[0]['regularizer']['filter']
    decayed = [n + '.' + pn for n, mod in m.named_modules() if f['module'](mod)
               for pn, _ in mod.named_parameters(recurse=False) if f['parameter_name'](pn)]
    want = [k for k in m.state_dict() if k.endswith('.weight') and '.bn' not in k and not k.startswith('bn')
            and 'downsample.1' not in k]
    assert sorted(decayed) == sorted(want) and 'fc.weight' in decayed and 'fc.bias' not in decayed


@pytest.mark.parametrize('kw, reason', [
    (dict(regime='sampled'), 'sampled'), (dict(regime='sampled_D+'), 'sampled'), (dict(mixup=True), 'MixUp'),
    (dict(quantize=True), 'quantize=.*quantised operators'), (dict(bn_norm='L1'), 'bn_norm=.*L1 norm'),
    (dict(groups=[2, 2, 2]), 'grouped convolutions'), (dict(residual_block=object), 'residual_block=.*gated shortcut')],
    ids=['sampled', 'sampled_D', 'mixup', 'quantize', 'bn_norm', 'groups', 'residual_block'])
def test_refusals_name_their_reason(kw, reason):
    """Each option is refused under its own name and reason, and the message says which CIFAR dataset it was."""
    import convnet_amd as ca
    with pytest.raises(NotImplementedError, match=reason) as e:
        ca.models.resnet(dataset='cifar10', **kw)
    assert 'cifar' in str(e.value)


def test_pinned_refusals_still_hold():
    import convnet_amd as ca
    with pytest.raises(NotImplementedError):
        ca.models.resnext(dataset='cifar10')
    with pytest.raises(NotImplementedError):
        ca.models.resnet_se(dataset='cifar10')
    with pytest.raises(NotImplementedError):
        ca.models.resnet(dataset='cifar10', bn_norm='TopK')
    with pytest.raises(NotImplementedError):
        ca.models.resnet(dataset='mnist')
    assert ca.models.resnet(dataset='cifar10', groups=[1, 1, 1], depth=8).fc.out_features == 10


def _run(meta, dtype, device, steps=None, graph=True, grads_after_step0=None):
    """helpers.run_engine_trajectory for a fixture that names its dataset."""
    import convnet_amd as ca
    torch.manual_seed(123)
    model = ca.models.resnet(dataset=meta['dataset'], **meta['model_kw'])
    if meta.get('warm_seed') is not None:
        warm_bn_state(model, meta['warm_seed'], last_gamma=tuple(meta['warm_last_gamma']))
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(device), dtype=dtype,
                    loss_scale=meta['loss_scale'], grad_clip=meta['grad_clip'], print_freq=10 ** 9)
    if not graph:
        tr._use_graph = False
    data = golden_batches(meta)[:steps]
    recs = []
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if i == 0 and grads_after_step0 is not None:
            params = dict(model.named_parameters())
            for k in list(grads_after_step0):
                grads_after_step0[k] = sample_tensor(params[k].grad, k)
    return recs, tr, model, data


def _check_fp32(meta, final, recs, tr, model, data):
    for r, g in zip(recs, meta['records']):
        assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
        assert r['prec1'] == g['prec1'] and r['prec5'] == g['prec5']
        assert r['grad'] == pytest.approx(g['grad'], rel=1e-3)
    if len(recs) != meta['steps']:
        return
    sd = model.state_dict()
    for k, v in final.items():
        assert rel_l2(sd[k].float().cpu(), v) < 1e-4, k
    assert int(sd['bn1.num_batches_tracked']) == meta['num_batches_tracked']
    val = tr.validate(data[:2])
    assert val['loss'] == pytest.approx(meta['validate']['loss'], rel=1e-3)
    assert val['prec1'] == meta['validate']['prec1'] and val['prec5'] == meta['validate']['prec5']


def _check_bf16(meta, recs):
    B = meta['B']
    for i, (r, g) in enumerate(zip(recs, meta['records'])):
        assert r['loss'] == pytest.approx(g['loss'], abs=2e-2 if i == 0 else 5e-2), i
        assert abs(r['prec1'] - g['prec1']) <= 100.0 / B + 1e-6
        assert abs(r['prec5'] - g['prec5']) <= 100.0 / B + 1e-6
        assert r['grad'] == pytest.approx(g['grad'], rel=5e-2 if i == 0 else 1.5e-1), i


TAGS = ['c8', 'c20', 'c8_wide_drop']


def test_fixtures_are_what_they_claim():
    for tag in TAGS + ['c20_warm']:
        with open(os.path.join(GOLDEN, 'traj_%s.json' % tag)) as f:
            meta = json.load(f)
        assert meta['min_logit_gap'] > 1e-4 and meta['B'] == 8 and meta['steps'] == 3
    assert load_traj('c20')[0]['dataset'] == 'cifar100' and load_traj('c20')[0]['classes'] == 100
    kw = load_traj('c8_wide_drop')[0]['model_kw']
    assert kw['dropout'] == 0.3 and kw['width'] == [32, 64, 128] and kw['regime'] == 'wide-resnet'
    meta, tens = load_warm('c20_warm')
    assert meta['reference_dtype'] == 'float64'
    import convnet_amd as ca
    names = [k for k, _ in ca.models.resnet(dataset='cifar10', depth=20).named_parameters()]
    assert sorted(tens['grad0']) == sorted(names)
    norms = meta['grad0_norms']
    for k in names:        # every parameter has a step-0 gradient of natural size: any wrong kernel shows
        assert norms[k] > 1e-4 * max(norms.values()), k


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('tag', TAGS)
def test_fp32_trajectory(mode, tag):
    dev = _dev(mode)
    meta, final = load_traj(tag)
    steps = None if (mode == 'gpu' or tag == 'c8') else (2 if tag == 'c8_wide_drop' else 1)     # (emulator cost: see above)
    recs, tr, model, data = _run(meta, torch.float32, dev, steps, graph=False)
    _check_fp32(meta, final, recs, tr, model, data)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('tag', TAGS)
def test_16bit_trajectory(mode, dtype, tag):
    dev = _dev(mode)
    meta, _ = load_traj(tag)
    steps = 2 if (mode == 'gpu' or tag != 'c20') else 1     # (emulator cost: see above)
    recs, tr, model, data = _run(meta, dtype, dev, steps)
    assert len(recs) == steps
    _check_bf16(meta, recs)


@pytest.mark.parametrize('mode', MODES)
def test_fp32_warm_step0_gradients(mode):
    dev = _dev(mode)
    meta, tens = load_warm('c20_warm')
    grads = {k: None for k in tens['grad0']}
    recs, tr, model, data = _run(meta, torch.float32, dev, 1, graph=False, grads_after_step0=grads)
    r, g = recs[0], meta['records'][0]
    assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
    assert r['grad'] == pytest.approx(g['grad'], rel=5e-3)
    for k, gold in tens['grad0'].items():
        norm, val = grads[k]
        assert gold['norm'] > 0, k
        assert norm == pytest.approx(gold['norm'], rel=5e-3), (k, norm, gold['norm'])
        assert rel_l2(val, gold['val']) < 5e-3, (k, rel_l2(val, gold['val']))


@pytest.mark.gpu
def test_plan_is_bit_identical_to_eager():
    """5 training steps of depth 20 at B = 8: the recorded launch plan against plan = 0."""
    import convnet_amd as ca
    dev = _dev('gpu')
    g = torch.Generator().manual_seed(9)
    data = [(torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(5)]
    outs = []
    for plan in (False, True):
        torch.manual_seed(123)
        model = ca.models.resnet(dataset='cifar10', depth=20)
        warm_bn_state(model, 977)
        tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(dev),
                        dtype=torch.bfloat16, grad_clip=1e9, print_freq=10 ** 9)
        tr._graph_mode = '1' if plan else '0'
        tr._use_graph = plan
        losses = [float(tr.train([(x, t)])['loss']) for x, t in data]
        torch.cuda.synchronize()
        if plan:
            assert any(s['graph'] is not None and s['graph'].get('plan') is not None for s in tr._gstates.values()), \
                'the step never ran as a recorded plan'
        outs.append((losses, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()
                              if v.dtype.is_floating_point}))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize('mode', MODES)
def test_cli_one_epoch_on_synthetic_cifar(mode, tmp_path):
    """--dataset cifar10-synthetic: 32 x 32 inputs and 10 classes by default; train, validate, checkpoint, resume."""
    dev = _dev(mode)
    from convnet_amd.main import main
    depth, b, steps = (20, '8', '3') if mode == 'gpu' else (8, '4', '1')      # (the emulator runs one lane at a time)
    common = ['--model', 'resnet', '--dataset', 'cifar10-synthetic', '--model-config', "{'depth': %d}" % depth, '-b', b,
              '--device', 'cuda' if dev.type == 'cuda' else 'cpu', '--steps-per-epoch', steps, '--val-steps', '1',
              '--results-dir', str(tmp_path), '--print-freq', '1']
    out = main(common + ['--save', 'run', '--epochs', '1'])
    ck = torch.load(tmp_path / 'run' / 'checkpoint.pth.tar', map_location='cpu')
    assert ck['epoch'] == 1 and tuple(ck['state_dict']['fc.weight'].shape) == (10, 64)
    assert tuple(ck['state_dict']['conv1.weight'].shape) == (16, 3, 3, 3)
    assert out['train']['loss'] == out['train']['loss'] and out['val']['loss'] > 0
    main(common + ['--save', 'run2', '--epochs', '2', '--resume', str(tmp_path / 'run' / 'checkpoint.pth.tar')])
    assert torch.load(tmp_path / 'run2' / 'checkpoint.pth.tar', map_location='cpu')['epoch'] == 2
