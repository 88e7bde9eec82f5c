"""resnet(bn_norm='L1') (nn.L1BatchNorm2d on csrc/l1bn.hip in the place of every BatchNorm2d) against the reference.

  * structure: keys in order / shapes / parameter counts against tests/golden/structure_l1.json (written by
    tools/make_golden_l1bn.py from the reference), seeded construction, a reference-layout state dict, the refusals;
  * trajectories: tests/golden/traj_r50s_l1 / r18s_l1 / rx18s_l1 (the reference Trainer, fp32 CPU) with test_resnext.py's
    bounds (fp32: loss abs 1e-4, grad-norm rel 1e-3, prec identical, final tensors rel-L2 1e-4, validate loss rel 1e-3;
    bf16 / f16: _check_bf16's bounds on the first two steps);
  * warm start: tests/golden/traj_r50s_l1_warm (reference in float64, every L1 norm with a seeded non-trivial state so that
    the branches carry a step-0 gradient): the step-0 gradient of EVERY parameter, norm and sampled rel-L2 within 5e-3;
  * plan == eager on the GPU, and the CLI (train, checkpoint, resume)."""
import json
import os

import pytest
import torch

from conftest import HAS_GPU
from helpers import GOLDEN, golden_batches, load_traj, load_warm, rel_l2, sample_tensor, tensor_sums

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
SMALL = dict(width=[8, 16, 32, 64], inplanes=8, num_classes=16)


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


# ---- structure ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('depth', [18, 50])
def test_structure_matches_reference(depth):
    import convnet_amd as ca
    with open(os.path.join(GOLDEN, 'structure_l1.json')) as f:
        ref = json.load(f)[str(depth)]
    m = ca.models.resnet(depth=depth, bn_norm='L1')
    sd = m.state_dict()
    assert list(sd.keys()) == ref['keys']
    assert [list(v.shape) for v in sd.values()] == ref['shapes']
    assert sum(p.numel() for p in m.parameters()) == ref['n_params']
    assert not any(k.endswith('num_batches_tracked') for k in sd)
    norms = [x for x in m.modules() if isinstance(x, ca.nn.L1BatchNorm2d)]
    assert len(norms) == (20 if depth == 18 else 53)
    assert not any(isinstance(x, ca.nn.BatchNorm2d) for x in m.modules())
    assert list(norms[0].state_dict().keys()) == ['bias', 'weight', 'running_mean', 'running_var']


def test_no_convolution_epilogue_fusion_is_wired():
    """An L1 norm takes part in no fusion: no convolution feeds it statistics, parks an operand on it or reduces its
    backward sums, and the block-input gradients are added by the fork."""
    import convnet_amd as ca
    for kw in (dict(depth=50), dict(depth=18), dict(depth=50, groups=[2, 2, 2, 2])):
        m = ca.models.resnet(bn_norm='L1', **SMALL, **kw)
        for x in m.modules():
            for attr in ('stats_bn', 'input_bn', 'producer_conv', 'inner_consumer_conv', 'consumer_conv', '_res_holder',
                         'junction_conv1'):
                assert attr not in x.__dict__, (type(x).__name__, attr)
            if isinstance(x, ca.nn.Conv2d):
                assert not getattr(x, 'feeds_batchnorm', False)
            if type(x).__name__ == 'ResidualBlock':
                assert x._holder is None
    # ... and the default model keeps every one of them
    d = ca.models.resnet(depth=50, **SMALL)
    assert d.conv1.feeds_batchnorm and 'stats_bn' in d.conv1.__dict__ and d.layer1[0]._holder is not None


def test_seeded_construction_and_weight_decay_filter():
    import convnet_amd as ca
    meta, _ = load_traj('r50s_l1')
    torch.manual_seed(123)
    m = ca.models.resnet(dataset='imagenet', **meta['model_kw'])
    sums = tensor_sums(m.state_dict())
    assert set(sums) == set(meta['init_sums'])
    for k, (s, a) in meta['init_sums'].items():
        assert sums[k][0] == pytest.approx(s, rel=1e-6, abs=1e-6), k
        assert sums[k][1] == pytest.approx(a, rel=1e-6, abs=1e-6), k
    assert sum(p.numel() for p in m.parameters()) == 378264 and len(m.state_dict()) == 267
    # gamma 1, beta 0, the last gamma of every block 0; no L1-norm parameter is decayed
    assert float(m.bn1.weight.detach().sum()) == 8.0 and float(m.layer1[0].bn3.weight.detach().abs().sum()) == 0.0
    flt = m.regime[0]['regularizer']['filter']['module']
    assert not flt(m.bn1) and not flt(m.layer2[0].downsample[1]) and flt(m.conv1) and flt(m.fc)


def test_reference_layout_state_dict_loads_strictly():
    import convnet_amd as ca
    with open(os.path.join(GOLDEN, 'structure_l1.json')) as f:
        ref = json.load(f)['18']
    g = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(*s, generator=g) for k, s in zip(ref['keys'], ref['shapes'])}
    m = ca.models.resnet(depth=18, bn_norm='L1')
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.layer3[1].bn2.running_var, sd['layer3.1.bn2.running_var'])
    assert torch.equal(m.layer3[0].downsample[1].bias, sd['layer3.0.downsample.1.bias'])


def test_refusals():
    import convnet_amd as ca
    with pytest.raises(NotImplementedError, match='L1'):
        ca.models.resnet(depth=18, bn_norm='TopK')
    with pytest.raises(NotImplementedError):
        ca.models.resnet(depth=18, bn_norm='L1', quantize=True)
    with pytest.raises(NotImplementedError):
        ca.models.resnext(depth=50, bn_norm='L1')
    with pytest.raises(NotImplementedError):
        ca.nn.L1BatchNorm2d(8, noise=True)
    with pytest.raises(NotImplementedError):
        ca.nn.L1BatchNorm2d(8, normalized=False)
    model = ca.models.resnet(depth=18, bn_norm='L1', **SMALL)
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime),
                    device='cuda:0' if HAS_GPU else 'cpu', dtype=torch.float32, print_freq=10 ** 9)
    with pytest.raises(NotImplementedError):
        tr.calibrate_bn([(torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long))], num_steps=1)
    # --sync-bn leaves these modules alone (they are no BatchNorm2d), as in the reference
    ca.nn.convert_sync_batchnorm(model)
    assert not any(hasattr(x, 'sync_group') for x in model.modules() if isinstance(x, ca.nn.L1BatchNorm2d))


# ---- trajectories --------------------------------------------------------------------------------------------------------

WARM_SEED = 977     # == tools/make_golden_l1bn.py


def warm_l1_state(model, seed):
    """tools/make_golden_l1bn.py:warm_l1_state restated for the engine's model (same module order): gamma ~ U(0.5, 1.5) for
    every L1 norm - the last one of every block included -, beta ~ N(0, 0.1), running buffers zeroed (they are then set by
    one seeded training-mode forward, _warm_running)."""
    import convnet_amd as ca
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, m in model.named_modules():
            if isinstance(m, ca.nn.L1BatchNorm2d):
                C = m.weight.numel()
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_mean.zero_()
                m.running_var.zero_()


def _warm_running(tr, meta):
    x = torch.randn(meta['B'], 3, meta['size'], meta['size'], generator=torch.Generator().manual_seed(meta['l1_warm_seed'] + 1))
    tr.model.train()
    with torch.no_grad():
        tr.model(x.to(tr.device))


def _run(meta, dtype, device, steps=None, graph=False, grads_after_step0=None, graph_mode=None):
    """helpers.run_engine_trajectory with the L1 warm recipe (meta['l1_warm_seed']) and an optional forced graph mode."""
    import convnet_amd as ca
    torch.manual_seed(123)
    model = ca.models.resnet(dataset='imagenet', **dict(meta['model_kw']))
    if meta.get('l1_warm_seed') is not None:
        warm_l1_state(model, meta['l1_warm_seed'])
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(device), dtype=dtype,
                    loss_scale=meta['loss_scale'], grad_clip=meta['grad_clip'], print_freq=10 ** 9)
    if graph_mode is not None:
        tr._graph_mode = graph_mode
        tr._use_graph = graph_mode != '0'
    elif not graph:
        tr._use_graph = False
    if meta.get('l1_warm_seed') is not None:
        _warm_running(tr, meta)
    data = golden_batches(meta)
    if steps is not None:
        data = data[:steps]
    recs = []
    for i, (x, t) in enumerate(data):
        r = tr.train([(x, t)], chunk_batch=meta['chunk_batch'])
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
        if i == 0 and grads_after_step0 is not None:   # zero_grad runs at the START of a step: these are step 0's
            params = dict(model.named_parameters())
            for k in list(grads_after_step0):
                grads_after_step0[k] = sample_tensor(params[k].grad, k)
    return recs, tr, model, data


def _load(tag):
    meta, final = load_traj(tag)
    assert meta['model_kw']['bn_norm'] == 'L1' and 'num_batches_tracked' not in meta
    return meta, final


def _check_fp32(meta, final, recs, tr, model, data, wtol):
    """test_resnext.py:_check_fp32 minus its num_batches_tracked line (this norm has no such buffer)."""
    for r, g in zip(recs, meta['records']):
        assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
        assert r['prec1'] == g['prec1'] and r['prec5'] == g['prec5']
        assert r['grad'] == pytest.approx(g['grad'], rel=1e-3)
    if len(recs) == meta['steps']:
        sd = model.state_dict()
        for k, v in final.items():
            assert rel_l2(sd[k].float().cpu(), v) < wtol, k
        val = tr.validate(data[:2])
        assert val['loss'] == pytest.approx(meta['validate']['loss'], rel=1e-3)
        assert val['prec1'] == meta['validate']['prec1'] and val['prec5'] == meta['validate']['prec5']


def _check_bf16(meta, recs):
    """test_resnext.py:_check_bf16: loss abs 2e-2 at step 0 / 5e-2 later, prec within one sample, grad-norm rel 5e-2 at
    step 0 / 1.5e-1 later."""
    B = meta['B']
    for i, (r, g) in enumerate(zip(recs, meta['records'])):
        assert r['loss'] == pytest.approx(g['loss'], abs=2e-2 if i == 0 else 5e-2), i
        assert abs(r['prec1'] - g['prec1']) <= 100.0 / B + 1e-6
        assert abs(r['prec5'] - g['prec5']) <= 100.0 / B + 1e-6
        assert r['grad'] == pytest.approx(g['grad'], rel=5e-2 if i == 0 else 1.5e-1), i


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('tag', ['r50s_l1', 'r18s_l1', 'rx18s_l1'])
def test_fp32_trajectory_small(mode, tag):
    """r50s_l1: one step on the emulator (every step on the GPU); r18s_l1 and rx18s_l1 (grouped 3x3 convolutions AND L1
    norms: both no-fusion operators): every step on both."""
    dev = _dev(mode)
    meta, final = _load(tag)
    steps = 1 if (mode == 'emul' and tag == 'r50s_l1') else None
    recs, tr, model, data = _run(meta, torch.float32, dev, steps)
    assert len(recs) == (meta['steps'] if steps is None else steps)
    print(tag, [(r['loss'], g['loss'], r['grad'], g['grad']) for r, g in zip(recs, meta['records'])])
    _check_fp32(meta, final, recs, tr, model, data, 1e-4)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('tag', ['r50s_l1', 'r18s_l1'])
def test_16bit_trajectory_small(mode, dtype, tag):
    """The first two steps (one on the emulator): the rx50s precedent of test_resnext.py - the loss of this 8-image
    trajectory rises as well."""
    dev = _dev(mode)
    meta, _ = _load(tag)
    recs, tr, model, data = _run(meta, dtype, dev, 1 if mode == 'emul' else 2, graph=True)
    print(tag, dtype, [(r['loss'], g['loss'], r['grad'], g['grad']) for r, g in zip(recs, meta['records'])])
    _check_bf16(meta, recs)


def _branch_norm_params(names):
    """The parameters of the norms INSIDE the residual branches (bn1 / bn2 of every bottleneck block): with the cold
    init (last gamma of every block 0) no gradient reaches them at step 0."""
    b = [k for k in names if k.startswith('layer') and ('.bn1.' in k or '.bn2.' in k)]
    assert len(b) == 16 * 2 * 2
    return b


def test_warm_fixture_exercises_the_branch_norms():
    meta, tens = load_warm('r50s_l1_warm')
    assert meta['reference_dtype'] == 'float64' and meta['l1_warm_seed'] == WARM_SEED
    norms = meta['grad0_norms']
    assert len(norms) == 161 and set(norms) == set(tens['grad0'])      # every parameter
    for k in _branch_norm_params(norms):
        assert norms[k] > 0 and norms[k] > 1e-5 * max(norms.values()), k


@pytest.mark.parametrize('mode', MODES)
def test_fp32_warm_step0_gradients(mode):
    """fp32 engine against the float64 reference on the warm fixture, the step-0 gradient of every parameter: norm rel
    5e-3 and sampled rel-L2 5e-3 (test_resnext.py's bounds for its warm fixture)."""
    dev = _dev(mode)
    meta, tens = load_warm('r50s_l1_warm')
    grads = {k: None for k in tens['grad0']}
    recs, tr, model, data = _run(meta, torch.float32, dev, 1, grads_after_step0=grads)
    r, g = recs[0], meta['records'][0]
    errs = {k: (abs(grads[k][0] - gold['norm']) / gold['norm'], rel_l2(grads[k][1], gold['val']))
            for k, gold in tens['grad0'].items()}
    worst = sorted(errs.items(), key=lambda kv: -max(kv[1]))[:4]
    print('warm step 0: loss %.6f (ref %.6f), grad norm %.5f (ref %.5f); worst (norm rel, sampled rel-L2): %s'
          % (r['loss'], g['loss'], r['grad'], g['grad'], [(k, '%.2e' % a, '%.2e' % b) for k, (a, b) in worst]))
    assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
    assert r['grad'] == pytest.approx(g['grad'], rel=5e-3)
    for k, gold in tens['grad0'].items():
        assert gold['norm'] > 0, k
        assert errs[k][0] < 5e-3, (k, grads[k][0], gold['norm'])
        assert errs[k][1] < 5e-3, (k, errs[k][1])


@pytest.mark.gpu
def test_plan_is_bit_identical_to_eager():
    """The 4 steps of r50s_l1 with the launch plan forced from the third step on against eager launches: the same
    per-step records, a bit-identical final state dict, and the plan really ran."""
    dev = _dev('gpu')
    meta, _ = _load('r50s_l1')
    outs = []
    for mode in ('0', '1'):
        recs, tr, model, data = _run(meta, torch.float32, dev, graph_mode=mode)
        torch.cuda.synchronize()
        if mode == '1':    # the later steps really ran as a recorded plan (not an eager fall-back compared with eager)
            assert any(g['graph'] is not None for g in tr._gstates.values()), 'the step was never captured'
            assert any(g['graph'] is not None and g['graph'].get('plan') is not None for g in tr._gstates.values())
        else:
            assert all(g['graph'] is None for g in tr._gstates.values())
        outs.append((recs, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()
                            if v.dtype.is_floating_point}))
    assert outs[0][0] == outs[1][0]
    assert len(outs[0][1]) == 267
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize('mode', MODES)
def test_cli_train_checkpoint_resume(mode, tmp_path):
    dev = _dev(mode)
    from convnet_amd.main import main
    cfg = "{'depth': 18, 'bn_norm': 'L1', 'inplanes': 8, 'width': [8, 16, 32, 64], 'num_classes': 16}"
    common = ['--model', 'resnet', '--model-config', cfg, '--input-size', '32', '-b', '4', '--device',
              'cuda' if dev.type == 'cuda' else 'cpu', '--steps-per-epoch', '2', '--val-steps', '1',
              '--results-dir', str(tmp_path), '--print-freq', '1']
    out = main(common + ['--save', 'run', '--epochs', '1'])
    run = tmp_path / 'run'
    ck = torch.load(run / 'checkpoint.pth.tar', map_location='cpu')
    assert ck['epoch'] == 1 and ck['model'] == 'resnet'
    sd = ck['state_dict']
    assert [k for k in sd if k.startswith('bn1.')] == ['bn1.bias', 'bn1.weight', 'bn1.running_mean', 'bn1.running_var']
    assert float(sd['bn1.running_var'].abs().sum()) > 0      # the scale buffer left 0 after two training steps
    assert set(out['train']) >= {'loss', 'prec1', 'prec5'} and out['train']['loss'] == out['train']['loss']
    main(common + ['--save', 'run2', '--epochs', '2', '--resume', str(run / 'checkpoint.pth.tar')])
    ck2 = torch.load(tmp_path / 'run2' / 'checkpoint.pth.tar', map_location='cpu')
    assert ck2['epoch'] == 2
    assert not torch.equal(ck2['state_dict']['bn1.running_var'], sd['bn1.running_var'])
