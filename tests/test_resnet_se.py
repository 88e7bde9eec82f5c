"""models.resnet_se (one shared nn.SEBlock per stage on the SHORTCUT of every block, csrc/se.hip) against the reference.

  * structure: keys in order (alias keys of the shared module included) / shapes / parameter counts / named_parameters
    against tests/golden/structure_se.json (written by tools/make_golden_se.py from the reference), the module object
    shared within a stage, one arena slot per unique parameter, seeded construction, a reference-layout state dict;
  * trajectories: tests/golden/traj_r50s_se / r18s_se / rx18s_se (the reference Trainer, fp32 CPU) with test_resnet_l1.py's
    bounds (fp32: loss abs 1e-4, grad-norm rel 1e-3, prec identical, final tensors rel-L2 1e-4, validate loss rel 1e-3;
    bf16 / f16: _check_bf16's bounds on the first two steps);
  * warm start: tests/golden/traj_r50s_se_warm (reference in float64, helpers.warm_bn_state: branch AND gated shortcut
    carry signal): the step-0 gradient of EVERY unique parameter, norm and sampled rel-L2 within 5e-3.  The SE parameters'
    gradient is the sum over the blocks of a stage of a gate on the shortcut: a per-block SE, or an SE on the branch (the
    textbook placement), cannot meet it;
  * no junction fusion is wired in an SE model, the default model keeps them;
  * plan == eager on the GPU, and the CLI (train, checkpoint, resume)."""
import json
import os

import pytest
import torch

from conftest import HAS_GPU
from helpers import GOLDEN, golden_batches, load_traj, load_warm, rel_l2, sample_tensor, tensor_sums, warm_bn_state

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
SMALL = dict(width=[8, 16, 32, 64], inplanes=8, num_classes=16)
SE_NAMES = ['transform.0.weight', 'transform.0.bias', 'transform.2.weight', 'transform.2.bias']


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _structure(depth):
    with open(os.path.join(GOLDEN, 'structure_se.json')) as f:
        return json.load(f)[str(depth)]


# ---- structure ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('depth', [18, 50])
def test_structure_matches_reference(depth):
    import convnet_amd as ca
    ref = _structure(depth)
    m = ca.models.resnet_se(depth=depth)
    sd = m.state_dict()
    assert list(sd.keys()) == ref['keys']
    assert [list(v.shape) for v in sd.values()] == ref['shapes']
    assert sum(p.numel() for p in m.parameters()) == ref['n_params']
    assert [k for k, _ in m.named_parameters()] == ref['named_parameters']
    if depth == 50:
        assert ref['n_params'] == 26257432 and len(sd) == 384 and len(ref['named_parameters']) == 177
    # ONE module per stage, the same object in every block; every block lists its alias keys, named_parameters the first
    for s, nblocks in zip((1, 2, 3, 4), (2, 2, 2, 2) if depth == 18 else (3, 4, 6, 3)):
        stage = getattr(m, 'layer%d' % s)
        assert len(stage) == nblocks and isinstance(stage[0].residual_block, ca.nn.SEBlock)
        for b in range(nblocks):
            assert stage[b].residual_block is stage[0].residual_block
            for n in SE_NAMES:
                k = 'layer%d.%d.residual_block.%s' % (s, b, n)
                assert k in sd and sd[k].data_ptr() == sd['layer%d.0.residual_block.%s' % (s, n)].data_ptr()
                assert (k in ref['named_parameters']) == (b == 0)
    assert m.layer1[0].residual_block is not m.layer2[0].residual_block
    assert 'resnet_se' in ca.models.__dict__ and 'resnet_se' in __import__('convnet_amd.main', fromlist=['x']).model_names


@pytest.mark.parametrize('mode', MODES)
def test_one_arena_slot_per_unique_parameter(mode):
    dev = _dev(mode)
    import convnet_amd as ca
    m = ca.models.resnet_se(depth=50, **SMALL)
    arena = ca.engine.prepare(m, dev, torch.float32)
    names = [k for k, _ in m.named_parameters()]
    assert len(arena.slots) == len(names) == 177
    assert sorted(s.name for s in arena.slots) == sorted(names)
    assert len({s.offset for s in arena.slots}) == 177
    se = m.layer3[0].residual_block
    for b in m.layer3:      # every block of the stage reads and accumulates into the same segments
        assert b.residual_block.transform[0].master_view('weight').data_ptr() == se.transform[0].master_view('weight').data_ptr()
    assert sum(s.numel for s in arena.slots) == 389654
    # the weight-decay run of a shared parameter comes from the filter on its first name
    opt = ca.OptimRegime(m, m.regime)
    flt = m.regime[0]['regularizer']['filter']
    for s in arena.slots:
        if 'residual_block' in s.name:
            assert '.0.residual_block.transform.' in s.name
            assert flt['module'](s.module) and flt['parameter_name'](s.name) == s.name.endswith('weight')
    del opt


def test_seeded_construction_and_weight_decay_filter():
    import convnet_amd as ca
    meta, _ = load_traj('r50s_se')
    torch.manual_seed(123)
    m = ca.models.resnet_se(dataset='imagenet', **meta['model_kw'])
    sums = tensor_sums(m.state_dict())
    assert set(sums) == set(meta['init_sums'])
    for k, (s, a) in meta['init_sums'].items():      # pins the draw order: the stage's SE behind its downsample
        assert sums[k][0] == pytest.approx(s, rel=1e-6, abs=1e-6), k
        assert sums[k][1] == pytest.approx(a, rel=1e-6, abs=1e-6), k
    assert sum(p.numel() for p in m.parameters()) == meta['n_params'] == 389654 and len(m.state_dict()) == meta['n_keys'] == 384
    # init_model leaves the two dense layers at torch's default initialisation
    assert float(m.layer1[0].residual_block.transform[2].bias.detach().abs().sum()) > 0
    flt = m.regime[0]['regularizer']['filter']
    se = m.layer2[0].residual_block
    assert flt['module'](se.transform[0]) and flt['module'](se.transform[2]) and not flt['module'](m.bn1)
    assert flt['parameter_name']('layer2.0.residual_block.transform.0.weight')
    assert not flt['parameter_name']('layer2.0.residual_block.transform.0.bias')


def test_reference_layout_state_dict_loads_strictly():
    import convnet_amd as ca
    ref = _structure(18)
    g = torch.Generator().manual_seed(3)
    sd = {}
    for k, s in zip(ref['keys'], ref['shapes']):
        first = k.split('.residual_block.')
        if len(first) == 2 and not first[0].endswith('.0'):      # an alias key holds the shared tensor's values
            sd[k] = sd[first[0].rsplit('.', 1)[0] + '.0.residual_block.' + first[1]]
        else:
            sd[k] = torch.randn(*s, generator=g) if s else torch.tensor(3)
    m = ca.models.resnet_se(depth=18)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.layer3[1].residual_block.transform[2].weight, sd['layer3.0.residual_block.transform.2.weight'])
    assert torch.equal(m.layer3[1].bn2.running_var, sd['layer3.1.bn2.running_var'])
    missing = dict(sd)
    del missing['layer2.1.residual_block.transform.0.bias']
    with pytest.raises(RuntimeError):
        m.load_state_dict(missing, strict=True)


def test_no_junction_fusion_is_wired():
    """In an SE model the junction reads the GATED shortcut: no block carries a ResGradHolder, conv1 / the projection reduce
    no BatchNorm across the block boundary, no junction is left lazy for the next conv1; the fusions inside the branch
    stay.  The default model keeps every one of them."""
    import convnet_amd as ca
    for kw in (dict(depth=50), dict(depth=18), dict(depth=50, groups=[2, 2, 2, 2])):
        m = ca.models.resnet_se(**SMALL, **kw) if kw['depth'] == 50 else \
            ca.models.resnet_se(depth=18, width=[16, 32, 64, 128], inplanes=16, num_classes=16)
        blocks = [x for x in m.modules() if type(x).__name__ == 'ResidualBlock']
        assert blocks
        for b in blocks:
            assert b._holder is None and b.gated
            assert 'input_bn' not in b.conv1.__dict__ and '_res_holder' not in b.conv1.__dict__
            assert 'junction_conv1' not in b.conv1.__dict__
            assert 'consumer_conv' not in b.last_bn().__dict__ and '_res_holder' not in b.last_bn().__dict__
            if b.downsample is not None:
                assert 'input_bn' not in b.downsample[0].__dict__ and '_res_holder' not in b.downsample[0].__dict__
        for x in m.modules():
            assert 'consumer_conv' not in x.__dict__ and '_res_holder' not in x.__dict__ and 'junction_conv1' not in x.__dict__
        if kw == dict(depth=50):     # inside the branch: statistics from the epilogue, the inner BatchNorm's backward sums
            assert m.layer1[0].conv3.feeds_batchnorm and 'input_bn' in m.layer1[0].conv2.__dict__
    d = ca.models.resnet(depth=50, **SMALL)
    b0, b1 = d.layer1[0], d.layer1[1]
    assert b0._holder is not None and not b0.gated and b0.residual_block is None
    assert b0.conv1.__dict__.get('junction_conv1') and b0.conv1._res_holder is b0._holder
    assert b0.downsample[0]._res_holder is b0._holder and b1.last_bn()._res_holder is b1._holder
    assert b1.conv1.__dict__['input_bn'] is b0.last_bn() and b0.last_bn().__dict__['consumer_conv'] is b1.conv1
    assert d.layer2[0].downsample[0].__dict__['input_bn'] is d.layer1[2].last_bn()
    assert 'residual_block' not in ''.join(d.state_dict().keys())


def test_refusals():
    import convnet_amd as ca
    with pytest.raises(NotImplementedError):
        ca.models.resnet_se(depth=18, quantize=True)
    with pytest.raises(NotImplementedError):
        ca.models.resnet_se(depth=18, bn_norm='L1')
    with pytest.raises(NotImplementedError):
        ca.models.resnet_se(depth=18, dataset='cifar10')
    with pytest.raises(NotImplementedError):      # 8 // 16 == 0 hidden units: the basic-block small model of width 8
        ca.models.resnet_se(depth=18, **SMALL)
    with pytest.raises(NotImplementedError):
        ca.models.resnet(depth=18, residual_block=ca.nn.SEBlock, quantize=True)


# ---- trajectories --------------------------------------------------------------------------------------------------------

def _run(meta, dtype, device, steps=None, graph=False, grads_after_step0=None, graph_mode=None):
    """helpers.run_engine_trajectory on models.resnet_se, with an optional forced graph mode."""
    import convnet_amd as ca
    torch.manual_seed(123)
    model = ca.models.resnet_se(dataset='imagenet', **dict(meta['model_kw']))
    if meta.get('warm_seed') is not None:
        warm_bn_state(model, meta['warm_seed'], last_gamma=tuple(meta['warm_last_gamma']))
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(device), dtype=dtype,
                    loss_scale=meta['loss_scale'], grad_clip=meta['grad_clip'], print_freq=10 ** 9)
    if graph_mode is not None:
        tr._graph_mode = graph_mode
        tr._use_graph = graph_mode != '0'
    elif not graph:
        tr._use_graph = False
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


def _check_fp32(meta, final, recs, tr, model, data, wtol):
    """test_resnet_l1.py:_check_fp32, plus num_batches_tracked (these are BatchNorm2d)."""
    for r, g in zip(recs, meta['records']):
        assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
        assert r['prec1'] == g['prec1'] and r['prec5'] == g['prec5']
        assert r['grad'] == pytest.approx(g['grad'], rel=1e-3)
    if len(recs) == meta['steps']:
        sd = model.state_dict()
        assert any('residual_block' in k for k in final)
        for k, v in final.items():
            assert rel_l2(sd[k].float().cpu(), v) < wtol, k
        assert int(sd['bn1.num_batches_tracked']) == meta['num_batches_tracked']
        val = tr.validate(data[:2])
        assert val['loss'] == pytest.approx(meta['validate']['loss'], rel=1e-3)
        assert val['prec1'] == meta['validate']['prec1'] and val['prec5'] == meta['validate']['prec5']


def _check_bf16(meta, recs):
    """test_resnet_l1.py:_check_bf16: loss abs 2e-2 at step 0 / 5e-2 later, prec within one sample, grad-norm rel 5e-2 at
    step 0 / 1.5e-1 later."""
    B = meta['B']
    for i, (r, g) in enumerate(zip(recs, meta['records'])):
        assert r['loss'] == pytest.approx(g['loss'], abs=2e-2 if i == 0 else 5e-2), i
        assert abs(r['prec1'] - g['prec1']) <= 100.0 / B + 1e-6
        assert abs(r['prec5'] - g['prec5']) <= 100.0 / B + 1e-6
        assert r['grad'] == pytest.approx(g['grad'], rel=5e-2 if i == 0 else 1.5e-1), i


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('tag', ['r50s_se', 'r18s_se', 'rx18s_se'])
def test_fp32_trajectory_small(mode, tag):
    """r50s_se: one step on the emulator (every step on the GPU); r18s_se (hidden widths 1, 2, 4, 8; layer1 has no
    projection: its first block gates a post-ReLU input) and rx18s_se (grouped 3x3 convolutions): every step on both."""
    dev = _dev(mode)
    meta, final = load_traj(tag)
    steps = 1 if (mode == 'emul' and tag == 'r50s_se') else None
    recs, tr, model, data = _run(meta, torch.float32, dev, steps)
    assert len(recs) == (meta['steps'] if steps is None else steps)
    print(tag, [(r['loss'], g['loss'], r['grad'], g['grad']) for r, g in zip(recs, meta['records'])])
    _check_fp32(meta, final, recs, tr, model, data, 1e-4)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('tag', ['r50s_se', 'r18s_se'])
def test_16bit_trajectory_small(mode, dtype, tag):
    """The first two steps (one on the emulator)."""
    dev = _dev(mode)
    meta, _ = load_traj(tag)
    recs, tr, model, data = _run(meta, dtype, dev, 1 if mode == 'emul' else 2, graph=True)
    print(tag, dtype, [(r['loss'], g['loss'], r['grad'], g['grad']) for r, g in zip(recs, meta['records'])])
    _check_bf16(meta, recs)


# ---- warm start: step-0 gradients ------------------------------------------------------------------------------------------

_WARM = {}


def _warm_step0(mode):
    """One fp32 step on the warm fixture per mode, shared by the two tests below (nothing in it is modified later)."""
    if mode not in _WARM:
        dev = _dev(mode)
        meta, tens = load_warm('r50s_se_warm')
        grads = {k: None for k in tens['grad0']}
        recs, tr, model, data = _run(meta, torch.float32, dev, 1, grads_after_step0=grads)
        errs = {k: (abs(grads[k][0] - gold['norm']) / gold['norm'], rel_l2(grads[k][1], gold['val']))
                for k, gold in tens['grad0'].items()}
        _WARM[mode] = (meta, tens, grads, recs, errs)
    return _WARM[mode]


def test_warm_fixture_covers_every_unique_parameter():
    meta, tens = load_warm('r50s_se_warm')
    assert meta['reference_dtype'] == 'float64' and meta['warm_seed'] == 977
    norms = meta['grad0_norms']
    assert len(norms) == 177 and set(norms) == set(tens['grad0'])
    se = [k for k in norms if 'residual_block' in k]
    assert len(se) == 16 and all('.0.residual_block.' in k for k in se)
    for k in se:      # the gated shortcut carries signal into every SE parameter
        assert norms[k] > 1e-5 * max(norms.values()), k
    # ... and the branch too (last gammas non-zero)
    assert norms['layer1.1.conv2.weight'] > 1e-4 * max(norms.values())


@pytest.mark.parametrize('mode', MODES)
def test_se_gradients_are_shared_over_the_stage_and_sit_on_the_shortcut(mode):
    """The step-0 gradient of each stage's SE parameters against the float64 reference: norm rel 5e-3, sampled rel-L2 5e-3.
    The reference sums it over the blocks of the stage (3, 4, 6, 3) through ONE gate on the shortcut."""
    _dev(mode)
    meta, tens, grads, recs, errs = _warm_step0(mode)
    se = sorted(k for k in tens['grad0'] if 'residual_block' in k)
    print('SE step-0 gradients (norm rel, sampled rel-L2):', [(k, '%.2e' % errs[k][0], '%.2e' % errs[k][1]) for k in se])
    assert len(se) == 16
    for k in se:
        assert tens['grad0'][k]['norm'] > 0
        assert errs[k][0] < 5e-3, (k, grads[k][0], tens['grad0'][k]['norm'])
        assert errs[k][1] < 5e-3, (k, errs[k][1])


@pytest.mark.parametrize('mode', MODES)
def test_fp32_warm_step0_gradients(mode):
    """fp32 engine against the float64 reference on the warm fixture, the step-0 gradient of every unique parameter: norm
    rel 5e-3 and sampled rel-L2 5e-3."""
    _dev(mode)
    meta, tens, grads, recs, errs = _warm_step0(mode)
    r, g = recs[0], meta['records'][0]
    worst = sorted(errs.items(), key=lambda kv: -max(kv[1]))[:4]
    print('warm step 0: loss %.6f (ref %.6f), grad norm %.5f (ref %.5f); worst (norm rel, sampled rel-L2): %s'
          % (r['loss'], g['loss'], r['grad'], g['grad'], [(k, '%.2e' % a, '%.2e' % b) for k, (a, b) in worst]))
    assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
    assert r['grad'] == pytest.approx(g['grad'], rel=5e-3)
    for k, gold in tens['grad0'].items():
        assert gold['norm'] > 0, k
        assert errs[k][0] < 5e-3, (k, grads[k][0], gold['norm'])
        assert errs[k][1] < 5e-3, (k, errs[k][1])


# ---- plan, CLI ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_plan_is_bit_identical_to_eager():
    """The 4 steps of r50s_se with the launch plan forced from the third step on against eager launches: the same
    per-step records, a bit-identical final state dict, and the plan really ran."""
    dev = _dev('gpu')
    meta, _ = load_traj('r50s_se')
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
    assert len(outs[0][1]) == 384 - 53
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize('mode', MODES)
def test_cli_train_checkpoint_resume(mode, tmp_path):
    dev = _dev(mode)
    from convnet_amd.main import main
    cfg = "{'depth': 18, 'inplanes': 16, 'width': [16, 32, 64, 128], 'num_classes': 16}"
    common = ['--model', 'resnet_se', '--model-config', cfg, '--input-size', '32', '-b', '4', '--device',
              'cuda' if dev.type == 'cuda' else 'cpu', '--steps-per-epoch', '2', '--val-steps', '1',
              '--results-dir', str(tmp_path), '--print-freq', '1']
    out = main(common + ['--save', 'run', '--epochs', '1'])
    run = tmp_path / 'run'
    ck = torch.load(run / 'checkpoint.pth.tar', map_location='cpu')
    assert ck['epoch'] == 1 and ck['model'] == 'resnet_se'
    sd = ck['state_dict']
    assert list(sd.keys()) == [k for k in _structure(18)['keys']]      # the reference layout, alias keys included
    for n in SE_NAMES:
        assert torch.equal(sd['layer2.1.residual_block.' + n], sd['layer2.0.residual_block.' + n])
    assert set(out['train']) >= {'loss', 'prec1', 'prec5'} and out['train']['loss'] == out['train']['loss']
    main(common + ['--save', 'run2', '--epochs', '2', '--resume', str(run / 'checkpoint.pth.tar')])
    ck2 = torch.load(tmp_path / 'run2' / 'checkpoint.pth.tar', map_location='cpu')
    assert ck2['epoch'] == 2
    for s in (1, 2, 3, 4):      # the SE weights of every stage moved between the two checkpoints
        for n in SE_NAMES:
            k = 'layer%d.0.residual_block.%s' % (s, n)
            assert not torch.equal(ck2['state_dict'][k], sd[k]), k
