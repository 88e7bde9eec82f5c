"""Duplicates ("batch augmentation") from the averaging kernels up to the CLI.

  * cn_avg_duplicates_fwd / _bwd (csrc/loss.hip, ops.average_duplicates): bit-identical to torch's CPU mean / to dy / D on
    exactly summable data, fp32 and bf16 gradients;
  * Trainer on B x D x C x H x W batches against tests/golden/traj_r18s_dup / traj_r18s_dup_chunk2 (written by
    tools/make_golden_dup.py from the unmodified reference Trainer, fp32 CPU) with test_resnet_l1.py's bounds (fp32: loss
    abs 1e-4, grad-norm rel 1e-3, prec identical, final tensors rel-L2 1e-4, validate loss rel 1e-3 with prec identical for
    both average_output settings; bf16: _check_bf16's bounds on the first two steps, one on the emulator);
  * 5-D training == training on the same data flattened by hand (bit-identical state dict), plan == eager on the GPU;
  * the CLI (--duplicates with synthetic data and an image folder, --device-resize, --chunk-batch, --evaluate --avg-out
    --augment) and the refusals that remain."""
import numpy as np
import pytest
import torch

from conftest import HAS_GPU
from helpers import load_traj, rel_l2

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
SMALL_CFG = "{'depth': 18, 'inplanes': 8, 'width': [8, 16, 32, 64], 'num_classes': %d}"


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


# ---- average over duplicates -----------------------------------------------------------------------------------------

AVG_SHAPES = [(1, 2, 1), (3, 3, 10), (2, 4, 1000), (5, 5, 1037)]


def _exact(shape, seed):
    """Integers in [-64, 64) / 8: every partial sum over D <= 5 of them is exact in fp32."""
    return torch.randint(-64, 64, shape, generator=torch.Generator().manual_seed(seed)).float() / 8


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B,D,K', AVG_SHAPES)
def test_average_duplicates_forward_is_torchs_mean(mode, B, D, K):
    import convnet_amd as ca
    dev = _dev(mode)
    x = _exact((B * D, K), 100 + K)
    want = x.view(B, D, K).mean(1)
    got = ca.ops.average_duplicates(x.to(dev), D)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, K)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('gdtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('B,D,K', AVG_SHAPES)
def test_average_duplicates_backward_is_dy_over_d(mode, gdtype, B, D, K):
    import convnet_amd as ca
    dev = _dev(mode)
    dy = _exact((B, K), 200 + K)
    want = (dy / D).view(B, 1, K).expand(B, D, K).reshape(B * D, K).to(gdtype)     # the fp32 quotient, rounded once
    got = ca.ops.average_duplicates_bwd(dy.to(dev), D, gdtype)
    assert got.dtype == gdtype and torch.equal(got.cpu(), want)
    if gdtype == torch.float32:      # ... and through autograd
        x = _exact((B * D, K), 300 + K).to(dev).requires_grad_(True)
        ca.ops.average_duplicates(x, D).backward(dy.to(dev))
        assert torch.equal(x.grad.cpu(), want)


def test_average_duplicates_argument_checks():
    import convnet_amd as ca
    dev = torch.device('cuda', 0) if HAS_GPU else torch.device('cpu')
    Err = ca._lib.ConvNetHipError
    with pytest.raises(Err):
        ca.ops.average_duplicates(torch.zeros(5, 4, device=dev), 2)           # 5 rows do not divide by 2
    with pytest.raises(Err):
        ca.ops.average_duplicates(torch.zeros(4, 4, device=dev).bfloat16(), 2)
    L = ca._lib.load()
    with pytest.raises(Err, match='null operand'):
        L.cn_avg_duplicates_fwd(None, None, 1, 2, 3, None)
    with pytest.raises(Err, match='bad shape'):
        L.cn_avg_duplicates_bwd(ca._lib.ptr(torch.zeros(4, device=dev)), ca._lib.ptr(torch.zeros(8, device=dev)), 0, 2, 0, 2, None)


# ---- trainer against the reference -------------------------------------------------------------------------------------

def dup_batches(meta):
    """tools/make_golden_dup.py:dup_batches restated (seeds 61 / 62 of the two fixtures travel in meta['seed'])."""
    g = torch.Generator().manual_seed(meta['seed'])
    data = [(torch.randn(meta['B'], meta['D'], 3, meta['size'], meta['size'], generator=g),
             torch.randint(0, meta['classes'], (meta['B'],), generator=g)) for _ in range(meta['steps'])]
    for (x, t), (sx, st) in zip(data, meta['input_sums']):
        assert abs(float(x.double().sum()) - sx) < 1e-6 * max(1.0, abs(sx)) and float(t.sum()) == st
    return data


def _load(tag):
    meta, final = load_traj(tag)
    assert meta['D'] == 2 and meta['B'] == 4 and meta['steps'] == 3 and meta['model_kw']['depth'] == 18
    assert meta['seed'] == {'r18s_dup': 61, 'r18s_dup_chunk2': 62}[tag]
    assert meta['chunk_batch'] == {'r18s_dup': 1, 'r18s_dup_chunk2': 2}[tag]
    ref, _ = load_traj('r18s')
    assert (meta['grad_clip'], meta['loss_scale']) == (ref['grad_clip'], ref['loss_scale'])
    assert meta['avg_top_gap'] > 1e-4            # the reference's averaged prec values are not decided by a tie
    return meta, final


def _trainer(meta, dtype, device, graph_mode='0'):
    import convnet_amd as ca
    torch.manual_seed(123)
    model = ca.models.resnet(dataset='imagenet', **dict(meta['model_kw']))
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(device), dtype=dtype,
                    loss_scale=meta['loss_scale'], grad_clip=meta['grad_clip'], print_freq=10 ** 9)
    tr._graph_mode = graph_mode
    tr._use_graph = graph_mode != '0'
    return tr, model


def _train(tr, data, chunk_batch, to=None):
    recs = []
    for x, t in data:
        if to is not None:
            x, t = x.to(to), t.to(to)
        r = tr.train([(x, t)], chunk_batch=chunk_batch)
        recs.append({k: float(r[k]) for k in ('loss', 'prec1', 'prec5', 'grad')})
    return recs


def _state(model):
    return {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items() if v.dtype.is_floating_point}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('tag', ['r18s_dup', 'r18s_dup_chunk2'])
def test_fp32_trajectory_matches_the_reference(mode, tag):
    dev = _dev(mode)
    meta, final = _load(tag)
    tr, model = _trainer(meta, torch.float32, dev)
    data = dup_batches(meta)
    # r18s_dup_chunk2: one step on the emulator, every step on the GPU (test_resnet_l1.py's precedent for its slowest case)
    steps = 1 if (mode == 'emul' and tag == 'r18s_dup_chunk2') else meta['steps']
    recs = _train(tr, data[:steps], meta['chunk_batch'])
    print(tag, [(r['loss'], g['loss'], r['grad'], g['grad']) for r, g in zip(recs, meta['records'])])
    assert len(recs) == steps
    for r, g in zip(recs, meta['records']):
        assert r['loss'] == pytest.approx(g['loss'], abs=1e-4)
        assert r['prec1'] == g['prec1'] and r['prec5'] == g['prec5']
        assert r['grad'] == pytest.approx(g['grad'], rel=1e-3)
    if steps < meta['steps']:
        return
    sd = model.state_dict()
    for k, v in final.items():
        assert rel_l2(sd[k].float().cpu(), v) < 1e-4, k
    assert int(sd['bn1.num_batches_tracked']) == meta['num_batches_tracked']
    for avg, gold in ((False, meta['validate']), (True, meta['validate_avg'])):
        val = tr.validate(data[:2], average_output=avg)
        print(tag, 'validate average_output=%s' % avg, val['loss'], gold['loss'], val['prec1'], gold['prec1'])
        assert val['loss'] == pytest.approx(gold['loss'], rel=1e-3)
        assert val['prec1'] == gold['prec1'] and val['prec5'] == gold['prec5']


@pytest.mark.parametrize('mode', MODES)
def test_bf16_trajectory(mode):
    """test_resnet_l1.py:_check_bf16's bounds on the first two steps of traj_r18s_dup (one on the emulator); a batch is
    B * D = 8 rows."""
    dev = _dev(mode)
    meta, _ = _load('r18s_dup')
    tr, model = _trainer(meta, torch.bfloat16, dev, graph_mode='auto')
    recs = _train(tr, dup_batches(meta)[:1 if mode == 'emul' else 2], 1)
    print([(r['loss'], g['loss'], r['grad'], g['grad']) for r, g in zip(recs, meta['records'])])
    rows = meta['B'] * meta['D']
    for i, (r, g) in enumerate(zip(recs, meta['records'])):
        assert r['loss'] == pytest.approx(g['loss'], abs=2e-2 if i == 0 else 5e-2), i
        assert abs(r['prec1'] - g['prec1']) <= 100.0 / rows + 1e-6
        assert abs(r['prec5'] - g['prec5']) <= 100.0 / rows + 1e-6
        assert r['grad'] == pytest.approx(g['grad'], rel=5e-2 if i == 0 else 1.5e-1), i


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('chunk_batch', [1, 2])
def test_5d_training_equals_hand_flattened_4d(mode, chunk_batch):
    """Sample-major for chunk_batch = 1, view-major for chunk_batch = 2 (each chunk: one view of every sample)."""
    dev = _dev(mode)
    meta, _ = _load('r18s_dup')
    data = dup_batches(meta)[:2]
    if mode == 'emul':                     # (emulated threads are slow: one step on two samples, still two chunks of two rows)
        data = [(x[:2], t[:2]) for x, t in data[:1]]
    outs = []
    for flat in (False, True):
        tr, model = _trainer(meta, torch.float32, dev)
        if flat:
            D = meta['D']
            if chunk_batch == 1:
                d4 = [(x.reshape(-1, *x.shape[2:]), t.repeat_interleave(D)) for x, t in data]
            else:
                d4 = [(x.transpose(0, 1).reshape(-1, *x.shape[2:]), t.repeat(D)) for x, t in data]
            assert all(x.dim() == 4 and x.shape[0] == t.shape[0] == data[0][0].shape[0] * D for x, t in d4)
            recs = _train(tr, d4, chunk_batch)
        else:
            recs = _train(tr, data, chunk_batch)
        outs.append((recs, _state(model)))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize('mode', MODES)
def test_average_output_training_step(mode):
    """train(average_output=True): the loss is the criterion of the averaged output (B rows), the step is never captured,
    and the parameters move."""
    import convnet_amd as ca
    dev = _dev(mode)
    meta, _ = _load('r18s_dup')
    x, t = dup_batches(meta)[0]
    tr, model = _trainer(meta, torch.float32, dev, graph_mode='1')
    tr.model.train()
    with torch.no_grad():
        out = tr.model(x.flatten(0, 1).to(dev)).float().cpu()
    want = float(torch.nn.functional.cross_entropy(out.view(meta['B'], meta['D'], -1).mean(1), t))
    w0 = model.fc.weight.detach().float().cpu().clone()
    torch.manual_seed(123)
    tr2, model2 = _trainer(meta, torch.float32, dev, graph_mode='1')
    losses = [tr2.train([(x, t)], average_output=True)['loss'] for _ in range(1 if mode == 'emul' else 4)]
    assert losses[0] == pytest.approx(want, abs=1e-4)
    assert all(l == l for l in losses) and not tr2._gstates        # eager body every time
    assert not torch.equal(model2.fc.weight.detach().float().cpu(), w0)
    assert ca is not None


@pytest.mark.gpu
def test_plan_is_bit_identical_to_eager():
    """The steps of traj_r18s_dup on 5-D CUDA inputs with the launch plan forced against eager launches: the same records,
    a bit-identical final state dict, and a plan really ran."""
    dev = _dev('gpu')
    meta, _ = _load('r18s_dup')
    data = dup_batches(meta)
    data = data + data[:1]                 # (two eager warm-up steps, the capture, one replay)
    outs = []
    for mode in ('0', '1'):
        tr, model = _trainer(meta, torch.float32, dev, graph_mode=mode)
        recs = _train(tr, data, 1, to=dev)
        torch.cuda.synchronize()
        if mode == '1':
            assert any(g['graph'] is not None and g['graph'].get('plan') is not None for g in tr._gstates.values()), \
                'the step never ran as a recorded plan'
            assert all(k[0] == (meta['B'] * meta['D'], 3, meta['size'], meta['size']) for k in tr._gstates)
        else:
            assert all(g['graph'] is None for g in tr._gstates.values())
        outs.append((recs, _state(model)))
    assert outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


# ---- refusals that remain ----------------------------------------------------------------------------------------------

def test_refusals():
    import convnet_amd as ca
    dev = torch.device('cuda', 0) if HAS_GPU else torch.device('cpu')
    meta, _ = _load('r18s_dup')
    model = ca.models.resnet(dataset='imagenet', **dict(meta['model_kw']))
    with pytest.raises(NotImplementedError, match='adapt_grad_norm'):
        ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(dev), adapt_grad_norm=4)
    tr, _ = _trainer(meta, torch.float32, dev)
    x, t = dup_batches(meta)[0]
    with pytest.raises(NotImplementedError, match='different samples'):
        tr.train([(x, t)], average_output=True, chunk_batch=2)
    with pytest.raises(ValueError, match='duplicates dimension'):
        tr.validate([(x[:, 0], t)], average_output=True)


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def _folder(root, classes=2, per_class=2):
    PIL = pytest.importorskip('PIL')
    from PIL import Image
    assert PIL is not None
    rng = np.random.RandomState(4)
    for split in ('train', 'val'):
        for c in range(classes):
            d = root / 'imagenet' / split / ('c%d' % c)
            d.mkdir(parents=True)
            for i in range(per_class):
                a = (rng.rand(48 + 9 * i, 70 - 7 * c, 3) * 255).astype(np.uint8)
                Image.fromarray(a).save(str(d / ('%d.png' % i)))
    return root


def _cli(dev, tmp_path, classes, extra):
    return ['--model', 'resnet', '--model-config', SMALL_CFG % classes, '--input-size', '32', '-b', '2', '--device',
            'cuda' if dev.type == 'cuda' else 'cpu', '--results-dir', str(tmp_path / 'results'), '--print-freq', '1',
            '--epochs', '1', '--duplicates', '2'] + extra


def _finite(res):
    return all(res[k] == res[k] and abs(res[k]) != float('inf') for k in ('loss', 'prec1', 'prec5'))


@pytest.mark.parametrize('mode', MODES)
def test_cli_trains_with_duplicates_on_synthetic_data(mode, tmp_path):
    from convnet_amd.main import main, SyntheticLoader
    dev = _dev(mode)
    x, t = next(iter(SyntheticLoader(1, 4, 32, 16, 3, 1, duplicates=2)))
    assert tuple(x.shape) == (4, 2, 3, 32, 32) and tuple(t.shape) == (4,)
    x1, _ = next(iter(SyntheticLoader(1, 4, 32, 16, 3, 1)))
    g = torch.Generator().manual_seed(1)
    assert torch.equal(x1, torch.randn(4, 3, 32, 32, generator=g))         # D = 1: exactly today's tensors
    runs = (('plain', []), ('chunk', ['--chunk-batch', '2']))
    for name, extra in runs[1:] if mode == 'emul' else runs:      # (emulated threads are slow: the folder test runs the plain form)
        out = main(_cli(dev, tmp_path, 16, ['--steps-per-epoch', '2', '--val-steps', '1', '--save', name] + extra))
        assert _finite(out['train']) and _finite(out['val'])
        ck = torch.load(tmp_path / 'results' / name / 'checkpoint.pth.tar', map_location='cpu')
        assert ck['epoch'] == 1 and bool(torch.isfinite(ck['state_dict']['fc.weight']).all())


@pytest.mark.parametrize('mode', MODES)
def test_cli_trains_with_duplicates_on_an_image_folder(mode, tmp_path):
    """4 training images, b = 2 (one epoch of 2 steps of 2 x 2 views): with and without --device-resize, and with
    --chunk-batch 2; the --device-resize run and the host-resize run report the same training loss under the same seed
    (-j 0)."""
    from convnet_amd.main import main
    dev = _dev(mode)
    root = _folder(tmp_path / 'ds', classes=2, per_class=2)
    common = ['--dataset', 'imagenet', '--datasets-dir', str(root), '-j', '0']
    res = {}
    runs = (('host', []), ('devres', ['--device-resize']), ('chunk', ['--device-resize', '--chunk-batch', '2']))
    for name, extra in runs[:2] if mode == 'emul' else runs:      # (--chunk-batch on the emulator: the synthetic-data test)
        res[name] = main(_cli(dev, tmp_path, 3, common + ['--save', name] + extra))
        assert _finite(res[name]['train']) and _finite(res[name]['val'])
        ck = torch.load(tmp_path / 'results' / name / 'checkpoint.pth.tar', map_location='cpu')
        assert ck['epoch'] == 1 and bool(torch.isfinite(ck['state_dict']['fc.weight']).all())
    assert res['host']['train']['loss'] == res['devres']['train']['loss']
    assert res['host']['train']['prec1'] == res['devres']['train']['prec1']
    # --evaluate --duplicates 2 --avg-out --augment
    ev = main(_cli(dev, tmp_path, 3, common + ['--evaluate', str(tmp_path / 'results' / 'host' / 'checkpoint.pth.tar'),
                                               '--avg-out', '--augment', '--device-resize']))
    assert set(ev) >= {'loss', 'prec1', 'prec5'} and _finite(ev)
    if mode == 'gpu':      # host-resized centre views, averaged
        ev2 = main(_cli(dev, tmp_path, 3, common + ['--evaluate', str(tmp_path / 'results' / 'host' / 'checkpoint.pth.tar'),
                                                    '--avg-out']))
        assert _finite(ev2)


def test_cli_refusals(tmp_path):
    from convnet_amd.main import main
    dev = torch.device('cuda', 0) if HAS_GPU else torch.device('cpu')
    root = _folder(tmp_path / 'ds')
    common = ['--dataset', 'imagenet', '--datasets-dir', str(root), '-j', '0']
    for flag in ('--autoaugment', '--cutout'):
        with pytest.raises(NotImplementedError):
            main(_cli(dev, tmp_path, 3, common + ['--save', 'r' + flag.strip('-'), flag]))
    with pytest.raises(NotImplementedError):
        main(_cli(dev, tmp_path, 3, ['--save', 'agn', '--adapt-grad-norm', '4', '--steps-per-epoch', '1']))
