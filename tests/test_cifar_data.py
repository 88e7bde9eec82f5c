"""The CIFAR input path of data.py: the pickle reader (CIFAR), get_transform('cifar...'), DeviceCifarLoader and DataRegime.
Everything runs on fabricated pickle files in the CIFAR-10 and CIFAR-100 layouts (20 train / 6 test images); the loader runs
on the GPU when there is one and on the emulator otherwise."""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import HAS_GPU

DEV = torch.device('cuda', 0) if HAS_GPU else torch.device('cpu')
STATS = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}
# torch.manual_seed(2024); then per sample torch.randint(0, 9, (1,)) [top], torch.randint(0, 9, (1,)) [left],
# torch.rand(1) < 0.5 [flip] - torchvision's RandomCrop.get_params + RandomHorizontalFlip.forward on a 40 x 40 padded image
RECORDED = [(8, 2, False), (8, 6, True), (1, 8, True), (3, 2, False), (3, 4, False), (8, 6, False)]


def _planar(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3072)).astype(np.uint8)


def fabricate(root, classes, n_train=20, n_test=6):
    """The python-pickle release layout under <root>/cifar10|cifar100; returns (train planar, train labels, test planar, labels)."""
    tr, te = _planar(n_train, 1), _planar(n_test, 2)
    ltr = [(7 * i + 3) % classes for i in range(n_train)]
    lte = [(5 * i + 1) % classes for i in range(n_test)]
    if classes == 10:
        d = os.path.join(root, 'cifar10', 'cifar-10-batches-py')
        os.makedirs(d)
        cuts = [n_train * b // 5 for b in range(6)]
        for b in range(5):
            with open(os.path.join(d, 'data_batch_%d' % (b + 1)), 'wb') as f:
                pickle.dump({'data': tr[cuts[b]:cuts[b + 1]], 'labels': ltr[cuts[b]:cuts[b + 1]]}, f)
        with open(os.path.join(d, 'test_batch'), 'wb') as f:
            pickle.dump({'data': te, 'labels': lte}, f)
    else:
        d = os.path.join(root, 'cifar100', 'cifar-100-python')
        os.makedirs(d)
        with open(os.path.join(d, 'train'), 'wb') as f:
            pickle.dump({'data': tr, 'fine_labels': ltr, 'coarse_labels': [0] * n_train}, f)
        with open(os.path.join(d, 'test'), 'wb') as f:
            pickle.dump({'data': te, 'fine_labels': lte, 'coarse_labels': [0] * n_test}, f)
    return tr, ltr, te, lte


@pytest.mark.parametrize('classes', [10, 100])
def test_pickle_reader(tmp_path, classes):
    from convnet_amd import data as D
    tr, ltr, te, lte = fabricate(str(tmp_path), classes)
    name = 'cifar%d' % classes
    train = D.get_dataset(name, 'train', datasets_path=str(tmp_path), download=True)
    val = D.get_dataset(name, 'val', datasets_path=str(tmp_path))
    assert len(train) == 20 and len(val) == 6 and train.num_classes == classes
    assert train.targets == ltr and val.targets == lte
    assert train.data.dtype == np.uint8 and train.data.shape == (20, 32, 32, 3)
    hand = np.empty((20, 32, 32, 3), np.uint8)       # planar CHW -> HWC, by hand
    for c in range(3):
        hand[:, :, :, c] = tr[:, 1024 * c:1024 * (c + 1)].reshape(20, 32, 32)
    assert np.array_equal(train.data, hand)
    assert np.array_equal(val.data[5, 31, 30], te[5, [1022, 2046, 3070]])
    img, t = train[3]
    assert img.size == (32, 32) and t == ltr[3] and np.array_equal(np.asarray(img), hand[3])


def test_missing_files_raise_naming_the_path(tmp_path):
    from convnet_amd import data as D
    with pytest.raises(FileNotFoundError, match='data_batch_1'):
        D.get_dataset('cifar10', 'train', datasets_path=str(tmp_path), download=True)
    with pytest.raises(FileNotFoundError, match='cifar-100-python'):
        D.get_dataset('cifar100', 'val', datasets_path=str(tmp_path))
    with pytest.raises(NotImplementedError):
        D.get_dataset('svhn', 'train', datasets_path=str(tmp_path))


def test_random_crop_and_flip_follow_the_recorded_draws():
    from PIL import Image
    from convnet_amd import data as D
    img = Image.fromarray(_planar(1, 9).reshape(3, 32, 32).transpose(1, 2, 0))
    a = np.asarray(img)
    padded = np.zeros((40, 40, 3), np.uint8)
    padded[4:36, 4:36] = a
    t = D.get_transform('cifar10', augment=True)
    assert [type(x).__name__ for x in t.transforms] == ['RandomCrop', 'RandomHorizontalFlip', 'ToTensor', 'Normalize']
    assert t.transforms[0].size == 32 and t.transforms[0].padding == 4
    torch.manual_seed(2024)
    for top, left, flip in RECORDED:
        out = t(img)
        want = padded[top:top + 32, left:left + 32]
        want = want[:, ::-1] if flip else want
        ref = D.Normalize(**STATS)(torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1))).float().div_(255.0))
        assert torch.equal(out, ref), (top, left, flip)
    torch.manual_seed(2024)       # the crop transform alone: top first, then left
    rc = D.RandomCrop(32, padding=4)
    assert rc.get_params(40, 40) == RECORDED[0][:2]
    state = torch.get_rng_state()
    assert D.RandomCrop(32).get_params(32, 32) == (0, 0) and torch.equal(torch.get_rng_state(), state)     # no draw


def test_eval_transform_cutout_duplicates_and_refusals():
    from PIL import Image
    from convnet_amd import data as D
    a = _planar(1, 9).reshape(3, 32, 32).transpose(1, 2, 0)
    img = Image.fromarray(a)
    ev = D.get_transform('cifar100', augment=False)
    plain = D.Normalize(**STATS)(torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div_(255.0))
    assert torch.equal(ev(img), plain)                          # the identity crop
    cut = D.get_transform('cifar10', augment=False, cutout={'holes': 1, 'length': 16})
    np.random.seed(5)
    y, x = np.random.randint(32), np.random.randint(32)
    np.random.seed(5)
    out = cut(img)
    y1, y2, x1, x2 = D.cutout_rect(y, x, 16, 32, 32)
    assert (y1, y2, x1, x2) == (max(y - 8, 0), min(y + 8, 32), max(x - 8, 0), min(x + 8, 32))
    want = plain.clone()
    want[:, y1:y2, x1:x2] = 0
    assert torch.equal(out, want)
    dup = D.get_transform('cifar10', augment=True, duplicates=3)
    assert isinstance(dup, D.MultiTransform) and tuple(dup(img).shape) == (3, 3, 32, 32)
    with pytest.raises(NotImplementedError):
        D.get_transform('cifar10', autoaugment=True)
    with pytest.raises(NotImplementedError):                    # the imagenet branch and its refusals are untouched
        D.get_transform('imagenet', cutout={'holes': 1, 'length': 16})


def _loader(tmp_path, split='train', classes=10, **kw):
    from convnet_amd import data as D
    if not os.path.isdir(os.path.join(str(tmp_path), 'cifar%d' % classes)):
        fabricate(str(tmp_path), classes)
    ds = D.get_dataset('cifar%d' % classes, split, datasets_path=str(tmp_path))
    return ds, D.DeviceCifarLoader(ds, device=DEV, **kw)


def _host(ds, i, top, left, flip, pad, rect=(0, 0, 0, 0)):
    padded = np.zeros((32 + 2 * pad, 32 + 2 * pad, 3), np.uint8)
    padded[pad:pad + 32, pad:pad + 32] = ds.data[i]
    w = padded[top:top + 32, left:left + 32]
    w = w[:, ::-1] if flip else w
    from convnet_amd import data as D
    t = D.Normalize(**STATS)(torch.from_numpy(np.ascontiguousarray(w.transpose(2, 0, 1))).float().div_(255.0))
    t[:, rect[0]:rect[1], rect[2]:rect[3]] = 0
    return t


def test_device_loader_train_epoch(tmp_path):
    """An epoch is a permutation cut into full batches (drop_last); every batch is what the host transforms make of the same
    samples with the same drawn parameters; reseeding reproduces the epoch."""
    import convnet_amd as ca
    ds, ld = _loader(tmp_path, batch_size=6, augment=True, cutout={'holes': 1, 'length': 16})
    assert len(ld) == 3
    torch.manual_seed(11)
    np.random.seed(11)
    order = torch.randperm(20)
    first = ld.draw_params(6, 1, 4, {'holes': 1, 'length': 16})
    assert first.dtype == torch.int32 and tuple(first.shape) == (6, 8)
    assert int(first[:, :2].min()) >= 0 and int(first[:, :2].max()) <= 8 and set(first[:, 2].tolist()) <= {0, 1}
    torch.manual_seed(11)
    np.random.seed(11)
    batches = [(x.float().cpu(), t.cpu()) for x, t in ld]
    assert len(batches) == 3
    seen = torch.cat([t for _, t in batches])
    assert seen.tolist() == [ds.targets[i] for i in order[:18].tolist()]          # a permutation, the tail dropped
    x0 = batches[0][0]
    assert tuple(x0.shape) == (6, 32, 32, 4)
    for j in range(6):
        top, left, flip, y1, y2, x1, x2, _ = first[j].tolist()
        want = _host(ds, int(order[j]), top, left, flip, 4, (y1, y2, x1, x2))
        assert torch.equal(x0[j, :, :, :3].permute(2, 0, 1), want), j
    assert float(x0[..., 3].abs().sum()) == 0.0
    torch.manual_seed(11)
    np.random.seed(11)
    again = [(x.float().cpu(), t.cpu()) for x, t in ld]
    for (xa, ta), (xb, tb) in zip(batches, again):
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert ca.ops.AUGMENT_PARAMS == 8


def test_device_loader_eval_is_sequential_identity_with_partial_last_batch(tmp_path):
    ds, ld = _loader(tmp_path, split='val', batch_size=4, augment=False)
    assert len(ld) == 2
    out = [(x.float().cpu(), t.cpu()) for x, t in ld]
    assert [x.shape[0] for x, _ in out] == [4, 2]
    assert torch.cat([t for _, t in out]).tolist() == ds.targets
    for i in range(6):
        x = torch.cat([x for x, _ in out])[i]
        assert torch.equal(x[:, :, :3].permute(2, 0, 1), _host(ds, i, 0, 0, False, 0))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_device_loader_duplicates_layout_and_compute_dtype(tmp_path, dtype):
    ds, ld = _loader(tmp_path, classes=100, batch_size=5, augment=True, duplicates=2, dtype=dtype)
    torch.manual_seed(3)
    order = torch.randperm(20)
    p = ld.draw_params(5, 2)
    torch.manual_seed(3)
    x, t = next(iter(ld))
    assert tuple(x.shape) == (5, 2, 32, 32, 8) and x.dtype == dtype and tuple(t.shape) == (5,)
    assert t.tolist() == [ds.targets[i] for i in order[:5].tolist()]
    x = x.float().cpu()
    for b in range(5):
        for d in range(2):          # sample-major: view b * D + d belongs to sample b
            top, left, flip = p[b * 2 + d, :3].tolist()
            want = _host(ds, int(order[b]), top, left, flip, 4).to(dtype).float()
            assert torch.equal(x[b, d, :, :, :3].permute(2, 0, 1), want), (b, d)


def test_device_loader_ranks_partition_the_epoch(tmp_path):
    ds, l0 = _loader(tmp_path, batch_size=5, augment=True, distributed=True, rank=0, world_size=2)
    _, l1 = _loader(tmp_path, batch_size=5, augment=True, distributed=True, rank=1, world_size=2)
    for ld in (l0, l1):
        ld.set_epoch(3)
    a, b = l0.epoch_indices(), l1.epoch_indices()
    assert len(l0) == len(l1) == 2 and a.numel() == b.numel() == 10
    assert sorted(a.tolist() + b.tolist()) == list(range(20))
    g = torch.Generator().manual_seed(3)       # DistributedSampler: seed + epoch, rank::world
    perm = torch.randperm(20, generator=g)
    assert torch.equal(a, perm[0::2]) and torch.equal(b, perm[1::2])
    l0.set_epoch(4)
    assert not torch.equal(l0.epoch_indices(), a)
    l0.set_epoch(3)
    assert torch.equal(l0.epoch_indices(), a)


def test_data_regime_builds_the_resident_loader_or_the_worker_pipeline(tmp_path):
    from convnet_amd import data as D
    fabricate(str(tmp_path), 10)
    common = {'datasets_path': str(tmp_path), 'name': 'cifar10', 'split': 'train', 'augment': True, 'batch_size': 4,
              'shuffle': True, 'num_workers': 0, 'drop_last': True, 'duplicates': 1, 'cutout': None, 'autoaugment': False}
    res = D.DataRegime(None, defaults=dict(common, device_normalize=True, device=DEV, dtype=torch.float32))
    ld = res.get_loader()
    assert isinstance(ld, D.DeviceCifarLoader) and len(ld) == 5 and len(res) == 20
    x, t = next(iter(ld))
    assert x.device.type == DEV.type and tuple(x.shape) == (4, 32, 32, 4)
    host = D.DataRegime(None, defaults=dict(common, device_normalize=False, device=DEV, dtype=torch.float32))
    x, t = next(iter(host.get_loader()))
    assert not isinstance(host.get_loader(), D.DeviceCifarLoader) and tuple(x.shape) == (4, 3, 32, 32) and x.dtype == torch.float32
    with pytest.raises(NotImplementedError):
        D.DataRegime(None, defaults=dict(common, device_normalize=True, device=DEV, autoaugment=True))
    with pytest.raises(NotImplementedError):
        D.DataRegime(None, defaults=dict(common, device_normalize=False, autoaugment=True))


@pytest.mark.gpu
def test_plan_on_resident_loader_batches_is_bit_identical_to_eager(tmp_path):
    """bf16, 6 steps on DeviceCifarLoader's NHWC compute-dtype batches: the trainer passes them through uncast, the recorded
    launch plan re-points every reader of the batch (conv1's forward and its weight gradient) at the loader's tensor, and
    losses and every state tensor equal the run with plan = 0 bit for bit."""
    import convnet_amd as ca
    fabricate(str(tmp_path), 10, n_train=48, n_test=6)
    from convnet_amd import data as D
    ds = D.get_dataset('cifar10', 'train', datasets_path=str(tmp_path))
    ld = D.DeviceCifarLoader(ds, 8, DEV, torch.bfloat16, augment=True, cutout={'holes': 1, 'length': 16})
    torch.manual_seed(5)
    np.random.seed(5)
    batches = list(ld)
    torch.cuda.synchronize()
    assert len(batches) == 6 and batches[0][0].dtype == torch.bfloat16 and tuple(batches[0][0].shape) == (8, 32, 32, 8)
    assert not torch.equal(batches[0][0], batches[1][0])
    outs = []
    for plan in (False, True):
        torch.manual_seed(123)
        model = ca.models.resnet(dataset='cifar10', depth=20)
        from helpers import warm_bn_state
        warm_bn_state(model, 977)
        tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device=str(DEV),
                        dtype=torch.bfloat16, grad_clip=1e9, print_freq=10 ** 9)
        tr._graph_mode = '1' if plan else '0'
        tr._use_graph = plan
        assert tr._is_compute_nhwc(batches[0][0])
        losses = [float(tr.train([b])['loss']) for b in batches]
        torch.cuda.synchronize()
        if plan:
            planned = [s['graph'] for s in tr._gstates.values() if s['graph'] is not None and s['graph'].get('plan') is not None]
            assert planned, 'the step never ran as a recorded plan'
            assert all(g['x_sites'] >= 2 for g in planned), [g['x_sites'] for g in planned]      # conv1 forward + its wgrad
            assert all(bool(torch.isnan(g['x'].float()).all()) for g in planned)                # the static copy is poisoned
        outs.append((losses, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()
                              if v.dtype.is_floating_point}))
    assert all(l == l and abs(l) < 1e3 for l in outs[1][0]), outs[1][0]
    assert len(set(outs[0][0])) > 1 and outs[0][0] == outs[1][0]
    for k in outs[0][1]:
        assert bool(torch.isfinite(outs[1][1][k]).all()), k
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.mark.parametrize('mode', MODES)
def test_cli_on_pickle_files_through_the_resident_loader(mode, tmp_path):
    """One epoch of main.py on fabricated CIFAR-10 files: train, validate, checkpoint, resume."""
    if (mode == 'gpu') != HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts' if HAS_GPU else 'no GPU')
    from convnet_amd.main import main
    n_train, n_test, b = (20, 6, '8') if HAS_GPU else (8, 4, '4')      # (the emulator runs one lane at a time)
    fabricate(str(tmp_path / 'ds'), 10, n_train, n_test)
    common = ['--model', 'resnet', '--dataset', 'cifar10', '--datasets-dir', str(tmp_path / 'ds'), '--model-config',
              "{'depth': 8}", '-b', b, '--eval-batch-size', '4', '--dtype', 'bfloat16' if HAS_GPU else 'float', '--device',
              'cuda' if HAS_GPU else 'cpu', '--results-dir', str(tmp_path), '--print-freq', '1', '-j', '0', '--cutout']
    out = main(common + ['--save', 'run', '--epochs', '1'])
    assert out['train']['loss'] == out['train']['loss'] and out['val']['loss'] > 0
    ck = torch.load(tmp_path / 'run' / 'checkpoint.pth.tar', map_location='cpu')
    assert ck['epoch'] == 1 and tuple(ck['state_dict']['fc.weight'].shape) == (10, 64)
    main(common + ['--save', 'run2', '--epochs', '2', '--resume', str(tmp_path / 'run' / 'checkpoint.pth.tar')])
    assert torch.load(tmp_path / 'run2' / 'checkpoint.pth.tar', map_location='cpu')['epoch'] == 2
