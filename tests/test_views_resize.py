"""duplicates > 1 on the input side: cn_resize_u8_views (csrc/resize.hip - PIL's fixed-point BILINEAR resize for views that
share one source region) bit for bit against PIL, and the loader paths that feed it (data.get_transform(duplicates=D),
RandomResizedCropViews / ViewsForDevice / collate_views, trainer.DevicePrefetcher).

Reference value of every view: Image.fromarray(src).crop(box).resize((S, S), BILINEAR), then FLIP_LEFT_RIGHT where flipped;
every byte must match.  Kernel tests run on the TEST-ONLY emulator on a GPU-less host and on the MI355X (`gpu`)."""
import numpy as np
import pytest
import torch

from conftest import HAS_GPU
from helpers import ROOT  # noqa: F401  (puts the repo root on sys.path)

PIL = pytest.importorskip('PIL')
from PIL import Image  # noqa: E402

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _to(inputs, dev):
    """What DevicePrefetcher._stage does with a views batch: everything but `size` to the device, the meta table also kept
    on the host."""
    out = {k: (v if k == 'size' else v.to(dev)) for k, v in inputs.items()}
    out['meta_host'] = inputs['meta']
    return out


def _sample(src, boxes, S):
    """ViewsForDevice of `boxes` = [((left, top, right, bottom), flip)] over the bounding region of the boxes, the way
    data.RandomResizedCropViews builds it, plus the PIL reference of every view."""
    from convnet_amd import data as D
    img = Image.fromarray(src if src.shape[2] > 1 else src[:, :, 0])
    x0, y0 = min(b[0] for b, _ in boxes), min(b[1] for b, _ in boxes)
    x1, y1 = max(b[2] for b, _ in boxes), max(b[3] for b, _ in boxes)
    pix = np.array(img.crop((x0, y0, x1, y1)), dtype=np.uint8)
    if pix.ndim == 2:
        pix = pix[:, :, None]
    views, ref = [], []
    for (l, t, r, b), flip in boxes:
        views.append((D.resample_table_cached(r - l, S), D.resample_table_cached(b - t, S), flip, l - x0, t - y0, r - l, b - t))
        want = img.crop((l, t, r, b)).resize((S, S), Image.BILINEAR)
        if flip:
            want = want.transpose(Image.FLIP_LEFT_RIGHT)
        want = np.array(want)
        ref.append(want if want.ndim == 3 else want[:, :, None])
    return D.ViewsForDevice(pix, views, S), ref


def _run(samples, dev):
    import convnet_amd as ca
    from convnet_amd import data as D
    inputs, target = D.collate_views([(s, i) for i, s in enumerate(samples)])
    assert target.tolist() == list(range(len(samples)))
    return ca.ops.resize_views(_to(inputs, dev)).cpu().numpy(), inputs


def _sources(C=3):
    rng = np.random.RandomState(17)
    return [rng.randint(0, 256, (h, w, C)).astype(np.uint8) for h, w in ((23, 31), (150, 200), (40, 52))]


def _cases_d3(srcs):
    """(source, [(box, flip)] * 3) per sample.  Sample 0: a view strictly inside a wider source (stride != w * C), the whole
    region, an up-scaled 3 x 5 view.  Sample 1: heavy down-scaling (a 200 x 150 view = the whole region, many taps) and two
    overlapping views with different flips.  Sample 2 (last in the pixel buffer): a view touching the region's right and
    bottom edge comes last."""
    return [
        (srcs[0], [((5, 3, 22, 18), False), ((0, 0, 31, 23), True), ((9, 7, 12, 12), False)]),
        (srcs[1], [((0, 0, 200, 150), True), ((20, 10, 120, 90), False), ((60, 40, 170, 140), True)]),
        (srcs[2], [((0, 0, 30, 25), False), ((4, 2, 40, 30), True), ((21, 17, 52, 40), False)]),
    ]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('S', [16, 33])
def test_views_match_pil_bit_for_bit(mode, S):
    dev = _dev(mode)
    cases = _cases_d3(_sources())
    samples, refs = zip(*[_sample(src, boxes, S) for src, boxes in cases])
    # the strictly-inside view really has a stride that differs from its own width
    assert samples[0].pix.shape[1] == 31 and samples[0].views[0][5] == 17
    out, inputs = _run(samples, dev)
    assert out.shape == (9, S, S, 3) and out.dtype == np.uint8
    meta = inputs['meta'].numpy()
    assert meta[0, 8] == 31 * 3 and meta[0, 2] * 3 < meta[0, 8]
    assert meta[8, 0] + (meta[8, 1] - 1) * meta[8, 8] + meta[8, 2] * 3 == inputs['views'].numel()   # ends the pixel buffer
    for b in range(3):
        for d in range(3):
            got, want = out[b * 3 + d], refs[b][d]
            assert np.array_equal(got, want), (S, b, d, int(np.abs(got.astype(int) - want.astype(int)).max()))


@pytest.mark.parametrize('mode', MODES)
def test_views_d1_wide_output_and_one_channel(mode):
    """D = 1 batches: S = 260 from a 40 x 30 source (the 256-thread column loop takes its second trip), and a C = 1 case."""
    dev = _dev(mode)
    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, (30, 40, 3)).astype(np.uint8)
    s, ref = _sample(src, [((0, 0, 40, 30), True)], 260)
    out, _ = _run([s], dev)
    assert out.shape == (1, 260, 260, 3) and np.array_equal(out[0], ref[0])
    g = rng.randint(0, 256, (37, 29, 1)).astype(np.uint8)
    s1, ref1 = _sample(g, [((3, 2, 25, 30), True)], 16)
    s2, ref2 = _sample(g, [((0, 5, 29, 37), False)], 16)
    out, _ = _run([s1, s2], dev)
    assert out.shape == (2, 16, 16, 1)
    assert np.array_equal(out[0], ref1[0]) and np.array_equal(out[1], ref2[0])


@pytest.mark.parametrize('mode', MODES)
def test_views_equal_separate_crops_through_the_crops_kernel(mode):
    """The same D views fed as D separate CropForDevice crops through cn_resize_u8_crops: identical bytes."""
    import convnet_amd as ca
    from convnet_amd import data as D
    dev = _dev(mode)
    S = 33
    cases = _cases_d3(_sources())
    samples = [_sample(src, boxes, S)[0] for src, boxes in cases]
    out, _ = _run(samples, dev)
    crops = []
    for src, boxes in cases:
        for (l, t, r, b), flip in boxes:
            c = D.CropForDevice(np.ascontiguousarray(src[t:b, l:r]), D.resample_table_cached(r - l, S),
                                D.resample_table_cached(b - t, S), S)
            c.flip = flip
            crops.append((c, 0))
    inputs, _ = D.collate_crops(crops)
    sep = ca.ops.resize_crops({k: (v if k == 'size' else v.to(dev)) for k, v in inputs.items()}).cpu().numpy()
    assert sep.shape == out.shape and np.array_equal(sep, out)


@pytest.mark.parametrize('mode', MODES)
def test_views_argument_checks(mode):
    """Null operand, C = 5, stride < w * C (and a view that leaves the pixel buffer): refused before any launch."""
    import convnet_amd as ca
    from convnet_amd import data as D
    dev = _dev(mode)
    Err = ca._lib.ConvNetHipError
    s, _ = _sample(_sources()[0], [((5, 3, 22, 18), False), ((0, 0, 31, 23), True)], 16)
    inputs, _ = D.collate_views([(s, 0)])
    good = _to(inputs, dev)
    ca.ops.resize_views(good)
    L = ca._lib.load()
    p = ca._lib.ptr
    px, meta, tables, owner, mh = good['views'], good['meta'], good['tables'], good['row_owner'], good['meta_host']
    rows = owner.numel()
    tmp = torch.empty(rows * 16 * 3, dtype=torch.uint8, device=dev)
    out = torch.empty(2 * 16 * 16 * 3, dtype=torch.uint8, device=dev)

    def call(px_=p(px), C=3, mh_=mh):
        return L.cn_resize_u8_views(px_, p(meta), p(tables), p(owner), p(tmp), p(out), p(mh_), px.numel(), tables.numel(), 2,
                                    rows, 16, C, None if dev.type == 'cpu' else torch.cuda.current_stream(dev).cuda_stream)
    call()
    with pytest.raises(Err, match='null operand'):
        call(px_=None)
    with pytest.raises(Err, match='bad shape'):
        call(C=5)
    bad = mh.clone()
    bad[0, 8] = bad[0, 2] * 3 - 1
    with pytest.raises(Err, match='stride'):
        call(mh_=bad)
    bad = mh.clone()
    bad[1, 0] += 1
    with pytest.raises(Err, match='outside the pixel buffer'):
        call(mh_=bad)
    with pytest.raises(Err, match='stride'):
        b2 = dict(good)
        b2['meta_host'] = mh.clone()
        b2['meta_host'][0, 8] = 1
        ca.ops.resize_views(b2)


# ---- loader ---------------------------------------------------------------------------------------------------------------

def _image(seed=0, h=75, w=100):
    return Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8))


@pytest.mark.parametrize('augment', [True, False])
@pytest.mark.parametrize('device_normalize', [False, True])
def test_duplicates_is_multi_transform(augment, device_normalize):
    """multi_transform's definition: get_transform(duplicates=3) on an image after manual_seed(s) == torch.stack of three
    successive calls of the duplicates=1 transform after the same seed (draw order crop, flip; crop, flip; ...)."""
    from convnet_amd import data as D
    img = _image()
    kw = dict(input_size=32, augment=augment, device_normalize=device_normalize)
    one, three = D.get_transform('imagenet', **kw), D.get_transform('imagenet', duplicates=3, **kw)
    torch.manual_seed(4)
    want = torch.stack([one(img) for _ in range(3)], dim=0)
    torch.manual_seed(4)
    got = three(img)
    assert got.dtype == (torch.uint8 if device_normalize else torch.float32)
    assert tuple(got.shape) == ((3, 32, 32, 3) if device_normalize else (3, 3, 32, 32))
    assert torch.equal(got, want)
    if augment:
        assert not torch.equal(got[0], got[1])      # the views really differ
    else:
        assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def test_views_transform_draws_in_host_order():
    """RandomResizedCropViews draws its D (box, flip) pairs exactly as D calls of the host transform do, crops the image
    once to their bounding box, and every view's tables are those of its own box."""
    from convnet_amd import data as D
    img = _image(1)
    torch.manual_seed(6)
    rrc = D.RandomResizedCrop(32)
    want = []
    for _ in range(3):
        box = rrc.get_params(*img.size)
        want.append((box, bool(torch.rand(1) < 0.5)))
    torch.manual_seed(6)
    v = D.get_transform('imagenet', input_size=32, duplicates=3, device_normalize=True, device_resize=True)(img)
    assert isinstance(v, D.ViewsForDevice) and len(v.views) == 3 and v.size == 32
    x0, y0 = min(b[0] for b, _ in want), min(b[1] for b, _ in want)
    x1, y1 = max(b[0] + b[2] for b, _ in want), max(b[1] + b[3] for b, _ in want)
    assert v.pix.shape == (y1 - y0, x1 - x0, 3)
    assert np.array_equal(v.pix, np.asarray(img)[y0:y1, x0:x1])
    for (th, tv, flip, left, top, w, h), ((bl, bt, bw, bh), bf) in zip(v.views, want):
        assert (flip, left + x0, top + y0, w, h) == (bf, bl, bt, bw, bh)
        assert th is D.resample_table_cached(bw, 32) and tv is D.resample_table_cached(bh, 32)
        assert int((th[:, 0] + th[:, 1]).max()) <= w and int((tv[:, 0] + tv[:, 1]).max()) <= h    # no tap outside the box


def test_duplicates_1_keeps_todays_objects():
    from convnet_amd import data as D
    img = _image(2)
    t = D.get_transform('imagenet', input_size=32, duplicates=1, device_normalize=True, device_resize=True)
    c = t(img)
    assert isinstance(c, D.CropForDevice)
    inputs, _ = D.collate_crops([(c, 0)])
    assert isinstance(inputs, dict) and 'crops' in inputs and 'views' not in inputs
    assert tuple(D.get_transform('imagenet', input_size=32, duplicates=1)(img).shape) == (3, 32, 32)
    assert isinstance(D.get_transform('imagenet', input_size=32, duplicates=1), D.Compose)
    for kw in (dict(autoaugment=True), dict(cutout={'holes': 1, 'length': 16}), dict(num_crops=5)):
        with pytest.raises(NotImplementedError):
            D.get_transform('imagenet', input_size=32, duplicates=2, **kw)
    with pytest.raises(ValueError):
        D.get_transform('imagenet', input_size=32, duplicates=0)


def _make_folder(root, seed=2):
    """(test_data.py's recipe, own copy) root/imagenet/{train,val}/c{0,1,2}/{0..3}.png of different sizes."""
    rng = np.random.RandomState(seed)
    for split in ('train', 'val'):
        for c in range(3):
            d = root / 'imagenet' / split / ('c%d' % c)
            d.mkdir(parents=True)
            for i in range(4):
                a = (rng.rand(60 + 17 * i, 90 - 11 * c, 3) * 255).astype(np.uint8)
                Image.fromarray(a).save(str(d / ('%d.png' % i)))
    return root


def _path_equivalence(root, dev, num_workers):
    import convnet_amd as ca
    from convnet_amd import data as D
    for split, augment in (('train', True), ('val', False)):
        got = {}
        for name, dn, dres in (('host', False, False), ('device_normalize', True, False), ('device_resize', True, True)):
            torch.manual_seed(9)
            reg = D.DataRegime([{'epoch': 0}], defaults={'datasets_path': str(root), 'name': 'imagenet', 'split': split,
                                                          'augment': augment, 'input_size': 32, 'batch_size': 4,
                                                          'shuffle': False, 'num_workers': num_workers, 'drop_last': False,
                                                          'pin_memory': num_workers > 0, 'duplicates': 2,
                                                          'device_normalize': dn, 'device_resize': dres})
            loader = reg.get_loader()
            if num_workers == 0:
                first = next(iter(loader))[0]
                if dres:
                    assert isinstance(first, dict) and 'views' in first and first['size'].tolist() == [32, 3, 2]
                else:
                    assert first.dtype == (torch.uint8 if dn else torch.float32)
                    assert tuple(first.shape) == ((4, 2, 32, 32, 3) if dn else (4, 2, 3, 32, 32))
            torch.manual_seed(9)
            got[name] = [(x.cpu().clone(), t.cpu().clone()) for x, t in ca.trainer.DevicePrefetcher(loader, dev)]
            del loader, reg
        assert len(got['host']) == len(got['device_normalize']) == len(got['device_resize']) == 3
        for (x0, t0), (x1, t1), (x2, t2) in zip(got['host'], got['device_normalize'], got['device_resize']):
            assert x0.dtype == x1.dtype == x2.dtype == torch.float32
            assert tuple(x0.shape) == tuple(x1.shape) == tuple(x2.shape) == (4, 2, 3, 32, 32)
            assert torch.equal(t0, t1) and torch.equal(t0, t2) and tuple(t0.shape) == (4,)
            assert torch.equal(x0, x1), (split, 'device_normalize')
            assert torch.equal(x0, x2), (split, 'device_resize')
            if augment:
                assert not torch.equal(x0[:, 0], x0[:, 1])
            else:
                assert torch.equal(x0[:, 0], x0[:, 1])


def test_three_loader_paths_deliver_identical_batches(tmp_path):
    """DataRegime(duplicates=2, num_workers=0) as host / device_normalize / device_resize under the same seed: the batches
    DevicePrefetcher delivers are fp32 [B, 2, 3, 32, 32] and bit-identical to one another, train and val."""
    if HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    _path_equivalence(_make_folder(tmp_path / 'ds'), torch.device('cpu'), 0)


@pytest.mark.gpu
def test_three_loader_paths_deliver_identical_batches_gpu(tmp_path):
    """The same on the MI355X through two worker processes and pinned buffers."""
    _path_equivalence(_make_folder(tmp_path / 'ds'), torch.device('cuda', 0), 2)
