"""csrc/augment.hip (ops.crop_flip_normalize): RandomCrop(S, padding) -> flip -> ToTensor -> Normalize -> Cutout on a uint8
dataset resident in device memory, against the host transforms of data.py applied with the same parameters.

  * form 'nchw' equals the host pipeline value for value (torch.equal: -0.0 == 0.0);
  * form 'nhwc' is bit-equal to ops.nchw_to_nhwc of the former, in fp32 / bf16 / f16;
  * every (top, left, flip) combination of pad = 4, cutout rectangles (none, centre, clipped at each corner, the full image),
    pad = 0 (the eval identity), S = 8 with pad = 2;
  * wrong dtype, params / idx out of range: refused on the host, nothing is launched."""
import numpy as np
import pytest
import torch

from conftest import HAS_GPU

MODES = [pytest.param('emul'), pytest.param('gpu', marks=pytest.mark.gpu)]
DTYPES = [pytest.param(torch.float32, id='fp32'), pytest.param(torch.bfloat16, id='bf16'), pytest.param(torch.float16, id='f16')]
STATS = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}


def _dev(mode):
    if mode == 'emul' and HAS_GPU:
        pytest.skip('emulator mode is for GPU-less hosts')
    if mode == 'gpu' and not HAS_GPU:
        pytest.skip('no GPU')
    return torch.device('cuda', 0) if mode == 'gpu' else torch.device('cpu')


def _dataset(n, S, seed):
    d = torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    d[0, 0, 0] = 0          # both ends of the table occur
    d[-1, -1, -1] = 255
    return d


def _host_view(img, S, pad, top, left, flip, rect):
    """The host Compose of data.py with fixed parameters: pad the uint8 image with 0, crop, flip (PIL), ToTensor, Normalize,
    then Cutout's mask multiply."""
    from PIL import Image
    from convnet_amd import data as D
    im = Image.fromarray(img.numpy())
    canvas = Image.new('RGB', (S + 2 * pad, S + 2 * pad))
    canvas.paste(im, (pad, pad))
    im = canvas.crop((left, top, left + S, top + S))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    t = D.Normalize(**STATS)(D.ToTensor()(im))
    y1, y2, x1, x2 = rect
    mask = np.ones((S, S), np.float32)
    mask[y1:y2, x1:x2] = 0.
    return t * torch.from_numpy(mask).expand_as(t)


def _params(rows):
    p = torch.zeros((len(rows), 8), dtype=torch.int32)
    for i, (top, left, flip, rect) in enumerate(rows):
        p[i, :7] = torch.tensor([top, left, flip, *rect], dtype=torch.int32)
    return p


_REF = {}


def _case(name):
    """(data, idx, params, pad, host reference [V, 3, S, S]) - computed once, shared, never modified."""
    if name in _REF:
        return _REF[name]
    none = (0, 0, 0, 0)
    if name == 'all_crops':          # 9 x 9 x 2 = 162 views, idx cycling through the 7 images
        S, pad, data = 32, 4, _dataset(7, 32, 1)
        rows = [(t, l, f, none) for t in range(9) for l in range(9) for f in (0, 1)]
    elif name == 'cutout':           # none, centre, clipped at each corner, full image
        S, pad, data = 32, 4, _dataset(7, 32, 1)
        rows = [(3, 5, 1, none), (4, 4, 0, (8, 24, 8, 24)), (0, 8, 1, (0, 6, 0, 9)), (8, 0, 0, (0, 5, 25, 32)),
                (2, 7, 1, (27, 32, 0, 8)), (6, 1, 0, (24, 32, 30, 32)), (4, 4, 1, (0, 32, 0, 32))]
    elif name == 'identity':         # pad 0: the eval transform
        S, pad, data = 32, 0, _dataset(7, 32, 1)
        rows = [(0, 0, 0, none)] * 7
    elif name == 's8':
        S, pad, data = 8, 2, _dataset(5, 8, 2)
        rows = [(t, l, (t + l) & 1, (0, 0, 0, 0) if t != 2 else (1, 5, 2, 8)) for t in range(5) for l in range(5)]
    else:
        raise KeyError(name)
    idx = torch.tensor([i % data.shape[0] for i in range(len(rows))], dtype=torch.int32)
    ref = torch.stack([_host_view(data[int(i)], S, pad, *r) for i, r in zip(idx, rows)])
    _REF[name] = (data, idx, _params(rows), pad, ref)
    return _REF[name]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['all_crops', 'cutout', 'identity', 's8'])
def test_nchw_form_equals_the_host_pipeline(mode, case):
    import convnet_amd as ca
    dev = _dev(mode)
    data, idx, params, pad, ref = _case(case)
    lut = ca.ops.normalize_lut(**STATS)
    a = ca.ops.crop_flip_normalize(data.to(dev), idx, params, lut, torch.float32, 'nchw', pad=pad)
    assert a.shape == ref.shape and a.dtype == torch.float32
    assert torch.equal(a.cpu(), ref)
    if case == 'identity':
        from convnet_amd import data as D
        assert torch.equal(a.cpu()[3], D.Normalize(**STATS)(data[3].permute(2, 0, 1).float().div(255.0)))
    if case == 'all_crops':      # a padded pixel is byte 0 AFTER Normalize, not 0.0
        assert float(a[0, 0, 0, 0]) == float(lut[0, 0]) != 0.0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', ['all_crops', 'cutout', 'identity', 's8'])
def test_nhwc_form_is_bit_equal_to_the_converted_nchw_form(mode, dtype, case):
    import convnet_amd as ca
    dev = _dev(mode)
    data, idx, params, pad, ref = _case(case)
    lut = ca.ops.normalize_lut(**STATS)
    b = ca.ops.crop_flip_normalize(data.to(dev), idx, params, lut, dtype, 'nhwc', pad=pad)
    want = ca.ops.nchw_to_nhwc(ref.to(dev), dtype)
    assert b.dtype == dtype and tuple(b.shape) == tuple(want.shape) == (ref.shape[0], ref.shape[2], ref.shape[3],
                                                                       4 if dtype == torch.float32 else 8)
    # (value comparison would hide nothing here either, but the contract is the bits: cutout zeros are +0.0 in both)
    a = ca.ops.crop_flip_normalize(data.to(dev), idx, params, lut, torch.float32, 'nchw', pad=pad)
    want_a = ca.ops.nchw_to_nhwc(a, dtype)
    ib = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(b.cpu().view(ib), want_a.cpu().view(ib))
    assert torch.equal(b.cpu(), want.cpu())
    assert float(b[..., 3:].float().abs().sum()) == 0.0       # pad channels


@pytest.mark.parametrize('mode', MODES)
def test_refusals_happen_on_the_host(mode):
    import convnet_amd as ca
    dev = _dev(mode)
    data, idx, params, pad, _ = _case('cutout')
    d, lut = data.to(dev), ca.ops.normalize_lut(**STATS)
    E = ca._lib.ConvNetHipError
    with pytest.raises(E):
        ca.ops.crop_flip_normalize(d.float(), idx, params, lut, torch.float32, 'nchw')          # data not uint8
    with pytest.raises(E):
        ca.ops.crop_flip_normalize(d, idx, params, lut, torch.float64, 'nhwc')                   # unsupported compute dtype
    with pytest.raises(E):
        ca.ops.crop_flip_normalize(d, idx, params, lut, torch.bfloat16, 'nchw')                  # the nchw form is fp32
    with pytest.raises(E):
        ca.ops.crop_flip_normalize(d, idx.long(), params, lut, torch.float32, 'nchw')           # idx not int32
    for col, bad in ((0, 9), (0, -1), (1, 9), (2, 2), (3, -1), (4, 33), (6, 40)):
        p = params.clone()
        p[2, col] = bad
        with pytest.raises(E, match='out of range'):
            ca.ops.crop_flip_normalize(d, idx, p, lut, torch.float32, 'nchw')
    p = params.clone()
    p[1, 3], p[1, 4] = 20, 10                                                                      # y1 > y2
    with pytest.raises(E, match='out of range'):
        ca.ops.crop_flip_normalize(d, idx, p, lut, torch.float32, 'nchw')
    for bad in (-1, 7):
        i = idx.clone()
        i[3] = bad
        with pytest.raises(E, match='idx out of range'):
            ca.ops.crop_flip_normalize(d, i, params, lut, torch.float32, 'nchw')
    with pytest.raises(E):       # one record per index
        ca.ops.crop_flip_normalize(d, idx, params[:3], lut, torch.float32, 'nchw')
    # the C entry point checks its own arguments: the buffer size against N * S * S * 3, the chunk width, the form
    L = ca._lib.load()
    out = torch.empty(7 * 32 * 32 * 8, dtype=torch.float32, device=dev)
    di, dp, dl = idx.to(dev), params.to(dev), lut.to(dev)
    args = lambda **kw: [kw.get(k, v) for k, v in (('data', d.data_ptr()), ('bytes', d.numel()), ('idx', di.data_ptr()),    # noqa: E731
                         ('params', dp.data_ptr()), ('lut', dl.data_ptr()), ('out', out.data_ptr()), ('N', 7), ('V', 7), ('S', 32),
                         ('pad', 4), ('c_pad', 4), ('dtype', 0), ('form', 1), ('stream', None))]
    for kw in (dict(bytes=d.numel() - 1), dict(N=8), dict(c_pad=8), dict(form=2), dict(dtype=5), dict(form=0, dtype=1),
               dict(data=None), dict(V=0), dict(pad=-1)):
        with pytest.raises(E):
            L.cn_augment_crop_flip(*args(**kw))
