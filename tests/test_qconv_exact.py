"""Bit-exact checks of the int8 MFMA forward convolution (csrc/qconv_i8.hip), its pre-passes and the Python geometry
code of quant.py, element by element.  No tolerance appears anywhere: every assertion is an equality.

The path computes  y = sx sw[k] ACC + sx zw'[k] A[p] + zx' sw[k] B[cls][k] + zx' zw'[k] n_valid  from integer levels
a, b in [-128, 127] (x = sx a + zx', w[k] = sw[k] b + zw'[k]).  With operands that SIT ON the quantisation grids

  activation   range = 255 sx (sx a power of two, so range / 255.f is exact), zero_point zp = (z - 128) sx,
               x = zp + sx (a + 128) = sx (a + z),                              zx' = z sx
  filter row k w[k] = sw_k (b + 128) + mn_k, sw_k cycling through {1/2, 1, 2, 1}, mn_k = (z_k - 128) sw_k, every row
               holding b = -128 and b = 127, so the kernel's own min / max give scale = sw_k exactly; zw'_k = z_k sw_k

the quantisers must recover a and b exactly, and the product is the plain convolution of these very tensors: the
reference is ONE F.conv2d(x, w, stride, padding) in fp64 (zero padding contributes 0, not the zero point), which checks
the int8 GEMM, the window sums A[p], the border classes and the alpha / beta / gamma tables independently of how the
kernel splits the sum.  Exactness per case: B = conv2d(|x| + |zx'|, |w| + |zw'|) bounds each of the four terms of the
epilogue and their partial sums; B / (sx min sw) < 2^24 (helpers.assert_exact_domain) means every fp32 operation of the
epilogue is exact, so the correct output is one bit pattern: the reference itself in fp32, its round-to-nearest-even in
bf16.  Levels come from a narrow band (+-6) with the extremes -128 and 127 planted.

Modes as in test_exact.py: emul = the kernel sources through the TEST-ONLY SIMT emulator, gpu = a real MI355X.
test_qconv_exact_reaches_all_four_instantiations (last) fails if a qconv_i8_kernel instantiation was never launched."""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_exact_domain, assert_not_degenerate, assert_same_values, int_tensor
from test_ops import _dev

F32, BF16 = torch.float32, torch.bfloat16
TAG = {F32: 'f32', BF16: 'bf16'}
SW_CYCLE = (0.5, 1.0, 2.0, 1.0)          # filter scales sw_k
ZW_CYCLE = (0, 1, -2, 3, 2, -1)          # filter zero points zw'_k in units of sw_k
NARROW, WIDE = '1, 4, 2, 1', '2, 2, 2, 2'

SEEN = {'emul': set(), 'gpu': set()}
DONE = {'emul': set(), 'gpu': set()}

# name: ((N, H, W, C, K, R, S, (stride), (pad)), tile the library must pick, sx, modes)
CASES = {
    '1x1-one-chunk': ((2, 5, 6, 16, 8, 1, 1, (1, 1), (0, 0)), NARROW, 1.0, 'eg'),       # minimum K, M < 128
    '3x3-wide-ragged-k72': ((1, 7, 8, 16, 72, 3, 3, (1, 1), (1, 1)), WIDE, 0.5, 'eg'),  # ragged channels, 9 classes
    '3x3-s2-c48': ((2, 8, 7, 48, 24, 3, 3, (2, 2), (1, 1)), NARROW, 2.0, 'eg'),         # 3 chunks per tap, even / odd
    '7x7-s2-p3': ((1, 9, 10, 16, 16, 7, 7, (2, 2), (3, 3)), NARROW, 1.0, 'eg'),         # 49 taps, 20 classes
    'image-smaller-than-window': ((1, 2, 3, 32, 8, 3, 3, (1, 1), (1, 1)), NARROW, 0.5, 'eg'),
    'single-pixel': ((1, 1, 1, 16, 8, 3, 3, (1, 1), (1, 1)), NARROW, 2.0, 'eg'),
    '3x1-k136': ((1, 6, 9, 16, 136, 3, 1, (1, 1), (1, 0)), WIDE, 1.0, 'eg'),            # R != S, 2nd channel tile 8 wide
    '1x1-s2-c144': ((3, 7, 7, 144, 64, 1, 1, (2, 2), (0, 0)), NARROW, 0.5, 'eg'),       # 9 chunks: partial 2nd k-tile
    '5x5-s3': ((1, 12, 11, 16, 8, 5, 5, (3, 3), (2, 2)), NARROW, 2.0, 'eg'),
    '3x1-strides-2-1': ((1, 6, 9, 16, 8, 3, 1, (2, 1), (1, 0)), NARROW, 1.0, 'eg'),
    '1x3-strides-1-2': ((2, 9, 6, 16, 8, 1, 3, (1, 2), (0, 1)), NARROW, 0.5, 'eg'),
    '3x3-strides-2-1': ((1, 8, 8, 16, 8, 3, 3, (2, 1), (1, 1)), NARROW, 2.0, 'eg'),
    # seven pixel tiles with a ragged last one, two channel tiles
    '3x3-c256-k136': ((4, 14, 14, 256, 136, 3, 3, (1, 1), (1, 1)), WIDE, 1.0, 'g'),
    '1x1-s2-c128-k512': ((2, 28, 28, 128, 512, 1, 1, (2, 2), (0, 0)), WIDE, 0.5, 'g'),
}
ACCUM = (1, 4, 4, 512, 8, 3, 3, (1, 1), (1, 1))
SATURATED = (2, 8, 7, 48, 24, 3, 3, (2, 2), (1, 1))


# ---- data on the grids (CPU, built once per configuration and never modified)
def _plant(levels, gen, rate, per_row):
    """Plant the extremes -128 / 127: a share `rate` of all elements, and one of each in every row of the view
    [per_row rows][...] at distinct seeded positions."""
    ext = torch.where(torch.rand(levels.shape, generator=gen) < 0.5, -128, 127)
    levels = torch.where(torch.rand(levels.shape, generator=gen) < rate, ext, levels)
    rows = levels.view(per_row, -1)
    assert rows.shape[1] >= 2
    for r in range(per_row):
        i = torch.randperm(rows.shape[1], generator=gen)[:2]
        rows[r, i[0]], rows[r, i[1]] = -128, 127
    return levels


def _filter_data(K, taps_shape, C, gen, sw=None, zk=None, band=(-6, 6)):
    """Filter levels b [K, *taps_shape, C] (int64), per-row scale sw_k and zero point z_k (in units of sw_k), and the
    fp64 filter w = sw_k (b + z_k): every row holds b = -128 and b = 127."""
    shape = (K,) + tuple(taps_shape) + (C,)
    b = int_tensor(shape, gen, lo=band[0], hi=band[1], density=0.9).long()
    b = _plant(b, gen, 1.0 / 64, K)
    sw = torch.tensor([SW_CYCLE[k % 4] for k in range(K)] if sw is None else [sw] * K, dtype=torch.float64)
    zk = torch.tensor([ZW_CYCLE[k % 6] for k in range(K)] if zk is None else [zk] * K, dtype=torch.float64)
    bc = (K,) + (1,) * (len(shape) - 1)
    w = sw.view(bc) * (b.double() + zk.view(bc))
    return b, sw, zk, w


@functools.lru_cache(maxsize=None)
def _data(cfg, sx, z, kind='grid'):
    """kind: grid (band levels with planted extremes), saturated (every activation level -128), accum (levels in
    [90, 127], all scales 1 and zx' = zw' = 0: sums beyond 2^24)."""
    N, H, W, C, K, R, S, st, pad = cfg
    gen = torch.Generator().manual_seed(977 * H + 131 * W + 7 * C + K + 31 * R + S + int(4 * sx) + 1000 * z)
    if kind == 'accum':
        a = torch.randint(90, 128, (N, H, W, C), generator=gen)
        b, sw, zk, w = _filter_data(K, (R, S), C, gen, sw=1.0, zk=0, band=(90, 127))
        b = torch.where(b == 0, 101, b)                # int_tensor's zeros: keep every level but the planted -128 high
        w = b.double()
    else:
        if kind == 'saturated':
            a = torch.full((N, H, W, C), -128, dtype=torch.int64)
        else:
            a = _plant(int_tensor((N, H, W, C), gen, lo=-6, hi=6, density=0.9).long(), gen, 1.0 / 32, 1)
        b, sw, zk, w = _filter_data(K, (R, S), C, gen)
    assert int(a.min()) >= -128 and int(a.max()) <= 127 and int(b.min()) == -128 and int(b.max()) == 127
    assert bool(((b.view(K, -1) == -128).any(1) & (b.view(K, -1) == 127).any(1)).all())
    zp = (z - 128) * sx
    x = zp + sx * (a.double() + 128)                   # = sx (a + z)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    ref = F.conv2d(nchw(x), nchw(w), None, st, pad).permute(0, 2, 3, 1).contiguous()
    zw = (zk * sw).view(K, 1, 1, 1)
    bound = F.conv2d(nchw(x.abs() + abs(z * sx)), nchw(w.abs() + zw.abs()), None, st, pad).permute(0, 2, 3, 1)
    return dict(a=a, b=b, sw=sw, zk=zk, x=x, w=w, zp=zp, rng=255.0 * sx, ref=ref, bound=bound,
                unit=sx * float(sw.min()))


def _brute_valid(n_in, k, stride, pad, n_out):
    """[n_out][k] bool: tap t of output o reads inside the image."""
    o = torch.arange(n_out).view(-1, 1)
    pos = o * stride - pad + torch.arange(k).view(1, -1)
    return (pos >= 0) & (pos < n_in)


class Ctx(object):
    def __init__(self, mode):
        import convnet_amd as ca
        self.mode, self.dev = mode, _dev(mode)
        self.ca, self.lib, self.L = ca, ca._lib, ca._lib.load()

    def put(self, t, dtype):
        return t.to(dtype).to(self.dev).contiguous()

    def empty(self, shape, dtype, fill):
        return torch.full(tuple(shape) if isinstance(shape, (tuple, list)) else (shape,), fill, dtype=dtype,
                          device=self.dev)

    def stream(self, t):
        return self.lib.stream_of(t)


def _prepare_activation(cx, x, cfg, zp, rng):
    """cn_i8_prepare_activation on the device tensor x (NHWC) -> dict of its outputs and the geometry tables."""
    N, H, W, C, K, R, S, st, pad = cfg
    ptr = cx.lib.ptr
    P, Q = cx.ca.ops.conv_out_hw(H, W, R, S, st, pad)
    rowcls, colcls, ncolcls, clsmask, ncls = cx.ca.quant._i8_geometry(H, W, R, S, st, pad, cx.dev)
    o = dict(P=P, Q=Q, rowcls=rowcls, colcls=colcls, ncolcls=ncolcls, clsmask=clsmask, ncls=ncls,
             zp=torch.tensor([zp], dtype=F32, device=cx.dev), rng=torch.tensor([rng], dtype=F32, device=cx.dev),
             xq=cx.empty((N, H, W, C), torch.int8, 77), chansum=cx.empty(N * H * W, torch.int32, -12345),
             A=cx.empty(N * P * Q, torch.int32, -12345), cls=cx.empty(N * P * Q, torch.uint8, 255))
    cx.L.cn_i8_prepare_activation(ptr(x), ptr(o['xq']), ptr(o['chansum']), ptr(o['A']), ptr(o['cls']), N, H, W, C, R, S,
                                  st[0], st[1], pad[0], pad[1], cx.lib.dtype_code(x.dtype), ptr(o['zp']), ptr(o['rng']),
                                  ptr(rowcls), ptr(colcls), ncolcls, cx.stream(x))
    return o


def _check_activation_prepasses(o, a, cfg, what):
    """xq, chansum, A and cls of one cn_i8_prepare_activation call against plain torch integer arithmetic on the
    expected levels a (int64 NHWC)."""
    N, H, W, C, K, R, S, st, pad = cfg
    P, Q = o['P'], o['Q']
    assert torch.equal(o['xq'].cpu().long(), a), what + ': activation levels'
    cs = a.sum(-1)
    assert torch.equal(o['chansum'].cpu().long().view(N, H, W), cs), what + ': channel sums'
    win = F.conv2d(cs.double().view(N, 1, H, W), torch.ones(1, 1, R, S, dtype=torch.float64), None, st, pad)
    assert tuple(win.shape) == (N, 1, P, Q)
    assert torch.equal(o['A'].cpu().long().view(N, P, Q), win.view(N, P, Q).long()), what + ': window sums A'
    # border classes: the id the host tables define, and - brute force - the class's tap mask is the set of taps of
    # THIS pixel that read inside the image
    cls = o['cls'].cpu().long().view(N, P, Q)
    rc, cc = o['rowcls'].cpu().long(), o['colcls'].cpu().long()
    assert 0 < o['ncls'] <= 255 and int(cls.max()) < o['ncls']
    assert torch.equal(cls, (rc.view(1, P, 1) * o['ncolcls'] + cc.view(1, 1, Q)).expand(N, P, Q)), what + ': class ids'
    vr, vc = _brute_valid(H, R, st[0], pad[0], P), _brute_valid(W, S, st[1], pad[1], Q)
    brute = (vr.view(P, 1, R, 1) & vc.view(1, Q, 1, S)).reshape(1, P, Q, R * S).expand(N, P, Q, R * S)
    assert torch.equal(o['clsmask'].cpu().bool()[cls], brute), what + ': border-class tap masks'


def _prepare_weight(cx, w, K, taps, C):
    ptr = cx.lib.ptr
    wd = cx.put(w.reshape(K, taps, C), F32)
    assert torch.equal(wd.cpu().double(), w.reshape(K, taps, C)), 'the filter does not survive the cast to fp32'
    o = dict(wq=cx.empty(K * taps * C, torch.int8, 77), wsum=cx.empty(K * taps, torch.int32, -12345),
             wpar=cx.empty(K * 2, F32, float('nan')))
    cx.L.cn_i8_prepare_weight(ptr(wd), ptr(o['wq']), ptr(o['wsum']), ptr(o['wpar']), K, taps, C, cx.stream(wd))
    return o


def _check_weight_prepass(o, b, scale, zero, what):
    """wq, wsum and wpar = {scale_k, zero'_k} bit for bit; b: expected levels [K, taps, C] (int64), scale / zero: fp32."""
    K, taps, C = b.shape
    assert torch.equal(o['wq'].cpu().long().view(K, taps, C), b), what + ': filter levels'
    assert torch.equal(o['wsum'].cpu().long().view(K, taps), b.sum(-1)), what + ': filter tap sums'
    wpar = o['wpar'].cpu().view(K, 2)
    assert scale.dtype == F32 and zero.dtype == F32
    assert torch.equal(wpar[:, 0], scale) and torch.equal(wpar[:, 1], zero), what + ': wpar %s' % wpar.tolist()[:4]


def _forward(cx, act, wgt, cfg, out_dtype):
    N, H, W, C, K, R, S, st, pad = cfg
    ptr = cx.lib.ptr
    y = cx.empty((N, act['P'], act['Q'], K), out_dtype, float('nan'))     # an element nobody writes stays NaN
    tables = cx.empty((2 + act['ncls']) * K, F32, float('nan'))
    cx.L.cn_conv2d_fwd_i8(ptr(act['xq']), ptr(wgt['wq']), ptr(y), ptr(act['A']), ptr(act['cls']), ptr(act['zp']),
                          ptr(act['rng']), ptr(wgt['wpar']), ptr(wgt['wsum']), ptr(act['clsmask']), act['ncls'],
                          ptr(tables), N, H, W, C, K, R, S, st[0], st[1], pad[0], pad[1], cx.lib.dtype_code(out_dtype),
                          cx.stream(y))
    name = cx.L.cn_last_kernel_name().decode()
    SEEN[cx.mode].add(name)
    return y, name


def _run(cx, cfg, tile, sx, z, dtype, kind='grid'):
    """The three C entry points on grid data: every pre-pass output and every output element."""
    N, H, W, C, K, R, S, st, pad = cfg
    d = _data(cfg, sx, z, kind)
    what = '%s %s sx=%g z=%d %s' % (kind, cfg, sx, z, TAG[dtype])
    if kind == 'accum':
        top = float(d['ref'].abs().max())
        assert 2.0 ** 24 < top < 2.0 ** 31, top        # beyond fp32's integers, inside int32
        want = d['ref'].long().to(F32)                 # one round-to-nearest-even conversion of the exact integer
        assert dtype == F32 and d['unit'] == 1.0 and z == 0
    else:
        assert_exact_domain(d['bound'] / d['unit'])
        want = d['ref']
        if kind == 'grid':
            if d['ref'].numel() >= 32:
                assert_not_degenerate(d['ref'])
            else:                                      # fewer elements than the 16 distinct values asked for there
                r = d['ref'].flatten()
                assert int((r != 0).sum()) * 2 >= r.numel() and torch.unique(r).numel() * 2 >= r.numel()
    x = cx.put(d['x'], dtype)
    assert torch.equal(x.cpu().double(), d['x']), 'the activation does not survive the cast to %s' % TAG[dtype]
    act = _prepare_activation(cx, x, cfg, d['zp'], d['rng'])
    _check_activation_prepasses(act, d['a'], cfg, what)
    wgt = _prepare_weight(cx, d['w'], K, R * S, C)
    _check_weight_prepass(wgt, d['b'].view(K, R * S, C), d['sw'].float(), (d['zk'] * d['sw']).float(), what)
    y, name = _forward(cx, act, wgt, cfg, dtype)
    assert name == 'qconv_i8_kernel<%s, %s>' % (tile, 'true' if dtype == F32 else 'false'), name
    assert_same_values(y, want, dtype, what + ' ' + name)


# =====================================================================================================================
# 1. pre-passes beyond the grid data of the main cases
@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=lambda d: TAG[d])
def test_levels_round_ties_to_even_and_clamp(mode, dtype):
    """qi_levels_kernel at scale 1: x = zp + k + 0.5 for every k of 0..254 must round half to even (torch.round), and
    values below zp / above zp + range clamp to the levels -128 / 127."""
    cx = Ctx(mode)
    zp = -128.0
    ties = zp + torch.arange(255, dtype=torch.float64) + 0.5
    # (all of these have at most 8 significant bits: bf16 holds them)
    outside = torch.tensor([-129, -130, -256, -1024, 127.5, 128, 129, 8192,                  # below zp, above zp + range
                            -128, 127, -31.25, 31.75, 0.375, -0.625, 1, 2, 3], dtype=torch.float64)
    cfg = (1, 1, 17, 16, 8, 1, 1, (1, 1), (0, 0))
    x64 = torch.cat([ties, outside]).view(1, 1, 17, 16)
    x = cx.put(x64, dtype)
    assert torch.equal(x.cpu().double(), x64), 'the tie values must survive the cast to %s' % TAG[dtype]
    t = (x64 - zp).clamp(0, 255)
    assert int(((t - t.floor()) == 0.5).sum()) == 255 and int((x64 < zp).sum()) == 4 and int((x64 > zp + 255).sum()) == 4
    want = torch.round(t).long() - 128               # torch.round: half to even
    assert int(want[0, 0, 0, 0]) == -128 and int(want[0, 0, 0, 1]) == -126    # 0.5 -> 0, 1.5 -> 2
    act = _prepare_activation(cx, x, cfg, zp, 255.0)
    _check_activation_prepasses(act, want, cfg, 'ties and clamping, %s' % TAG[dtype])


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
def test_weight_prepass_special_rows(mode):
    """qi_weight_kernel: a constant row (range 0 -> 1: scale 1/255, every level -128), C = 272 (more than one element
    per thread) and C = 16 with one tap (240 idle threads)."""
    cx = Ctx(mode)
    g = torch.Generator().manual_seed(5)
    for K, taps, C in ((4, 2, 272), (8, 1, 16), (5, 3, 48)):
        b, sw, zk, w = _filter_data(K, (taps,), C, g)
        scale, zero = sw.float(), (zk * sw).float()
        w[1] = 0.75                                    # a constant row
        b[1] = -128
        scale[1] = torch.tensor(1.0, dtype=F32) / 255.0
        zero[1] = torch.tensor(0.75, dtype=F32) + 128.0 * scale[1]       # 128 * scale is exact: one rounding
        o = _prepare_weight(cx, w, K, taps, C)
        _check_weight_prepass(o, b, scale, zero, 'K=%d taps=%d C=%d' % (K, taps, C))


# =====================================================================================================================
# 2. the main kernel, all four instantiations
def _params():
    out = []
    for name, (cfg, tile, sx, modes) in CASES.items():
        for mode in (('emul',) if 'e' in modes else ()) + ('gpu',):
            for dtype in (F32, BF16):
                for z in (0, 3):
                    out.append(pytest.param(mode, name, dtype, z, id='%s-%s-%s-z%d' % (mode, name, TAG[dtype], z),
                                            marks=[pytest.mark.gpu] if mode == 'gpu' else []))
    return out


def _run_case(mode, name, dtype, z):
    cfg, tile, sx, _ = CASES[name]
    _run(Ctx(mode), cfg, tile, sx, z, dtype)
    DONE[mode].add((name, dtype, z))


@pytest.mark.parametrize('mode,name,dtype,z', _params())
def test_qconv_exact(mode, name, dtype, z):
    _run_case(mode, name, dtype, z)


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=lambda d: TAG[d])
def test_qconv_exact_saturated_activation(mode, dtype):
    """Every activation level is -128 (x = zp everywhere), random filters: the GEMM term is at its most negative and
    the borders differ only through the class tables.  (No degeneracy claim: the interior is constant by design.)"""
    _run(Ctx(mode), SATURATED, NARROW, 2.0, 3, dtype, kind='saturated')


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
def test_qconv_accumulates_in_int32(mode):
    """Levels in [90, 127], 4608 products per output, scales 1, zx' = zw' = 0: the sums reach about 5e7 > 2^24, where
    an fp32 accumulation would round along the way.  The fp32 output must be the exact integer converted once."""
    _run(Ctx(mode), ACCUM, NARROW, 1.0, 0, F32, kind='accum')


# =====================================================================================================================
# 3. geometry code of quant.py: CPU only, no library
def test_border_classes_against_brute_force():
    """Tap t of output o lies in its class's [lo, hi] iff it reads inside the image: 0 <= o stride - pad + t < n_in."""
    from convnet_amd.quant import _border_classes
    n = 0
    for n_in in range(1, 13):
        for k in range(1, 8):
            for stride in range(1, 4):
                for pad in range(0, k // 2 + 1):
                    n_out = (n_in + 2 * pad - k) // stride + 1
                    if n_out <= 0:
                        continue
                    ids, pats = _border_classes(n_in, k, stride, pad, n_out)
                    assert len(ids) == n_out and len(set(pats)) == len(pats) and set(ids) == set(range(len(pats)))
                    lo = torch.tensor([pats[i][0] for i in ids]).view(-1, 1)
                    hi = torch.tensor([pats[i][1] for i in ids]).view(-1, 1)
                    t = torch.arange(k).view(1, -1)
                    assert torch.equal((lo <= t) & (t <= hi), _brute_valid(n_in, k, stride, pad, n_out)), \
                        (n_in, k, stride, pad)
                    n += 1
    assert n > 500                                     # the sweep is not empty


@pytest.mark.parametrize('geom', [(7, 8, 3, 3, (1, 1), (1, 1)), (9, 10, 7, 7, (2, 2), (3, 3)), (2, 3, 3, 3, (1, 1), (1, 1)),
                                  (1, 1, 3, 3, (1, 1), (1, 1)), (6, 9, 3, 1, (2, 1), (1, 0)), (9, 6, 1, 3, (1, 2), (0, 1)),
                                  (12, 11, 5, 5, (3, 2), (2, 1)), (8, 12, 7, 4, (1, 3), (3, 2)), (5, 5, 1, 1, (2, 2), (0, 0))])
def test_i8_geometry_against_brute_force(geom):
    """rowcls / colcls / clsmask of quant._i8_geometry: the mask row of (rowcls[p], colcls[q]) is the set of taps
    (r, s) that read inside the image at output pixel (p, q); at most 255 classes (they are stored as bytes)."""
    from convnet_amd.quant import _i8_geometry
    H, W, R, S, st, pad = geom
    P, Q = (H + 2 * pad[0] - R) // st[0] + 1, (W + 2 * pad[1] - S) // st[1] + 1
    rowcls, colcls, ncolcls, clsmask, ncls = _i8_geometry(H, W, R, S, st, pad, 'cpu')
    assert rowcls.dtype == colcls.dtype == clsmask.dtype == torch.uint8
    assert tuple(rowcls.shape) == (P,) and tuple(colcls.shape) == (Q,) and tuple(clsmask.shape) == (ncls, R * S)
    assert 0 < ncls <= 255 and ncolcls == int(colcls.max()) + 1 and ncls == (int(rowcls.max()) + 1) * ncolcls
    cls = rowcls.long().view(P, 1) * ncolcls + colcls.long().view(1, Q)
    vr, vc = _brute_valid(H, R, st[0], pad[0], P), _brute_valid(W, S, st[1], pad[1], Q)
    assert torch.equal(clsmask.bool()[cls], (vr.view(P, 1, R, 1) & vc.view(1, Q, 1, S)).reshape(P, Q, R * S))


# =====================================================================================================================
# 4. module level: QConv2d.int8_forward through conv2d_fwd_int8, the measured range and the geometry cache
@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=lambda d: TAG[d])
def test_qconv2d_int8_forward_is_exact_on_grid_data(mode, dtype):
    """A 16 -> 24, 3x3, stride-2 QConv2d in training mode on grid data whose every sample holds its min and its max,
    so the measured (zero point, range) are exactly (zp, 255 sx): the module's output is the fp64 convolution."""
    cx = Ctx(mode)
    ca = cx.ca
    N, H, W, C, K, R, st, pad, sx, z = 4, 7, 8, 16, 24, 3, 2, 1, 0.5, 3
    g = torch.Generator().manual_seed(2024)
    a = _plant(int_tensor((N, H, W, C), g, lo=-6, hi=6, density=0.9).long(), g, 1.0 / 32, N)
    assert bool(((a.view(N, -1) == -128).any(1) & (a.view(N, -1) == 127).any(1)).all())
    b, sw, zk, w = _filter_data(K, (R, R), C, g)
    x64 = sx * (a.double() + z)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    ref = F.conv2d(nchw(x64), nchw(w), None, st, pad).permute(0, 2, 3, 1).contiguous()
    bound = F.conv2d(nchw(x64.abs() + z * sx), nchw(w.abs() + (zk * sw).abs().view(K, 1, 1, 1)), None, st, pad)
    assert_exact_domain(bound / (sx * float(sw.min())))
    assert_not_degenerate(ref)
    conv = ca.quant.QConv2d(C, K, R, stride=st, padding=pad, bias=False)
    with torch.no_grad():
        conv.weight.copy_(nchw(w).float())
    ca.engine.prepare(conv, cx.dev, dtype)
    conv.train()
    conv.int8_forward = True
    x = cx.put(x64, dtype)
    assert torch.equal(x.cpu().double(), x64)
    for _ in range(2):                                 # the second call takes the geometry from the cache
        cx.L.cn_kernel_log(1)
        with torch.no_grad():
            y = conv(x)
        names = [n for n in cx.L.cn_kernel_log(0).decode().split(';') if n] or [cx.L.cn_last_kernel_name().decode()]
        expect = 'qconv_i8_kernel<%s, %s>' % (NARROW, 'true' if dtype == F32 else 'false')
        assert expect in names, names
        SEEN[mode].update(n for n in names if 'qconv' in n)
        assert_same_values(y, ref, dtype, 'QConv2d int8_forward %s' % TAG[dtype])


# =====================================================================================================================
# 5. refusals: argument checks before any launch
@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
def test_refusals_leave_the_output_untouched(mode):
    cx = Ctx(mode)
    ptr, Err = cx.lib.ptr, cx.lib.ConvNetHipError
    cfg = (1, 4, 5, 32, 16, 3, 3, (1, 1), (1, 1))
    N, H, W, C, K, R, S, st, pad = cfg
    d = _data(cfg, 1.0, 3)
    x = cx.put(d['x'], F32)
    act = _prepare_activation(cx, x, cfg, d['zp'], d['rng'])
    wgt = _prepare_weight(cx, d['w'], K, R * S, C)
    y, _ = _forward(cx, act, wgt, cfg, F32)
    assert_same_values(y, d['ref'], F32, 'the valid call the refusals are derived from')
    tables = cx.empty((2 + 256) * K, F32, 0.0)
    big = cx.empty(81 * K * C, torch.int8, 0)          # operands large enough for the 9x9 call, were it launched

    def fwd(what, **kw):
        a = dict(xq=act['xq'], wq=wgt['wq'], A=act['A'], cls=act['cls'], wpar=wgt['wpar'], wsum=wgt['wsum'],
                 clsmask=act['clsmask'], ncls=act['ncls'], C=C, K=K, R=R, S=S, pad=pad, out=cx.lib.F32)
        a.update(kw)
        yy = cx.empty(y.numel() * 8, F32, -7.0)
        with pytest.raises(Err) as e:
            cx.L.cn_conv2d_fwd_i8(ptr(a['xq']), ptr(a['wq']), ptr(yy), ptr(a['A']), ptr(a['cls']), ptr(act['zp']),
                                  ptr(act['rng']), ptr(a['wpar']), ptr(a['wsum']), ptr(a['clsmask']), a['ncls'],
                                  ptr(tables), N, H, W, a['C'], a['K'], a['R'], a['S'], st[0], st[1], a['pad'][0],
                                  a['pad'][1], a['out'], cx.stream(yy))
        assert 'cn_conv2d_fwd_i8 failed (rc=-' in str(e.value) and 'conv2d_fwd_i8: ' in str(e.value), (what, str(e.value))
        assert cx.lib.last_error().startswith('conv2d_fwd_i8: '), what
        assert bool((yy.cpu() == -7.0).all()), what + ': the output buffer was written'

    fwd('C = 24', C=24)
    fwd('K = 12', K=12)
    fwd('9x9 taps', R=9, S=9, pad=(4, 4), wq=big)
    fwd('ncls = 0', ncls=0)
    fwd('ncls = 256', ncls=256)
    fwd('fp16 output', out=cx.lib.F16)
    for name in ('xq', 'wq', 'A', 'cls', 'wpar', 'wsum', 'clsmask'):
        fwd('null ' + name, **{name: None})

    def prep(what, x_=x, C_=C, dt=cx.lib.F32, rowcls=act['rowcls']):
        q = cx.empty(x.numel(), torch.int8, 77)
        with pytest.raises(Err) as e:
            cx.L.cn_i8_prepare_activation(ptr(x_), ptr(q), ptr(act['chansum']), ptr(act['A']), ptr(act['cls']), N, H, W,
                                          C_, R, S, st[0], st[1], pad[0], pad[1], dt, ptr(act['zp']), ptr(act['rng']),
                                          ptr(rowcls), ptr(act['colcls']), act['ncolcls'], cx.stream(x))
        assert 'i8_prepare_activation: ' in str(e.value), (what, str(e.value))
        assert bool((q.cpu() == 77).all()), what + ': the level buffer was written'

    prep('C = 24', C_=24)
    prep('null x', x_=None)
    prep('null rowcls', rowcls=None)
    prep('fp16 input', dt=cx.lib.F16)

    wq = cx.empty(K * R * S * C, torch.int8, 77)
    with pytest.raises(Err) as e:
        cx.L.cn_i8_prepare_weight(None, ptr(wq), ptr(wgt['wsum']), ptr(wgt['wpar']), K, R * S, C, cx.stream(wq))
    assert 'i8_prepare_weight: ' in str(e.value)
    assert bool((wq.cpu() == 77).all())


# =====================================================================================================================
# 6. reach
KERNELS = ['qconv_i8_kernel<%s, %s>' % (t, f) for t in (NARROW, WIDE) for f in ('true', 'false')]


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
def test_qconv_exact_reaches_all_four_instantiations(mode):
    """Each of the four qconv_i8_kernel instantiations was launched by an exact case of this file (cases that did not
    run in this process - a selection with -k - are run here first)."""
    _dev(mode)
    for p in _params():
        m, name, dtype, z = p.values
        if m == mode and (name, dtype, z) not in DONE[mode]:
            _run_case(mode, name, dtype, z)
    missing = [k for k in KERNELS if k not in SEEN[mode]]
    assert not missing, 'instantiations no exact case reached: %s\nseen: %s' % (missing, sorted(SEEN[mode]))
    assert all(n in KERNELS for n in SEEN[mode]), sorted(SEEN[mode])
