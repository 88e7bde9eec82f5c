"""Bit-exact checks of every convolution-class kernel on integer data, element by element.

With small-integer inputs every product and every partial sum of a convolution is an integer below 2^24, so an fp32
accumulation is exact in ANY summation order, tile shape or split count.  The correct result is therefore one fixed bit
pattern - the integer itself for fp32 outputs, its round-to-nearest-even for bf16 / fp16 outputs - and the reference is
plain torch on the CPU (fp64; exact fp32 at the training batch).  Every case

  * proves it stays in that domain (helpers.assert_exact_domain on the magnitude sums: the same operation on |inputs|),
  * refuses degenerate data (helpers.assert_not_degenerate: half the reference non-zero, 16 distinct values),
  * compares EVERY output element by value (helpers.assert_same_values: the failure message carries the count, the
    first indices and histograms by image / border / 8-channel chunk), and
  * records the kernel instantiation(s) the library launched; test_exact_sweep_reaches_every_kernel_family (last in
    this file) fails if a family listed there was never reached.

Coefficients of the fused epilogues and operand-side transforms are small integers or powers of two, so the fused
arithmetic is exact too (values that are multiples of 1/2 are handled by scaling the domain check by 2).

Modes as in test_ops.py: emul = the kernel sources through the TEST-ONLY SIMT emulator, gpu = a real MI355X."""
import contextlib
import re

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_exact_domain, assert_not_degenerate, assert_same_values, int_tensor
from test_gconv import EMUL_CASES as GCONV_EMUL, _shapes_resnext
from test_headline_parity import BIG_KERNELS, BIG_LAYERS
from test_ops import CONV_EMUL, CONV_GPU, _dev

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
HALF = [BF16, F16]
TAG = {F32: 'f32', BF16: 'bf16', F16: 'f16'}

# kernel names seen after the exact launches, per mode
SEEN = {'emul': set(), 'gpu': set()}
DONE = {'emul': set(), 'gpu': set()}

# defaults of the library's variant knobs (csrc: cn_get_option); every forced knob is put back in a `finally`
KNOB_DEFAULT = {'igemm_256sq': -1, 'igemm_variant': 0, 'igemm_8w': 16, 'wgrad_3x3': 1, 'wgrad_variant': 0,
                'conv3x3_wgs': 512, 'jbwd_splits': 256, 'jdgrad_splits': 256, 'stem_wgrad_wgs': 256, 'dense_smallm': 1}


class Ctx(object):
    """mode, device, library handle and the kernel-name recorder of one case."""

    def __init__(self, mode):
        import convnet_amd as ca
        self.mode, self.dev = mode, _dev(mode)
        self.ca, self.ops, self.lib, self.L = ca, ca.ops, ca._lib, ca._lib.load()
        self.names = []

    def begin(self):
        self.L.cn_kernel_log(1)

    def note(self, expect=None):
        """Record the GEMM-class kernels launched since begin(); `expect`: substring one of them must carry."""
        names = [n for n in self.L.cn_kernel_log(0).decode().split(';') if n] or [self.L.cn_last_kernel_name().decode()]
        self.names = names
        SEEN[self.mode].update(names)
        if expect is not None:
            assert any(expect in n for n in names), (expect, names)
        return names

    @contextlib.contextmanager
    def knobs(self, flags=None, **kw):
        """Library options (cn_set_option) and ops-module switches, restored on exit."""
        saved = {k: getattr(self.ops, k) for k in (flags or {})}
        try:
            for k, v in kw.items():
                self.L.cn_set_option(k.encode(), v)
            for k, v in (flags or {}).items():
                setattr(self.ops, k, v)
            yield
        finally:
            for k in kw:
                self.L.cn_set_option(k.encode(), KNOB_DEFAULT[k])
            for k, v in saved.items():
                setattr(self.ops, k, v)

    def put(self, t, dtype):
        return t.to(dtype).to(self.dev).contiguous()


def _ints(shape, gen, f32=False, **kw):
    """int_tensor; f32: built in slices of the leading dimension and kept in fp32 (the N=256 operands)."""
    shape = tuple(shape)
    if not f32:
        return int_tensor(shape, gen, **kw)
    out = torch.empty(shape, dtype=torch.float32)
    per = 1
    for s in shape[1:]:
        per *= s
    step = max(1, (1 << 23) // per)
    for i in range(0, shape[0], step):
        n = min(step, shape[0] - i)
        out[i:i + n] = int_tensor((n,) + shape[1:], gen, **kw)
    return out


# ---- references on NHWC / KRSC tensors (torch CPU, the dtype of the operands: fp64, or fp32 where stated)
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def ref_fwd(x, w, st, pad, groups=1):
    return F.conv2d(_nchw(x), _nchw(w), None, st, pad, 1, groups).permute(0, 2, 3, 1)


def ref_dgrad(dy, w, x_shape, st, pad, groups=1):
    N, H, W, C = x_shape
    return torch.nn.grad.conv2d_input((N, C, H, W), _nchw(w), _nchw(dy), st, pad, 1, groups).permute(0, 2, 3, 1)


def ref_wgrad(x, dy, w_shape, st, pad, groups=1):
    K, R, S, Cg = w_shape
    return torch.nn.grad.conv2d_weight(_nchw(x), (K, Cg, R, S), _nchw(dy), st, pad, 1, groups).permute(0, 2, 3, 1)


def _triple(fn, a, b, *args, unit=1.0, what=''):
    """The exact reference fn(a, b), proven exact: the magnitude sums stay below 2^24 (in units of `unit`, the
    spacing of the values), the reference is not degenerate, and an fp32 evaluation equals the fp64 one."""
    ref = fn(a, b, *args)
    A = fn(a.abs(), b.abs(), *args)
    assert_exact_domain(A / unit)
    if a.dtype == torch.float64:
        assert torch.equal(fn(a.float(), b.float(), *args).double(), ref), 'fp32 reference != fp64 reference: ' + what
    return ref, A


def _support(ref, R, st):
    """The elements a data gradient can reach: a strided 1x1 leaves the pixels between the samples structurally zero
    (they are still compared; only the degeneracy check looks at the sampled ones)."""
    return ref[:, ::st, ::st] if (R == 1 and st > 1) else ref


def conv_exact(cx, cfg, dtypes, which=('fwd', 'dgrad', 'wgrad'), seed=0, big=False, expect=(None, None, None)):
    """conv2d_fwd / conv2d_dgrad / conv2d_wgrad on integer data against the exact reference, every element, for each
    dtype of `dtypes` (integers up to 3 are exact in all of them, so one reference serves all).
    big: operands and reference in fp32 (exact: the analytic magnitude bound n * max|a| * max|b| is below 2^24)."""
    ops = cx.ops
    dtypes = dtypes if isinstance(dtypes, (list, tuple)) else [dtypes]
    N, H, W, C, K, R, st, pad = cfg
    P, Q = ops.conv_out_hw(H, W, R, R, (st, st), (pad, pad))
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + C + K)
    x = _ints((N, H, W, C), g, f32=big)
    w = _ints((K, R, R, C), g)
    dy = _ints((N, P, Q, K), g, f32=big)
    if big:
        w = w.float()

    def reference(fn, a, b, n, *args):
        if big:       # |values| <= 3: every magnitude sum is at most 9 n
            assert_exact_domain(torch.tensor(9.0 * n))
            return fn(a, b, *args)
        return _triple(fn, a, b, *args, what=str(cfg))[0]

    refs = {}
    if 'fwd' in which:
        refs['fwd'] = reference(ref_fwd, x, w, C * R * R, st, pad)
        assert_not_degenerate(refs['fwd'])
    if 'dgrad' in which:
        refs['dgrad'] = reference(ref_dgrad, dy, w, K * R * R, (N, H, W, C), st, pad)
        assert_not_degenerate(_support(refs['dgrad'], R, st))
    if 'wgrad' in which:
        refs['wgrad'] = reference(ref_wgrad, x, dy, N * P * Q, (K, R, R, C), st, pad)
        assert_not_degenerate(refs['wgrad'])
    for dtype in dtypes:
        if dtype != F32 and C % 8:
            continue
        what = '%s %s' % (cfg, TAG[dtype])
        xh, wk, dyh = cx.put(x, dtype), cx.put(w, dtype), cx.put(dy, dtype)
        wc = cx.put(w.permute(3, 1, 2, 0), dtype)
        if 'fwd' in which:
            cx.begin()
            y = ops.conv2d_fwd(xh, wk, None, K, R, R, (st, st), (pad, pad))
            cx.note(expect[0])
            assert_same_values(y, refs['fwd'], dtype, 'fwd ' + what + ' ' + str(cx.names))
        if 'dgrad' in which:
            cx.begin()
            dx = ops.conv2d_dgrad(dyh, wc, (N, H, W, C), K, R, R, (st, st), (pad, pad))
            cx.note(expect[1])
            assert_same_values(dx, refs['dgrad'], dtype, 'dgrad ' + what + ' ' + str(cx.names))
        if 'wgrad' in which:
            dw = torch.full((K, R, R, C), float('nan'), dtype=torch.float32, device=cx.dev)    # beta = 0 must not read it
            cx.begin()
            ops.conv2d_wgrad(xh, dyh, dw, C, K, R, R, (st, st), (pad, pad), beta=0.0)
            cx.note(expect[2])
            assert_same_values(dw, refs['wgrad'], F32, 'wgrad ' + what + ' ' + str(cx.names))


# =====================================================================================================================
# the case registry: (name, modes, function(cx)); one pytest case each, and the coverage test re-runs what was skipped
CASES = []


def case(name, modes=('emul', 'gpu')):
    def deco(fn):
        CASES.append((name, tuple(modes), fn))
        return fn
    return deco


# ---- 2. plain entry points
# ragged shapes for the emulator: odd maps, N*P*Q % 128 != 0, K just under / over a channel tile, C = 8; one single-image
# 56 x 56 64 -> 64 3x3 (the halo kernel) and one 1x1 64 -> 256 (the streaming kernel)
RAGGED_EMUL = [(1, 11, 13, 8, 72, 3, 1, 1), (3, 7, 9, 24, 136, 3, 2, 1), (2, 5, 5, 8, 8, 1, 1, 0),
               (1, 13, 3, 8, 136, 1, 1, 0)]
HALO_EMUL = (1, 56, 56, 64, 64, 3, 1, 1)
STREAM_EMUL = (1, 12, 11, 64, 256, 1, 1, 0)


def _reg_plain():
    for dt in DTYPES:
        def run(cx, dt=dt):
            for cfg in CONV_EMUL + RAGGED_EMUL:
                conv_exact(cx, cfg, dt)
        case('plain-%s' % TAG[dt], ('emul',))(run)

    def halo(cx):
        conv_exact(cx, HALO_EMUL, BF16, which=('fwd',), expect=('conv3x3_c64_kernel<bf16_t>', None, None))
        conv_exact(cx, (1, 20, 56, 64, 64, 3, 1, 1), F16, which=('dgrad',), expect=(None, 'conv3x3_c64_kernel<f16_t> [dgrad]', None))
    case('plain-halo3x3', ('emul',))(halo)

    def stream(cx):
        for dt in HALF:
            conv_exact(cx, STREAM_EMUL, dt, expect=('jfwd_kernel', None, None))
    case('plain-stream1x1', ('emul',))(stream)

    for cfg in CONV_GPU:
        def run(cx, cfg=cfg):
            conv_exact(cx, cfg, DTYPES)
        case('plain-n2-%dx%d_%d_%d_%dx%d_s%d' % (cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], cfg[5], cfg[6]), ('gpu',))(run)

    big_f32 = [(64, 56, 64, 3, 1, 1), (256, 56, 64, 1, 1, 0), (512, 7, 512, 3, 1, 1)]
    for lay in BIG_LAYERS:
        for dt in [BF16] + ([F32] if lay in big_f32 else []):
            def run(cx, lay=lay, dt=dt):
                C, H, K, R, st, pad = lay
                exp = BIG_KERNELS.get(lay, (None, None, None)) if dt == BF16 else (None, None, None)
                conv_exact(cx, (256, H, H, C, K, R, st, pad), dt, big=True, expect=exp)
            case('plain-n256-%d_%d_%d_%dx%d_s%d-%s' % (lay[0], lay[1], lay[2], lay[3], lay[3], lay[4], TAG[dt]), ('gpu',))(run)


_reg_plain()


# ---- forced variants, each against the reference (never against its sibling)
def _T(cfg):
    """The transposed problem: its dgrad has the forward's output width (so the same tile choice)."""
    N, H, W, C, K, R, st, pad = cfg
    return (N, H, W, K, C, R, st, pad)


@case('variant-igemm-tiles')
def _variant_igemm(cx):
    emul = cx.mode == 'emul'
    big = [(2, 12, 12, 16, 256, 3, 1, 1), (1, 18, 17, 64, 384, 1, 1, 0)] if emul else \
        [(8, 14, 14, 256, 256, 3, 1, 1), (6, 14, 14, 1024, 256, 1, 1, 0), (4, 28, 28, 256, 256, 3, 2, 1),
         (3, 14, 15, 512, 384, 1, 1, 0)]
    dma = [(2, 8, 9, 24, 128, 3, 1, 1), (1, 6, 6, 40, 192, 3, 2, 1)] if emul else \
        [(5, 7, 7, 512, 512, 3, 1, 1), (4, 7, 7, 2048, 512, 1, 1, 0), (3, 14, 15, 72, 384, 1, 1, 0)]
    narrow = [(1, 8, 8, 32, 40, 1, 2, 0), (2, 8, 8, 16, 64, 3, 1, 1)] if emul else \
        [(4, 56, 56, 256, 64, 1, 1, 0), (3, 17, 13, 64, 40, 3, 2, 1)]
    for dt in HALF:
        if emul and dt == F16:
            big, dma, narrow = big[:1], dma[:1], narrow[:1]
        for cfg in big:      # the 256 x 256 tile
            with cx.knobs(igemm_256sq=1):
                conv_exact(cx, cfg, dt, which=('fwd',), expect=('4, 2, 2, 4, 2,', None, None))
                conv_exact(cx, _T(cfg), dt, which=('dgrad',), expect=(None, '4, 2, 2, 4, 2,', None))
            with cx.knobs(igemm_256sq=0):
                conv_exact(cx, cfg, dt, which=('fwd',))
                assert not any('4, 2, 2, 4, 2,' in n for n in cx.names), cx.names
        for cfg in dma:      # the 128 x 128 LDS-DMA tile with interleaved issue
            with cx.knobs(igemm_variant=3, igemm_256sq=0):
                conv_exact(cx, cfg, dt, which=('fwd',), expect=('2, 2, 2, 2, 2, false, true, true,', None, None))
                conv_exact(cx, _T(cfg), dt, which=('dgrad',), expect=(None, '2, 2, 2, 2, 2, false, true, true,', None))
            with cx.knobs(igemm_variant=1, igemm_256sq=0, igemm_8w=0):     # register-staged, four waves
                conv_exact(cx, cfg, dt, which=('fwd',), expect=('2, 2, 2, 2, 1, false, false,', None, None))
                conv_exact(cx, _T(cfg), dt, which=('dgrad',), expect=(None, '2, 2, 2, 2, 1, false, false,', None))
            with cx.knobs(igemm_variant=1, igemm_256sq=0, igemm_8w=1 << 20):   # register-staged, eight waves
                conv_exact(cx, cfg, dt, which=('fwd',), expect=('2, 4, 2, 1, 1, false, false, false, false,', None, None))
        for cfg in narrow:   # the 64-channel tile, register-staged and LDS-DMA
            for v, tag in ((1, '1, 4, 2, 1, 1, false, false,'), (3, '1, 4, 2, 1, 2, false, true,')):
                with cx.knobs(igemm_variant=v):
                    conv_exact(cx, cfg, dt, which=('fwd',), expect=(tag, None, None))
                    conv_exact(cx, _T(cfg), dt, which=('dgrad',), expect=(None, tag, None))
    with cx.knobs(igemm_variant=3):    # fp32 storage through the LDS-DMA form of the generic tile
        conv_exact(cx, dma[0], F32, which=('fwd',), expect=('float, 2, 2, 2, 2, 2, true, true,', None, None))


@case('variant-wgrad-kernels')
def _variant_wgrad(cx):
    emul = cx.mode == 'emul'
    # 3x3 / stride 1: the band kernel and the tile kernels on the same shapes
    c3 = [(3, 5, 6, 32, 64), (2, 9, 7, 64, 128), (5, 3, 4, 96, 64), (7, 2, 3, 32, 64)] if emul else \
        [(64, 28, 28, 128, 128), (37, 14, 14, 256, 256), (61, 7, 7, 512, 512), (5, 28, 20, 96, 192), (3, 9, 31, 32, 64),
         (16, 56, 56, 64, 128)]
    for dt in HALF:
        for (N, H, W, C, K) in (c3[:1] if (emul and dt == F16) else c3):
            cfg = (N, H, W, C, K, 3, 1, 1)
            with cx.knobs(wgrad_3x3=1):
                conv_exact(cx, cfg, dt, which=('wgrad',), expect=(None, None, 'wgrad3x3_kernel'))
            with cx.knobs(wgrad_3x3=0):
                conv_exact(cx, cfg, dt, which=('wgrad',), expect=(None, None, 'wgrad_kernel'))
    # 1x1 and strided: the LDS-DMA kernel (where the dispatcher takes it) and the register-staged one
    c1 = [(3, 5, 5, 64, 136, 1, 1, 0), (2, 8, 8, 128, 128, 1, 1, 0), (1, 9, 7, 16, 72, 3, 2, 1), (2, 8, 8, 32, 136, 1, 2, 0)] \
        if emul else [(8, 56, 56, 64, 256, 1, 1, 0), (8, 14, 14, 1024, 256, 1, 1, 0), (4, 7, 7, 2048, 512, 1, 1, 0),
                      (4, 56, 56, 128, 128, 3, 2, 1), (4, 56, 56, 256, 512, 1, 2, 0), (3, 17, 13, 64, 72, 3, 2, 1)]
    for dt in DTYPES:
        for cfg in (c1[:2] if (emul and dt == F16) else c1):
            for v in (0, 1):
                with cx.knobs(wgrad_variant=v):
                    dma = dt == BF16 and v == 0 and cfg[5:] == (1, 1, 0) and cfg[4] > 64
                    conv_exact(cx, cfg, dt, which=('wgrad',), expect=(None, None, 'wgrad_dma_kernel' if dma else 'wgrad_kernel'))


@case('variant-halo-and-streaming')
def _variant_halo_stream(cx):
    emul = cx.mode == 'emul'
    halo = [(1, 9, 7, 2), (2, 5, 12, 256)] if emul else [(4, 56, 56, 256), (3, 13, 21, 5), (2, 9, 56, 512)]
    for dt in HALF:
        for (N, H, W, wgs) in halo:
            cfg = (N, H, W, 64, 64, 3, 1, 1)
            with cx.knobs(flags={'CONV3X3_HALO': True}, conv3x3_wgs=wgs):
                conv_exact(cx, cfg, dt, which=('fwd', 'dgrad'),
                           expect=('conv3x3_c64_kernel', 'conv3x3_c64_kernel', None))
            with cx.knobs(flags={'CONV3X3_HALO': False}):
                conv_exact(cx, cfg, dt, which=('fwd', 'dgrad'), expect=('igemm_kernel', 'igemm_kernel', None))
    stream = [(1, 6, 10, 64, 256), (2, 6, 6, 128, 256), (1, 5, 9, 128, 512), (1, 5, 7, 256, 1024)] if emul else \
        [(8, 56, 56, 64, 256), (8, 56, 56, 128, 256), (16, 28, 28, 128, 512), (3, 17, 13, 64, 256), (64, 14, 14, 256, 1024)]
    for dt in HALF:
        for (N, H, W, C, K) in (stream[:2] if (emul and dt == F16) else stream):
            cfg = (N, H, W, C, K, 1, 1, 0)
            with cx.knobs(flags={'CONV1X1_STREAM': True}):
                conv_exact(cx, cfg, dt, which=('fwd',), expect=('jfwd_kernel', None, None))
            with cx.knobs(flags={'CONV1X1_STREAM': False}):
                conv_exact(cx, cfg, dt, which=('fwd',), expect=('igemm_kernel', None, None))


# ---- 3. epilogues and operand-side fusions
def _small(shape, g, **kw):
    kw.setdefault('lo', -2)
    kw.setdefault('hi', 2)
    return int_tensor(shape, g, **kw)


def _pow2(n, g):
    """per-channel scale in {0.5, 1, 2}"""
    return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]


@case('epilogue-fwd-bias-relu-f32')
def _epi_fwd(cx):
    ops = cx.ops
    cfgs = [(2, 8, 8, 16, 64, 3, 1, 1), (1, 9, 7, 16, 72, 3, 2, 1), (3, 5, 5, 64, 136, 1, 1, 0)] if cx.mode == 'emul' else \
        [(2, 56, 56, 64, 64, 3, 1, 1), (2, 28, 28, 512, 256, 1, 1, 0), (3, 17, 13, 64, 72, 3, 2, 1), (2, 14, 14, 256, 1024, 1, 1, 0)]
    for dt in DTYPES:
        for (N, H, W, C, K, R, st, pad) in cfgs:
            g = torch.Generator().manual_seed(H + K)
            x, w = int_tensor((N, H, W, C), g), int_tensor((K, R, R, C), g)
            bias = int_tensor((K,), g, lo=-5, hi=5, density=0.8)
            conv, A = _triple(ref_fwd, x, w, st, pad)
            assert_exact_domain(A + 5)
            xh, wk, bh = cx.put(x, dt), cx.put(w, dt), cx.put(bias, F32)
            for relu in (False, True):
                for out_f32 in (False, True):
                    ref = conv + bias
                    ref = ref.clamp_min(0) if relu else ref
                    if not relu:
                        assert_not_degenerate(ref)
                    cx.begin()
                    y = ops.conv2d_fwd(xh, wk, bh, K, R, R, (st, st), (pad, pad), out_f32=out_f32, relu=relu)
                    cx.note('igemm_kernel')
                    assert_same_values(y, ref, F32 if out_f32 else dt,
                                       'fwd+bias relu=%s f32=%s %s %s' % (relu, out_f32, (N, H, W, C, K, R, st), TAG[dt]))


@case('epilogue-fwd-bn-statistics')
def _epi_stats(cx):
    """y exact and each partial row == the exact sum / sum of squares of its pixels; the halo and streaming kernels
    emit one row per workgroup, there the column sums over all rows are exact.  |y| <= 128 is asserted: then y is
    stored without rounding in every dtype and a 256-pixel row of squares stays below 2^24."""
    ops, L = cx.ops, cx.L
    emul = cx.mode == 'emul'
    cfgs = [(2, 9, 9, 16, 64, 3, 1, 1), (3, 7, 5, 16, 72, 1, 1, 0), (1, 20, 20, 8, 136, 3, 2, 1), (2, 12, 12, 16, 256, 3, 1, 1)] \
        if emul else [(8, 56, 56, 64, 64, 1, 1, 0), (4, 28, 28, 128, 128, 3, 1, 1), (3, 17, 13, 64, 72, 3, 2, 1),
                      (2, 224, 224, 8, 64, 7, 2, 3), (8, 14, 14, 256, 256, 3, 1, 1)]
    for dt in DTYPES:
        for (N, H, W, C, K, R, st, pad) in cfgs:
            g = torch.Generator().manual_seed(K + H)
            dens = min(0.5, 24.0 / (C * R * R)) ** 0.5 if C * R * R > 96 else 0.5
            x, w = _small((N, H, W, C), g, density=max(dens, 0.25)), _small((K, R, R, C), g, lo=-1, hi=1, density=dens)
            y_ref, A = _triple(ref_fwd, x, w, st, pad)
            assert float(y_ref.abs().max()) <= 128
            assert_not_degenerate(y_ref)
            xh, wk = cx.put(x, dt), cx.put(w, dt)
            M = y_ref.numel() // K
            y2 = y_ref.reshape(M, K)
            tiled = {'CONV1X1_STREAM': False, 'CONV3X3_HALO': False}
            variants = [(tiled, {}, 128, None), (tiled, {}, 128, 'pivot')]
            if dt != F32 and K >= 256 and K % 128 == 0:
                variants.append((tiled, {'igemm_256sq': 1}, 256, None))
            for flags, kn, rowpx, piv in variants:
                pivot = int_tensor((K,), g, lo=-4, hi=4, density=0.8) if piv else None
                with cx.knobs(flags=flags, **kn):
                    cx.begin()
                    y = ops.conv2d_fwd(xh, wk, None, K, R, R, (st, st), (pad, pad), bn_stats=True,
                                       pivot=cx.put(pivot, F32) if piv else None)
                    cx.note('igemm_kernel')
                what = 'bn_stats %s %s rows of %d pivot=%s' % ((N, H, W, C, K, R, st), TAG[dt], rowpx, piv)
                assert_same_values(y, y_ref, dt, what)
                ps = ops.take_pending_stats(y)
                assert ps is not None and ps.rows == (M + 127) // 128 and ops.take_pending_stats(y) is None
                part = ps.partial.cpu().double()
                c = y2 - pivot if piv else y2
                want = torch.zeros(ps.rows, 2 * K, dtype=torch.float64)
                for i in range(0, M, rowpx):         # a 256-pixel tile carries its sums in the first of its two rows
                    blk = c[i:i + rowpx]
                    want[i // 128, :K], want[i // 128, K:] = blk.sum(0), (blk * blk).sum(0)
                    assert_exact_domain((blk * blk).sum(0))
                assert_same_values(part.float(), want, F32, what + ' partial rows')
    # one row per workgroup: the halo 3x3 and the streaming 1x1 kernels
    per_wg = [((1, 9, 7, 64, 64, 3, 1, 1), 'conv3x3_c64_kernel'), ((2, 6, 6, 128, 256, 1, 1, 0), 'jfwd_kernel')] if emul else \
        [((4, 56, 56, 64, 64, 3, 1, 1), 'conv3x3_c64_kernel'), ((8, 56, 56, 64, 256, 1, 1, 0), 'jfwd_kernel'),
         ((16, 14, 14, 256, 1024, 1, 1, 0), 'jfwd_kernel')]
    for dt in HALF:
        for (N, H, W, C, K, R, st, pad), name in per_wg:
            g = torch.Generator().manual_seed(K + H)
            dens = (24.0 / (C * R * R)) ** 0.5
            x, w = _small((N, H, W, C), g, density=dens), _small((K, R, R, C), g, lo=-1, hi=1, density=dens)
            y_ref, A = _triple(ref_fwd, x, w, st, pad)
            assert float(y_ref.abs().max()) <= 128
            assert_not_degenerate(y_ref)
            y2 = y_ref.reshape(-1, K)
            assert_exact_domain((y2 * y2).sum(0))        # bounds every workgroup's row as well
            cx.begin()
            y = ops.conv2d_fwd(cx.put(x, dt), cx.put(w, dt), None, K, R, R, (st, st), (pad, pad), bn_stats=True)
            cx.note(name)
            what = 'bn_stats %s %s %s' % ((N, H, W, C, K, R), TAG[dt], name)
            assert_same_values(y, y_ref, dt, what)
            ps = ops.take_pending_stats(y)
            assert ps is not None and ps.rows in (L.cn_conv3x3_c64_rows(N, H), L.cn_conv1x1_stream_fwd_rows(N, H, W, K))
            s = ps.partial.cpu().double().sum(0)
            assert_same_values(s.float(), torch.cat([y2.sum(0), (y2 * y2).sum(0)]), F32, what + ' column sums')


@case('epilogue-wgrad-beta-scale')
def _epi_wgrad(cx):
    ops = cx.ops
    cfgs = [(2, 6, 6, 8, 64, 3, 1, 1), (3, 5, 5, 64, 136, 1, 1, 0), (2, 9, 7, 64, 128, 3, 1, 1)] if cx.mode == 'emul' else \
        [(8, 56, 56, 64, 256, 1, 1, 0), (16, 56, 56, 64, 64, 3, 1, 1), (4, 56, 56, 128, 128, 3, 2, 1), (3, 17, 13, 64, 72, 3, 2, 1)]
    for dt in DTYPES:
        for (N, H, W, C, K, R, st, pad) in cfgs:
            g = torch.Generator().manual_seed(C + K)
            P, Q = ops.conv_out_hw(H, W, R, R, (st, st), (pad, pad))
            x, dy = int_tensor((N, H, W, C), g), int_tensor((N, P, Q, K), g)
            ref, A = _triple(ref_wgrad, x, dy, (K, R, R, C), st, pad)
            assert_not_degenerate(ref)
            xh, dyh = cx.put(x, dt), cx.put(dy, dt)
            init = int_tensor((K, R, R, C), g, lo=-9, hi=9)
            for s1, s2 in ((1.0, 0.5), (2.0, 1.0), (0.5, 2.0)):
                assert_exact_domain(2 * ((s1 + s2) * A + init.abs()))     # in units of 1/2
                what = 'wgrad beta/scale %s %s scales %s' % ((N, H, W, C, K, R, st), TAG[dt], (s1, s2))
                dw = torch.full((K, R, R, C), float('nan'), device=cx.dev)
                cx.begin()
                ops.conv2d_wgrad(xh, dyh, dw, C, K, R, R, (st, st), (pad, pad), beta=0.0, scale=s1)
                cx.note('wgrad')
                assert_same_values(dw, s1 * ref, F32, what + ' beta=0 over NaN')
                ops.conv2d_wgrad(xh, dyh, dw, C, K, R, R, (st, st), (pad, pad), beta=1.0, scale=s2)
                assert_same_values(dw, (s1 + s2) * ref, F32, what + ' two accumulating calls')
                dw = cx.put(init, F32)
                ops.conv2d_wgrad(xh, dyh, dw, C, K, R, R, (st, st), (pad, pad), beta=1.0, scale=s2)
                assert_same_values(dw, init + s2 * ref, F32, what + ' beta=1 onto integers')


def _bits(on, ch, dev):
    """ReLU mask bytes: bit i of byte j = element j*ch + i (ch elements per 16-byte chunk)."""
    M, C = on.shape
    w8 = (2 ** torch.arange(ch)).view(1, 1, ch)
    return (on.view(M, C // ch, ch).long() * w8).sum(-1).to(torch.uint8).contiguous().to(dev)


@case('epilogue-dgrad-addend-bn-backward')
def _epi_dgrad(cx):
    """dx + addend (dense / the even pixels only), and the BatchNorm-backward epilogue: g == where(mask, dx) and the
    `sum g` half of the partial rows exactly; the `sum g*xhat` half under the forward bound.  mean is an integer and
    invstd a power of two, so xhat itself is exact.  The epilogue works on the accumulator as staged in the output type:
    dx + addend carries the two roundings of a data gradient followed by an add, round(round(dx) + addend), and the sums
    are those of the stored g."""
    ops, L, lib = cx.ops, cx.L, cx.lib
    emul = cx.mode == 'emul'
    # (N, H, W, C, K, R, stride, pad, mask bits given, addend: 0 none / 1 dense / 2 subsampled)
    cfgs = [(2, 9, 9, 16, 64, 3, 1, 1, False, 0), (3, 7, 5, 72, 16, 1, 1, 0, True, 1), (1, 12, 12, 16, 24, 3, 2, 1, False, 2),
            (2, 8, 8, 64, 32, 1, 2, 0, True, 0), (2, 9, 7, 16, 24, 1, 1, 0, True, 2), (2, 7, 7, 136, 16, 1, 1, 0, False, 1)] \
        if emul else \
        [(8, 56, 56, 64, 64, 3, 1, 1, False, 0), (16, 56, 56, 256, 64, 1, 1, 0, True, 1), (4, 56, 56, 128, 128, 3, 2, 1, False, 2),
         (4, 56, 56, 256, 512, 1, 2, 0, True, 1), (5, 14, 14, 1024, 256, 1, 1, 0, True, 1), (3, 17, 13, 72, 64, 3, 2, 1, False, 1),
         (8, 56, 56, 256, 128, 1, 1, 0, True, 2), (3, 17, 13, 64, 72, 1, 1, 0, False, 2)]
    for dt in DTYPES:
        ch = lib.chunk_elems(dt)
        for (N, H, W, C, K, R, st, pad, use_bits, add) in cfgs:
            if C % ch:
                continue
            g_ = torch.Generator().manual_seed(C + K + H)
            P, Q = ops.conv_out_hw(H, W, R, R, (st, st), (pad, pad))
            M = N * H * W
            dy, w = int_tensor((N, P, Q, K), g_), int_tensor((K, R, R, C), g_)
            dx, A = _triple(ref_dgrad, dy, w, (N, H, W, C), st, pad)
            addend = dense = None
            if add:
                dense = int_tensor((N, H, W, C), g_, lo=-6, hi=6, density=0.9)
                addend = dense
                if add == 2:
                    addend = dense[:, ::2, ::2].contiguous()
                    dense = torch.zeros_like(dense)
                    dense[:, ::2, ::2] = addend
                dx, A = dx.to(dt).double() + dense, A + dense.abs()
                assert_exact_domain(A)
            dx = dx.to(dt).double()           # as stored
            assert_not_degenerate(dx if add else _support(dx, R, st))
            dyh, wc = cx.put(dy, dt), cx.put(w.permute(3, 1, 2, 0), dt)
            ah = cx.put(addend, dt) if add else None
            what = 'dgrad addend=%d %s %s' % (add, (N, H, W, C, K, R, st), TAG[dt])
            if add:
                with cx.knobs(flags={'JDGRAD': False}):
                    cx.begin()
                    out = ops.conv2d_dgrad(dyh, wc, (N, H, W, C), K, R, R, (st, st), (pad, pad), addend=ah, addend_sub=max(add, 1))
                    cx.note('igemm_kernel')
                assert_same_values(out, dx, dt, what)
            # BatchNorm-backward epilogue
            bn_y = int_tensor((N, H, W, C), g_, lo=-4, hi=4, density=0.9)
            mean = int_tensor((C,), g_, lo=-2, hi=2)
            invstd = _pow2(C, g_)
            scale, shift = _pow2(C, g_), int_tensor((C,), g_, lo=-2, hi=2)
            stats = cx.put(torch.cat([mean, invstd, scale, shift]), F32)
            pre = bn_y * scale + shift
            on = (torch.rand(M, C, generator=g_) > 0.4) if use_bits else (pre > 0).reshape(M, C)
            bits = _bits(on, ch, cx.dev) if use_bits else None
            g_ref = torch.where(on.view(N, H, W, C), dx, torch.zeros_like(dx))
            xhat = ((bn_y - mean) * invstd).reshape(M, C)
            assert_exact_domain(torch.where(on, A.reshape(M, C), torch.zeros(())).sum(0))
            for jd in ((False, True) if (use_bits and add) else (False,)):
                with cx.knobs(flags={'JDGRAD': jd}):
                    cx.begin()
                    gq, partial, rows = ops.conv2d_dgrad(dyh, wc, (N, H, W, C), K, R, R, (st, st), (pad, pad), addend=ah,
                                                         bn=(cx.put(bn_y, dt), bits, stats, True), addend_sub=max(add, 1))
                    names = cx.note()
                    if any('jdgrad' in n for n in names):
                        assert jd and rows == L.cn_conv2d_dgrad_junction_rows_k(N, H, W, C, K)
                    else:
                        assert rows == L.cn_conv2d_dgrad_bnbwd_rows(N, H, W, C, st, st)
                assert tuple(partial.shape) == (rows, 2 * C)
                wh = what + ' bn-backward bits=%s %s' % (use_bits, names)
                assert_same_values(gq, g_ref, dt, wh)
                s = partial.cpu().double().sum(0)
                gs = g_ref.reshape(M, C)
                assert_same_values(s[:C].float(), gs.sum(0), F32, wh + ' sum g')
                bound = 2.0 * M * 2.0 ** -24 * (gs * xhat).abs().sum(0) + 1e-30
                err = (s[C:] - (gs * xhat).sum(0)).abs()
                assert bool((err <= bound).all()), (wh + ' sum g*xhat', float((err / bound).max()))


@case('epilogue-streaming-junction-dgrad')
def _epi_junction(cx):
    """jdgrad_kernel / jdgrad_w32_kernel on every instantiated (C, K), dense and subsampled addend, few and many splits."""
    ops, L = cx.ops, cx.L
    if cx.mode == 'emul':
        cases = [(1, 6, 10, 256, 64, 1, 3), (2, 6, 6, 256, 128, 2, 2), (1, 5, 9, 512, 128, 1, 5), (1, 4, 6, 512, 256, 2, 2),
                 (1, 3, 5, 1024, 256, 1, 3)]
    else:
        cases = [(8, 56, 56, 256, 64, 1, 256), (8, 56, 56, 256, 128, 2, 256), (16, 28, 28, 512, 128, 1, 256),
                 (3, 17, 13, 256, 64, 2, 7), (2, 9, 11, 512, 128, 1, 256), (16, 28, 28, 512, 256, 2, 256),
                 (32, 14, 14, 1024, 256, 1, 256), (64, 28, 28, 512, 128, 1, 256)]
    for dt in HALF:
        for (N, H, W, C, K, sub, splits) in (cases[:2] + cases[4:5] if (cx.mode == 'emul' and dt == F16) else cases):
            g_ = torch.Generator().manual_seed(C + K + H)
            M = N * H * W
            dens = (16.0 / K) ** 0.5
            dy, w = _ints((N, H, W, K), g_, f32=N > 64, density=dens), int_tensor((K, 1, 1, C), g_, density=dens)
            if N > 64:
                w = w.float()
            dx = ref_dgrad(dy, w, (N, H, W, C), 1, 0)
            assert_exact_domain(torch.tensor(9.0 * K + 6))
            dense = _ints((N, H, W, C), g_, f32=N > 64, lo=-6, hi=6, density=0.9)
            addend = dense
            if sub == 2:
                addend = dense[:, ::2, ::2].contiguous()
                dense = torch.zeros_like(dense)
                dense[:, ::2, ::2] = addend
            dx = (dx.to(dt).double() + dense).to(dt).double()      # round(round(dx) + addend), as stored
            assert_not_degenerate(dx)
            bn_y = _ints((N, H, W, C), g_, f32=N > 64, lo=-4, hi=4, density=0.9)
            mean, invstd = int_tensor((C,), g_, lo=-2, hi=2), _pow2(C, g_)
            stats = cx.put(torch.cat([mean, invstd, _pow2(C, g_), int_tensor((C,), g_, lo=-2, hi=2)]), F32)
            on = torch.rand(M, C, generator=g_) > 0.4
            g_ref = torch.where(on.view(N, H, W, C), dx, torch.zeros_like(dx))
            gs = g_ref.reshape(M, C).double()
            assert_exact_domain(gs.abs().sum(0))
            with cx.knobs(flags={'JDGRAD': True}, jdgrad_splits=splits):
                cx.begin()
                gq, partial, rows = ops.conv2d_dgrad(cx.put(dy, dt), cx.put(w.permute(3, 1, 2, 0), dt), (N, H, W, C), K, 1, 1,
                                                     (1, 1), (0, 0), addend=cx.put(addend, dt),
                                                     bn=(cx.put(bn_y, dt), _bits(on, 8, cx.dev), stats, True), addend_sub=sub)
                cx.note('jdgrad_w32_kernel' if K >= 256 else 'jdgrad_kernel')
                assert rows == L.cn_conv2d_dgrad_junction_rows_k(N, H, W, C, K) and rows <= max(splits, 1)
            what = 'junction dgrad %s sub=%d splits=%d %s %s' % ((N, H, W, C, K), sub, splits, TAG[dt], cx.names)
            assert_same_values(gq, g_ref, dt, what)
            s = partial.cpu().double().sum(0)
            assert_same_values(s[:C].float(), gs.sum(0), F32, what + ' sum g')
            xhat = ((bn_y.double() - mean) * invstd).reshape(M, C)
            bound = 2.0 * M * 2.0 ** -24 * (gs * xhat).abs().sum(0) + 1e-30
            err = (s[C:] - (gs * xhat).sum(0)).abs()
            assert bool((err <= bound).all()), (what + ' sum g*xhat', float((err / bound).max()))


@case('lazy-a')
def _lazy_a(cx):
    """a = relu?(y * scale + shift) formed on the operand path and written as a side output; out = conv(a)."""
    ops = cx.ops
    emul = cx.mode == 'emul'
    c1 = [(1, 6, 10, 64, 256), (2, 6, 6, 128, 256), (1, 5, 9, 128, 512), (1, 5, 7, 256, 1024)] if emul else \
        [(8, 56, 56, 64, 256), (8, 56, 56, 128, 256), (16, 28, 28, 128, 512), (3, 17, 13, 64, 256), (64, 14, 14, 256, 1024)]
    c3 = [(1, 6, 7, 64, 64), (2, 5, 4, 64, 64)] if emul else [(8, 56, 56, 64, 64), (3, 17, 13, 64, 64), (2, 9, 56, 64, 64)]
    for dt in HALF:
        for R, cases in ((1, c1[:2] if (emul and dt == F16) else c1), (3, c3)):
            for (N, H, W, C, K) in cases:
                for relu in (True, False):
                    g = torch.Generator().manual_seed(C + K + H + int(relu))
                    y = int_tensor((N, H, W, C), g, lo=-4, hi=4, density=0.9)
                    scale, shift = _pow2(C, g), int_tensor((C,), g, lo=-3, hi=3, density=0.8)   # relu(shift) != 0: a transformed pad would show
                    w = int_tensor((K, R, R, C), g, density=(16.0 / (C * R * R)) ** 0.5)
                    a_ref = y * scale + shift
                    a_ref = a_ref.clamp_min(0) if relu else a_ref
                    out_ref, A = _triple(ref_fwd, a_ref, w, 1, R // 2, unit=0.5)
                    assert_not_degenerate(out_ref)
                    stats = cx.put(torch.cat([torch.zeros(C).double(), torch.ones(C).double(), scale, shift]), F32)
                    a = torch.full((N, H, W, C), float('nan'), dtype=dt, device=cx.dev)
                    cx.begin()
                    out = ops.conv2d_fwd_lazya((cx.put(y, dt), stats, a, relu), cx.put(w, dt), K, bn_stats=True, kernel=(R, R))
                    cx.note('jfwd_kernel' if R == 1 else 'conv3x3_c64_kernel')
                    assert cx.names[-1].endswith(', true>') or ', true>' in cx.names[-1], cx.names
                    what = 'lazy a %dx%d %s relu=%s %s' % (R, R, (N, H, W, C, K), relu, TAG[dt])
                    assert_same_values(a, a_ref, dt, what + ' side output a')
                    assert_same_values(out, out_ref, dt, what)
                    assert ops.take_pending_stats(out) is not None


@case('lazy-z')
def _lazy_z(cx):
    """z = relu(y * s + t + residual) (or + residual * s_d + t_d with the shortcut's BatchNorm folded in) formed on the
    operand load and stored, with its ReLU bits; out = conv1x1(z)."""
    ops, lib = cx.ops, cx.lib
    cases = [(2, 5, 7, 40, 24), (1, 6, 6, 72, 128)] if cx.mode == 'emul' else [(4, 56, 56, 256, 64), (4, 28, 28, 512, 128), (3, 17, 13, 256, 128)]
    for dt in DTYPES:
        ch = lib.chunk_elems(dt)
        for (N, H, W, C, K) in cases:
            for dual in (False, True):
                g = torch.Generator().manual_seed(5 + C + int(dual))
                M = N * H * W
                y, r = int_tensor((N, H, W, C), g, lo=-4, hi=4, density=0.9), int_tensor((N, H, W, C), g, lo=-4, hi=4, density=0.9)
                s3, t3 = _pow2(C, g), int_tensor((C,), g, lo=-3, hi=3)
                sd, td = _pow2(C, g), int_tensor((C,), g, lo=-3, hi=3)
                w = int_tensor((K, 1, 1, C), g, density=(16.0 / C) ** 0.5)
                z_ref = (y * s3 + t3 + (r * sd + td if dual else r)).clamp_min(0)
                out_ref, A = _triple(ref_fwd, z_ref, w, 1, 0, unit=0.5)
                assert_not_degenerate(out_ref)
                zero, one = torch.zeros(C).double(), torch.ones(C).double()
                st3, std = cx.put(torch.cat([zero, one, s3, t3]), F32), cx.put(torch.cat([zero, one, sd, td]), F32)
                z = torch.full((N, H, W, C), float('nan'), dtype=dt, device=cx.dev)
                m = torch.zeros(M * (C // ch), dtype=torch.uint8, device=cx.dev)
                cx.begin()
                out = ops.conv2d_fwd_lazyz((cx.put(y, dt), cx.put(r, dt), st3, std if dual else None, z, m, True), cx.put(w, dt), K,
                                           bn_stats=True)
                cx.note(', 3, false>')
                what = 'lazy z %s dual=%s %s' % ((N, H, W, C, K), dual, TAG[dt])
                assert_same_values(z, z_ref, dt, what + ' side output z')
                m_ok = torch.equal(m.cpu(), _bits((z_ref > 0).reshape(M, C), ch, 'cpu').flatten())
                assert m_ok, what + ' ReLU bits'
                assert_same_values(out, out_ref, dt, what)
                ps = ops.take_pending_stats(out)
                assert ps is not None and ps.rows == (M + 127) // 128


def _lazy_dy_data(cx, N, P, Q, K, g, f32=False):
    """(g, y, coef) of a lazy upstream gradient and dy = c1*g + (c2*y + c3): multiples of 1/2, |dy| <= 16."""
    gz = _ints((N, P, Q, K), g, f32=f32, lo=-3, hi=3, density=0.7)
    y = _ints((N, P, Q, K), g, f32=f32, lo=-3, hi=3, density=0.7)
    c1, c2, c3 = _pow2(K, g), int_tensor((K,), g, lo=-2, hi=2, density=0.6), int_tensor((K,), g, lo=-2, hi=2, density=0.6)
    if f32:
        c1, c2, c3 = c1.float(), c2.float(), c3.float()
    dy = c1 * gz + (c2 * y + c3)
    return gz, y, cx.put(torch.cat([c1, c2, c3]), F32), dy


@case('lazy-dy')
def _lazy_dy(cx):
    """dgrad / wgrad whose upstream gradient dy = c1*g + c2*y + c3 is formed on the operand load: the tiled lazy
    kernels, the streaming lazy dgrad (jdlazy_kernel) and the junction pair (jbwd_kernel)."""
    ops = cx.ops
    emul = cx.mode == 'emul'
    tiled = [(3, 6, 5, 16, 64, 1), (2, 8, 8, 32, 136, 2)] if emul else [(32, 56, 56, 64, 256, 1), (16, 56, 56, 256, 512, 2), (8, 28, 28, 128, 512, 1)]
    for dt in DTYPES:
        for (N, H, W, C, K, st) in tiled:
            g = torch.Generator().manual_seed(K + H)
            P, Q = (H - 1) // st + 1, (W - 1) // st + 1
            x = int_tensor((N, H, W, C), g)
            w = int_tensor((K, 1, 1, C), g, density=(16.0 / K) ** 0.5)
            gz, y, coef, dy = _lazy_dy_data(cx, N, P, Q, K, g)
            dx_ref, _ = _triple(ref_dgrad, dy, w, (N, H, W, C), st, 0, unit=0.5)
            dw_ref, _ = _triple(ref_wgrad, x, dy, (K, 1, 1, C), st, 0, unit=0.5)
            assert_not_degenerate(_support(dx_ref, 1, st))
            assert_not_degenerate(dw_ref)
            what = 'lazy dy %s %s' % ((N, H, W, C, K, st), TAG[dt])
            gh, yh, xh, wc = cx.put(gz, dt), cx.put(y, dt), cx.put(x, dt), cx.put(w.permute(3, 1, 2, 0), dt)
            cx.begin()
            dx = ops.conv2d_dgrad_lazy(gh, yh, coef, wc, (N, H, W, C), K, 1, 1, (st, st), (0, 0))
            cx.note()
            assert_same_values(dx, dx_ref, dt, what + ' dgrad ' + str(cx.names))
            dw = torch.full((K, 1, 1, C), float('nan'), device=cx.dev)
            cx.begin()
            ops.conv2d_wgrad_lazy(xh, gh, yh, coef, dw, C, K, 1, 1, (st, st), (0, 0), beta=0.0)
            cx.note('wgrad_kernel')
            assert_same_values(dw, dw_ref, F32, what + ' wgrad ' + str(cx.names))
    # the streaming lazy dgrad: 512 -> 128 / 256 channels
    K = 512
    for dt in HALF:
        for (N, H, W, C) in ([(1, 5, 9, 128), (1, 6, 7, 256)] if emul else
                             [(16, 28, 28, 128), (3, 17, 13, 128), (256, 28, 28, 128), (3, 17, 13, 256), (64, 28, 28, 256)]):
            g = torch.Generator().manual_seed(N * H + W + C)
            big = N > 64
            w = int_tensor((K, 1, 1, C), g, density=(16.0 / K) ** 0.5)
            gz, y, coef, dy = _lazy_dy_data(cx, N, H, W, K, g, f32=big)
            if big:
                assert_exact_domain(torch.tensor(2.0 * 16 * 3 * K))
                dx_ref = ref_dgrad(dy, w.float(), (N, H, W, C), 1, 0)
            else:
                dx_ref, _ = _triple(ref_dgrad, dy, w, (N, H, W, C), 1, 0, unit=0.5)
            assert_not_degenerate(dx_ref)
            cx.begin()
            dx = ops.conv2d_dgrad_lazy(cx.put(gz, dt), cx.put(y, dt), coef, cx.put(w.permute(3, 1, 2, 0), dt), (N, H, W, C), K, 1, 1,
                                       (1, 1), (0, 0))
            cx.note('jdlazy_kernel')
            assert_same_values(dx, dx_ref, dt, 'streaming lazy dgrad %s %s' % ((N, H, W, C), TAG[dt]))
    # the junction pair: data + weight gradient of the 64 -> 256 1x1 in one pass
    C, K = 64, 256
    for dt in HALF:
        for (N, H, W, splits) in ([(1, 10, 13, 3), (2, 16, 16, 256)] if emul else [(3, 56, 56, 256), (256, 56, 56, 256), (5, 17, 9, 7)]):
            g = torch.Generator().manual_seed(N * H + W)
            big = N > 64
            x = _ints((N, H, W, C), g, f32=big)
            w = int_tensor((K, 1, 1, C), g, density=0.25)
            gz, y, coef, dy = _lazy_dy_data(cx, N, H, W, K, g, f32=big)
            if big:
                # fp32 references.  The magnitude sums in fp32 as well: sums of non-negative terms only grow under
                # rounding, so a true partial sum at or above 2^24 would show in them
                assert_exact_domain(torch.tensor(2.0 * 16 * 3 * K))
                assert_exact_domain(2 * ref_wgrad(x.abs(), dy.abs(), (K, 1, 1, C), 1, 0))
                dx_ref = ref_dgrad(dy, w.float(), (N, H, W, C), 1, 0)
                dw_ref = ref_wgrad(x, dy, (K, 1, 1, C), 1, 0)
            else:
                dx_ref, _ = _triple(ref_dgrad, dy, w, (N, H, W, C), 1, 0, unit=0.5)
                dw_ref, _ = _triple(ref_wgrad, x, dy, (K, 1, 1, C), 1, 0, unit=0.5)
            assert_not_degenerate(dx_ref)
            assert_not_degenerate(dw_ref)
            dw = torch.full((K, 1, 1, C), float('nan'), device=cx.dev)
            with cx.knobs(jbwd_splits=splits):
                cx.begin()
                dx = ops.conv2d_bwd1x1_lazy(cx.put(x, dt), cx.put(gz, dt), cx.put(y, dt), coef, cx.put(w.permute(3, 1, 2, 0), dt),
                                            dw, K, beta=0.0)
                cx.note('jbwd_kernel')
            what = 'junction pair %s splits=%d %s' % ((N, H, W), splits, TAG[dt])
            assert_same_values(dx, dx_ref, dt, what + ' dx')
            assert_same_values(dw, dw_ref, F32, what + ' dw')


@case('stem')
def _stem(cx):
    """The 7x7 / stride-2 stem through the module: pixel-pair form (halo forward kernel, stem weight-gradient kernel) and
    the channel-padded 49-tap form, against F.conv2d; plus an even kernel, a 1-channel and a 4-channel input."""
    ca, ops = cx.ca, cx.ops
    emul = cx.mode == 'emul'
    cases = [(2, 3, 20, 20, 64, 7, 3, True), (1, 3, 14, 32, 64, 7, 3, True), (1, 1, 12, 18, 16, 4, 1, True),
             (2, 4, 9, 14, 72, 3, 1, True)]
    if not emul:
        cases += [(4, 3, 224, 224, 64, 7, 3, True), (256, 3, 224, 224, 64, 7, 3, False)]
    for (N, C, H, W, K, R, pad, bwd) in cases:
        g = torch.Generator().manual_seed(H + K)
        big = N > 64
        x = _ints((N, C, H, W), g, f32=big)
        w0 = int_tensor((K, C, R, R), g, density=0.6)
        conv = ca.nn.Conv2d(C, K, kernel_size=R, stride=2, padding=pad, bias=False)
        conv.needs_dgrad = False
        conv.feeds_batchnorm = True       # as the model wires it: the halo forward kernel emits the statistics partials
        model = torch.nn.Sequential(conv)
        ca.engine.prepare(model, cx.dev, BF16)
        conv.weight.data.copy_(w0.float().to(cx.dev))
        model._cn_arena.bump_version()
        assert conv.pair_eligible(x)
        if big:
            assert_exact_domain(torch.tensor(9.0 * C * R * R))
            y_ref = F.conv2d(x, w0.float(), None, 2, pad).permute(0, 2, 3, 1)
        else:
            y_ref, _ = _triple(lambda a, b: F.conv2d(a, b, None, 2, pad).permute(0, 2, 3, 1), x, w0)
        assert_not_degenerate(y_ref)
        what = 'stem %s' % ((N, C, H, W, K, R),)
        xd = x.float().to(cx.dev)
        model._cn_arena.zero_grad()
        cx.begin()
        y = conv.forward_from_nchw(xd)
        names = cx.note('stem_fwd_kernel' if (R == 7 and C == 3) else None)
        assert_same_values(y, y_ref, BF16, what + ' pair form ' + str(names))
        if not bwd:
            continue
        P, Q = y_ref.shape[1], y_ref.shape[2]
        dy = int_tensor((N, P, Q, K), g)
        dw_ref, _ = _triple(lambda a, b: torch.nn.grad.conv2d_weight(a, (K, C, R, R), _nchw(b), 2, pad), x, dy)
        assert_not_degenerate(dw_ref)
        cx.begin()
        y.backward(cx.put(dy, BF16))
        if cx.dev.type == 'cuda':
            ops.SIDE.join(cx.dev)
        # (the stem weight-gradient kernel takes output rows that are whole 16-pixel fragments)
        names = ''
        if cx.dev.type != 'cuda':    # (on a GPU autograd runs the backward on its own thread; the kernel log is per thread)
            names = cx.note('stem_wgrad_kernel' if (R == 7 and C == 3 and Q % 16 == 0) else 'wgrad_kernel')
        assert_same_values(conv.weight.grad, dw_ref, F32, what + ' pair-form weight gradient ' + str(names))
        # the channel-padded R*R-tap form of the same convolution
        model._cn_arena.zero_grad()
        cx.begin()
        y2 = conv(ca.nn.to_nhwc(xd, BF16, conv.padded_in_channels()))
        cx.note('igemm_kernel')
        assert_same_values(y2, y_ref, BF16, what + ' channel-padded form')
        y2.backward(cx.put(dy, BF16))
        if cx.dev.type == 'cuda':
            ops.SIDE.join(cx.dev)
        assert_same_values(conv.weight.grad, dw_ref, F32, what + ' channel-padded weight gradient')
    # the stem weight-gradient kernel with few and many workgroups, on the pair image directly
    from convnet_amd._lib import ptr, dtype_code, stream_of, check
    L = cx.L
    K, R, S, C, pad, S2 = 64, 7, 7, 3, 3, 4
    code = dtype_code(BF16)
    for (N, H, W, wgs) in ([(2, 26, 32, 3), (1, 42, 64, 2)] if emul else [(3, 70, 96, 5), (16, 224, 224, 512)]):
        g = torch.Generator().manual_seed(H + W)
        x = int_tensor((N, C, H, W), g)
        xp = ops.nchw_to_pairs(x.float().to(cx.dev), (pad, pad))
        Hp, Jp = xp.shape[1], xp.shape[2]
        assert L.cn_stem_wgrad_ok(K, R, S2, Jp, code), Jp
        P, Q = (Hp - R) // 2 + 1, Jp - S2 + 1
        dy = int_tensor((N, P, Q, K), g)
        dw_ref, _ = _triple(lambda a, b: torch.nn.grad.conv2d_weight(a, (K, C, R, S), _nchw(b), 2, pad), x, dy)
        dyh = cx.put(dy, BF16)
        t1 = torch.full((K * R * S2 * 8,), float('nan'), dtype=torch.float32, device=cx.dev)
        with cx.knobs(stem_wgrad_wgs=wgs):
            ws = ops.workspace(L.cn_stem_wgrad_workspace(N, Hp), cx.dev, 'main')
            cx.begin()
            check(L.cn_stem_wgrad(ptr(xp), ptr(dyh), ptr(t1), N, Hp, Jp, code, 0.0, 1.0, ptr(ws), ws.numel() * 4,
                                  stream_of(xp)), 'cn_stem_wgrad')
            cx.note('stem_wgrad_kernel')
        dw = torch.zeros(K, R, S, C, device=cx.dev)
        check(L.cn_wgrad_unpack_pairs(ptr(t1), ptr(dw), K, R, S, C, 0.0, stream_of(t1)), 'cn_wgrad_unpack_pairs')
        assert_same_values(dw.permute(0, 3, 1, 2), dw_ref, F32, 'stem_wgrad_kernel %s wgs=%d' % ((N, H, W), wgs))


def gconv_exact(cx, cfg, dt, big=False):
    ops = cx.ops
    N, H, W, C, K, gr, st = cfg
    P, Q = (H - 1) // st + 1, (W - 1) // st + 1
    g = torch.Generator().manual_seed(H + C + K + gr)
    x, dy = _ints((N, H, W, C), g, f32=big), _ints((N, P, Q, K), g, f32=big)
    w = int_tensor((K, 3, 3, C // gr), g)
    w = w.float() if big else w
    what = 'gconv %s %s' % (cfg, TAG[dt])
    xh, wh, dyh = cx.put(x, dt), cx.put(w, dt), cx.put(dy, dt)

    def reference(fn, a, b, n, *args):
        if big:
            assert_exact_domain(torch.tensor(9.0 * n))
            return fn(a, b, *args)
        return _triple(fn, a, b, *args, what=what)[0]

    dense = 9 * (C // gr) >= 8        # a depthwise / two-wide group sums too few terms to be half non-zero at 50 % density
    ref = reference(ref_fwd, x, w, 9 * (C // gr), st, 1, gr)
    if dense:
        assert_not_degenerate(ref)
    cx.begin()
    y = ops.gconv2d_fwd(xh, wh, K, gr, st)
    cx.note('gconv_kernel')
    assert_same_values(y, ref, dt, what + ' fwd')
    ref = reference(ref_dgrad, dy, w, 9 * (K // gr), (N, H, W, C), st, 1, gr)
    cx.begin()
    dx = ops.gconv2d_dgrad(dyh, wh, (N, H, W, C), K, gr, st)
    cx.note('[dgrad]')
    assert_same_values(dx, ref, dt, what + ' dgrad')
    ref = reference(ref_wgrad, x, dy, N * P * Q, (K, 3, 3, C // gr), st, 1, gr)
    if N * P * Q >= 16:
        assert_not_degenerate(ref)
    dw = torch.full((K * 9 * (C // gr),), float('nan'), device=cx.dev)
    cx.begin()
    ops.gconv2d_wgrad(xh, dyh, dw, K, gr, st, beta=0.0)
    cx.note('gconv_dw_kernel')
    assert_same_values(dw.view(K, 3, 3, C // gr), ref, F32, what + ' wgrad')
    ops.gconv2d_wgrad(xh, dyh, dw, K, gr, st, beta=1.0, scale=0.5)
    assert_same_values(dw.view(K, 3, 3, C // gr), 1.5 * ref, F32, what + ' wgrad beta=1 scale=0.5')


def _reg_gconv():
    for dt in DTYPES:
        def run(cx, dt=dt):
            for cfg in GCONV_EMUL:
                gconv_exact(cx, cfg, dt)
            gconv_exact(cx, (1, 3, 5, 272, 272, 8, 1), dt)       # 34 rows per group
            gconv_exact(cx, (1, 4, 3, 272, 272, 8, 2), dt)
            if cx.mode == 'gpu':
                for cfg in _shapes_resnext(2):
                    gconv_exact(cx, cfg, dt)
        case('gconv-%s' % TAG[dt])(run)

    def wide(cx):      # 64 rows per group, unequal widths
        gconv_exact(cx, (1, 3, 4, 128, 128, 2, 1), BF16)
        gconv_exact(cx, (1, 3, 3, 128, 64, 2, 2), BF16)
        gconv_exact(cx, (1, 3, 3, 64, 128, 2, 1), F32)
    case('gconv-wide-groups')(wide)

    for dt in DTYPES:
        def run(cx, dt=dt):
            for H, C, st in ((56, 128, 1), (56, 256, 2), (28, 256, 1)):
                gconv_exact(cx, (256, H, H, C, C, 32, st), dt, big=True)
        case('gconv-b256-%s' % TAG[dt], ('gpu',))(run)


_reg_gconv()


@case('classifier')
def _classifier(cx):
    """nn.Linear with an integer bias and fp32 logits, and its data gradient: the small-batch dense kernel and the
    tiled kernel, each against the reference."""
    ops = cx.ops
    shapes = [(5, 64, 1000), (37, 96, 1000)] if cx.mode == 'emul' else [(256, 2048, 1000), (8, 2048, 1000), (37, 96, 1000)]
    for dt in DTYPES:
        for (B, C, K) in shapes:
            g = torch.Generator().manual_seed(B + C)
            x, w = int_tensor((B, C), g), int_tensor((K, C), g, density=min(0.5, (32.0 / C) ** 0.5))
            b = int_tensor((K,), g, lo=-5, hi=5, density=0.8)
            dy = int_tensor((B, K), g, density=0.2)
            y_ref, A = _triple(lambda a, c: a @ c.t(), x, w)
            y_ref = y_ref + b
            assert_exact_domain(A + 5)
            dx_ref, _ = _triple(lambda a, c: a @ c, dy, w)
            assert_not_degenerate(y_ref)
            assert_not_degenerate(dx_ref)
            xh, wh, bh = cx.put(x.view(B, 1, 1, C), dt), cx.put(w, dt), cx.put(b, F32)
            dyh, wt = cx.put(dy.view(B, 1, 1, K), dt), cx.put(w.t(), dt)
            for small in ((1, 0) if dt != F32 else (1,)):
                with cx.knobs(dense_smallm=small):
                    cx.begin()
                    y = ops.conv2d_fwd(xh, wh, bh, K, 1, 1, (1, 1), (0, 0), out_f32=True)
                    names = cx.note('dense_smallm_kernel' if (small and dt != F32) else 'igemm_kernel')
                    what = 'classifier %s %s %s' % ((B, C, K), TAG[dt], names)
                    assert_same_values(y.view(B, K), y_ref, F32, what)
                    cx.begin()
                    dx = ops.conv2d_dgrad(dyh, wt, (B, 1, 1, C), K, 1, 1, (1, 1), (0, 0))
                    names = cx.note('dense_smallm_kernel' if (small and dt != F32) else 'igemm_kernel')
                    assert_same_values(dx.view(B, C), dx_ref, dt, what + ' dgrad %s' % names)


# =====================================================================================================================
def _params():
    out = []
    for name, modes, _ in CASES:
        for m in modes:
            out.append(pytest.param(m, name, id='%s-%s' % (m, name), marks=[pytest.mark.gpu] if m == 'gpu' else []))
    return out


def _run_case(mode, name):
    fn = [f for n, _, f in CASES if n == name][0]
    cx = Ctx(mode)
    fn(cx)
    DONE[mode].add(name)


@pytest.mark.parametrize('mode,name', _params())
def test_exact(mode, name):
    _run_case(mode, name)


# kernel families (regular expressions on cn_last_kernel_name) the exact sweep must reach.  gpu: every family that
# cn_set_last_kernel can report outside qconv_i8.hip (that one has its own exact file, test_qconv_exact.py); emul: the ones reachable at emulator cost (all but the shapes that
# exist only at the training batch - none today: every family has a small instantiation)
FAMILIES_EMUL = {
    'igemm 64-channel tile, register-staged': r'igemm_kernel<\w+, 1, 4, 2, 1, 1, false, false, false, false, false, false>',
    'igemm 64-channel tile, LDS-DMA': r'igemm_kernel<\w+, 1, 4, 2, 1, 2, false, true, false, false, false, false>',
    'igemm 128x128 tile, register-staged': r'igemm_kernel<\w+, 2, 2, 2, 2, 1, false, false, false, false, false, false>',
    # (16-bit storage without epilogue operands takes the interleaved form below: this one serves fp32 storage)
    'igemm 128x128 tile, LDS-DMA': r'igemm_kernel<\w+, 2, 2, 2, 2, 2, (true|false), true, false, (true|false), false, false>',
    'igemm 128x128 tile, eight waves': r'igemm_kernel<\w+, 2, 4, 2, 1, 1, false, false, false, false, false, false>',
    'igemm 128x128 tile, LDS-DMA interleaved': r'igemm_kernel<\w+, 2, 2, 2, 2, 2, false, true, true, false, false, true>',
    'igemm 256x256 tile': r'igemm_kernel<\w+, 4, 2, 2, 4, 2, false, true, false, false, false, true>',
    'igemm epilogue operands (addend / BatchNorm backward)': r'igemm_kernel<\w+, (1, 4, 2, 1|2, 2, 2, 2), 1, false, false, false, true, false, false>',
    'igemm epilogue operands, eight waves': r'igemm_kernel<\w+, 2, 4, 2, 1, 1, false, false, false, true, false, false>',
    'igemm fp32 output from 16-bit operands': r'igemm_kernel<(bf16_t|f16_t), (1, 4, 2, 1|2, 2, 2, 2), [12], true,',
    'igemm lazy z': r'igemm_kernel<.*, false, false, false, 3, false>',
    'igemm lazy dy': r'igemm_kernel<.*, false, false, false, true, false>',
    'conv3x3_c64_kernel forward': r'conv3x3_c64_kernel<\w+>$',
    'conv3x3_c64_kernel dgrad': r'conv3x3_c64_kernel<\w+> \[dgrad\]',
    'conv3x3_c64_kernel lazy a': r'conv3x3_c64_kernel<\w+, true>',
    'jfwd_kernel': r'jfwd_kernel<\w+, \d+, \d+>',
    'jfwd_kernel lazy a': r'jfwd_kernel<\w+, \d+, \d+, true>',
    'jdgrad_kernel': r'jdgrad_kernel<',
    'jdgrad_w32_kernel': r'jdgrad_w32_kernel<',
    'jdlazy_kernel': r'jdlazy_kernel<',
    'jbwd_kernel': r'jbwd_kernel<',
    'wgrad_kernel': r'wgrad_kernel<',
    'wgrad_dma_kernel': r'wgrad_dma_kernel<128>',
    'wgrad3x3_kernel 64': r'wgrad3x3_kernel<\w+, 64>',
    'wgrad3x3_kernel 128': r'wgrad3x3_kernel<\w+, 128>',
    'stem_fwd_kernel': r'stem_fwd_kernel<',
    'stem_wgrad_kernel': r'stem_wgrad_kernel<',
    'gconv_kernel': r'gconv_kernel<\w+, (true|false)>$',
    'gconv_kernel dgrad': r'gconv_kernel<\w+, (true|false)> \[dgrad\]',
    'gconv_dw_kernel': r'gconv_dw_kernel<',
    'dense_smallm_kernel': r'dense_smallm_kernel<',
}
FAMILIES_GPU = dict(FAMILIES_EMUL)


@pytest.mark.parametrize('mode', ['emul', pytest.param('gpu', marks=pytest.mark.gpu)])
def test_exact_sweep_reaches_every_kernel_family(mode):
    """Every kernel family the library can report was launched by an exact case of this file (cases that did not run
    in this process - a selection with -k - are run here first).  A family nobody reached is a failure."""
    _dev(mode)
    for name, modes, _ in CASES:
        if mode in modes and name not in DONE[mode]:
            _run_case(mode, name)
    fam = FAMILIES_EMUL if mode == 'emul' else FAMILIES_GPU
    missing = [k for k, rx in fam.items() if not any(re.search(rx, n) for n in SEEN[mode])]
    assert not missing, 'kernel families no exact case reached: %s\nseen: %s' % (missing, sorted(SEEN[mode]))
    assert not any('qconv' in n for n in SEEN[mode])
