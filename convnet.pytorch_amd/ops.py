"""Functional wrappers + autograd Functions over the HIP kernels (C ABI in include/convnet_hip.h).

Tensor conventions of this layer (not of the user-facing modules, which keep the reference's
NCHW / OIHW shapes at their boundary): activations are contiguous NHWC tensors in the compute dtype
(bf16 or fp32), filters are KRSC, parameters / gradients / statistics are fp32.

PyTorch is used here for allocation, stream handles and the autograd tape only; every arithmetic
pass over tensor data is one of the `cn_*` kernels.
"""
import collections
import contextlib
import os
import typing
import weakref

import torch
import torch.distributed as dist
from torch.autograd import Function

from . import _lib, flags
from ._lib import dtype_code, ptr, stream_of

# ---------------------------------------------------------------------------------------------
# workspaces: one grow-only scratch buffer per (device, tag, stream).  Kernels on one stream are ordered,
# so reuse across ops on that stream is safe; keying by stream keeps a buffer from being shared (or, when
# it is replaced by a bigger one, recycled by the caching allocator) across streams without an event.
_WS = {}


def workspace(nbytes, device, tag='main'):
    dev = torch.device(device)
    sid = torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0
    key = (str(dev), tag, sid)
    buf = _WS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        n = max(int(nbytes + 3) // 4, 1024)
        old = buf
        buf = torch.empty(n, dtype=torch.float32, device=dev)
        if old is not None and dev.type == 'cuda':
            old.record_stream(torch.cuda.current_stream(dev))   # kernels still reading the old block finish first
        _WS[key] = buf
    return buf


def _L():
    return _lib.load()


class KernelProfiler(object):
    """Optional per-call HIP-event timing of the kernel wrappers (used by bench.py for the live
    roofline numbers).  Events are recorded on torch's current stream, which is the stream every
    kernel of this package is launched on.  Disabled by default: zero overhead in the hot loop."""

    def __init__(self):
        self.enabled = False
        self.records = []
        # True: the weight-gradient side stream is folded into the main stream while recording, so every kernel
        # runs ALONE (per-kernel / per-layer tables).  False: the step keeps its two-stream schedule and the events
        # sit on whichever stream the call is launched on: durations of the OVERLAPPED step, i.e. what rocprofv3
        # reports for the timed region (used to choose and price the dominant kernel).
        self.fold_streams = True

    def run(self, name, launches, flops, nbytes, fn, device, detail=None):
        """name: label, or a callable evaluated AFTER fn() (the library reports which kernel instantiation(s) its
        dispatcher picked: cn_kernel_log); detail: optional per-shape label (conv layers).  A call that launched
        several DIFFERENT GEMM instantiations (a strided dgrad: one launch per parity class) is recorded under the
        joined label 'a + b' with its true launch count - never under the last launch's name."""
        if not self.enabled or device.type != 'cuda':
            return fn()
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        if callable(name):
            _L().cn_kernel_log(1)
        s.record()
        out = fn()
        e.record()
        if callable(name):
            name = name()
        # (which stream the call was launched on: the weight-gradient side stream's launches are told apart)
        self.records.append((name, launches, flops, nbytes, s, e, detail, torch.cuda.current_stream(device).cuda_stream))
        return out

    def summary(self, by_detail=False):
        torch.cuda.synchronize()
        agg = {}
        # the stream the step runs along = the one most calls were launched on (the trainer's own high-priority stream);
        # everything else is the weight-gradient side stream
        cnt = {}
        for r in self.records:
            cnt[r[7]] = cnt.get(r[7], 0) + 1
        main = max(cnt, key=cnt.get) if cnt else None
        for name, launches, flops, nbytes, s, e, detail, stream in self.records:
            if by_detail and detail is None:
                continue
            a = agg.setdefault(detail if by_detail else name,
                               {'calls': 0, 'launches': 0, 'ms': 0.0, 'flops': 0.0, 'bytes': 0.0, 'records': [], 'side_ms': 0.0})
            ms = s.elapsed_time(e)
            if main is not None and stream != main:
                a['side_ms'] += ms
            a['calls'] += 1
            a['launches'] += launches
            a['ms'] += ms
            a['flops'] += flops
            a['bytes'] += nbytes
            a['records'].append((ms, flops, nbytes))
        return agg


PROFILER = KernelProfiler()
# The switches below mirror flags.py (ONE table: defaults, meaning, how to override for an A/B); tests flip these module
# attributes to compare a fused path with the one it replaces.
# 0: the stride-2 projection shortcut's input gradient as a dense tensor
SUBSAMPLED_SHORTCUT_GRAD = flags.on('subsampled_shortcut_grad')
# 0: the fused stem's BatchNorm-backward sums over the input map with the pool gather
STEM_XMAX = flags.on('stem_xmax')
# 0: plain sum / sum-of-squares statistics partials; 1: centred on the running mean for fp32 models; all: every dtype
CENTERED_STATS = 'all' if flags.text('centered_stats') == 'all' else flags.on('centered_stats')


class SideStream(object):
    """Optional second HIP stream for the weight-gradient kernels: wgrad(x, dy) and dgrad(dy, w) of a
    layer are independent, and the late layers' launches are too small to fill 256 CUs on their
    own, so running wgrad beside the main backward stream packs the machine better.
    Measured +5.2 % on ResNet-50 b=256 (10.04k -> 10.56k img/s).  On by default (flag wgrad_stream).  Trainer /
    BucketReducer join the stream before the gradient all-reduce and the optimizer step; while the KernelProfiler is
    recording in "alone" mode everything stays on one stream.  ONE side stream at the runtime's default priority, all
    CUs: two or three streams, a high-priority side stream and CU masks were measured slower or neutral
    (profiles/r03_ab_whole_step_knobs.txt, profiles/r04_ab_wgrad_reduce_lanes_and_side_streams_rejected.txt)."""

    def __init__(self):
        self.enabled = flags.on('wgrad_stream')
        self._streams = {}
        self.used = False
        self.marks = flags.on('marks')     # 0: always hand off with an event record
        self.capturing = False      # set by Trainer around HIP-graph capture
        self.hold = flags.on('side_hold')
        self._held = collections.deque()
        # a caller that runs backward passes without ever joining (anything but Trainer / BucketReducer) must not pin
        # every operand for ever: beyond this many pending hand-offs the oldest go back to the allocator the
        # record_stream way (correct without a join, just slower).  ResNet-200 with 8 accumulation chunks stays below.
        self.hold_max = 2048
        # ... nor more than this many bytes of them (a count alone lets thousands of activation-sized operands pile up:
        # one ResNet-50 b=256 step holds ~20 GB)
        self.hold_max_bytes = 64 * 2 ** 30
        self._held_bytes = 0
        self._mark = None

    def get(self, device):
        """The side stream the weight-gradient launches go to."""
        st = self._streams.get(device)
        if st is None:
            st = self._streams[device] = torch.cuda.Stream(device)
        return st

    @contextlib.contextmanager
    def mark(self, dy):
        """Around the library call that produces the gradient tensor `dy`: its last kernel signals a mark event on
        completion (cn_stream_arm), so the weight-gradient launch that consumes `dy` can wait for exactly that
        kernel (hipExtLaunchKernel's stop event) instead of an event recorded behind it in the chain's queue."""
        self._mark = None
        if not (self.marks and self.active(dy)):
            yield
            return
        h = _L().cn_stream_arm()
        try:
            yield
        finally:
            if _L().cn_stream_disarm() == 1 and h >= 0:
                self._mark = (dy.data_ptr(), h, dy)   # dy held: its memory cannot be recycled under the mark

    def submit(self, device, launch, notify, dy=None):
        """Run `launch()` (returns the tensors it reads / scratch it uses) on the side stream once `dy` - and
        everything else queued on the current stream so far - is ready, then `notify()`."""
        cur = torch.cuda.current_stream(device)
        side = self.get(device)
        mark, self._mark = self._mark, None
        if mark is not None and dy is not None and dy.data_ptr() == mark[0]:
            _L().cn_stream_wait_mark(mark[1], side.cuda_stream)   # dy's producer is done
        else:
            self.fork(cur, side)
        with torch.cuda.stream(side):
            held = launch()
        if self.hold:
            # the operands stay referenced until the chain has waited for the side stream (join, once per step): the
            # caching allocator then needs no cross-stream bookkeeping for them.  record_stream would make it record an
            # event (with torch's default flags: a system-scope fence) on the side stream at every free and poll it
            nbytes = sum(t.numel() * _esize(t) for t in held)
            self._held.append((held, nbytes))
            self._held_bytes += nbytes
            while len(self._held) > self.hold_max or (self._held_bytes > self.hold_max_bytes and len(self._held) > 1):
                old, ob = self._held.popleft()
                self._held_bytes -= ob
                for t in old:
                    t.record_stream(side)
        else:
            for t in held:
                t.record_stream(side)
        self.used = True
        notify()

    def gather(self, device):
        """The stream a collective (or a join) has to order itself behind."""
        return self.get(device)

    def active(self, t):
        # not while a HIP graph is being captured: a replayed graph runs faster as one chain (b=8 +4 %, b=32 +3 %,
        # b=64 +2 %, b=128 +1 %; the runtime's graph queues put the chain behind a weight gradient every few layers)
        return self.enabled and t.is_cuda and not (PROFILER.enabled and PROFILER.fold_streams) and not self.capturing

    def fork(self, cur, side):
        """`side` waits for everything queued on `cur` so far (one device-scope event from the library's ring)."""
        _L().cn_stream_fork(cur.cuda_stream, side.cuda_stream)

    def join(self, device):
        """Make the current stream wait for everything queued on the side stream(s).  MANDATORY once per step for whoever
        drives backward passes of this package by hand (Trainer._body and BucketReducer.finish do it): the optimizer
        step must not read weight gradients the side stream is still writing, and the operands held for it are released
        here."""
        if self.used and device.type == 'cuda':
            # the library's device-scope ring event, as for the hand-offs in the other direction (torch's wait_stream
            # records an event with the default flags: a system-scope fence on the side stream)
            self.fork(self.gather(device), torch.cuda.current_stream(device))
            self.used = False
        self._held.clear()     # (what the current stream does from here on is ordered behind the side stream's reads)
        self._held_bytes = 0

    def reset(self):
        """Forget the step in flight without waiting for it (an aborted capture: nothing was queued)."""
        self._held.clear()
        self._held_bytes, self.used, self._mark = 0, False, None


SIDE = SideStream()


def reset_step_state(model):
    """An aborted step body (a capture that failed half way) leaves the per-step mailboxes half filled: empty them, the
    next (eager) step starts clean.  Every mailbox of a step is cleared by the module that owns it."""
    for m in model.modules():
        h = getattr(m, '_res_holder', None)
        if h is not None:
            h.reset()
        for slot in _SLOTS + ('_fwd_ctx',):    # (_fwd_ctx: the BatchNorm's weak reference to its forward state)
            m.__dict__.pop(slot, None)
        if hasattr(m, '_pending_bwd'):
            m._pending_bwd = 0
    SIDE.reset()
    from . import quant
    quant.reset_step_state()


def _esize(t):
    return t.element_size()


def _last_kernel(suffix=''):
    """Label of the GEMM-class kernel(s) the library's dispatcher launched in the call just made (cn_kernel_log):
    one name, or the distinct names joined with ' + ' when the call's launches used different instantiations."""
    def label():
        names = [n for n in _L().cn_kernel_log(0).decode().split(';') if n]
        if not names:
            names = [_L().cn_last_kernel_name().decode()]
        uniq = []
        for n in names:
            if n not in uniq:
                uniq.append(n)
        return ' + '.join(uniq) + suffix
    return label


def _conv_detail(kind, C, H, K, R, stride):
    return '%s %d,%d->%d %dx%d/%d' % (kind, C, H, K, R, R, stride[0])


def conv_out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad[0] - R) // stride[0] + 1, (W + 2 * pad[1] - S) // stride[1] + 1


# ---------------------------------------------------------------------------------------------
# raw (non-autograd) kernel calls

# 0 = every BatchNorm re-reads its input for the statistics (bn_stats_kernel)
FUSE_BN_STATS = flags.on('fuse_bn_stats')
# 0 = the stem runs as a 49-tap conv on a 3->8 channel padded image instead of the pixel-pair form
STEM_PAIRS = flags.on('stem_pairs')
# 0 = the pixel-pair stem runs through the tiled implicit-GEMM kernel instead of the halo kernel (csrc/stem.hip)
STEM_HALO = flags.on('stem_halo')
# 0 = the 64 -> 64 channel 3x3 convolutions run through the tiled implicit-GEMM kernel instead of the halo kernel
# (csrc/conv3x3.hip)
CONV3X3_HALO = flags.on('conv3x3_halo')
# 0 = conv3 / the stride-1 projection forward through the tiled kernel instead of the streaming kernel
CONV1X1_STREAM = flags.on('conv1x1_stream')
# 0 = the stem's bn1 -> relu -> maxpool runs as separate BatchNorm and max-pool passes
FUSE_STEM_POOL = flags.on('fuse_stem_pool')
# 0 = BatchNorm backward always runs its own reduction pass over (dz, y).  The fusion is used at the residual JUNCTIONS
# only (the block-input dgrad's epilogue adds the other branch's gradient anyway and no dres tensor is written); at the
# BatchNorms inside a block the epilogue's extra operand stream costs the producing kernel more than the separate pass
# costs (profiles/r01_epilogue_fusions_per_layer.txt; whole step: junctions only 21.34 ms vs everywhere 21.71 ms).
FUSE_BN_BWD = flags.on('fuse_bn_bwd')
# "Lazy dy" (round 3): at a residual junction whose BatchNorm follows a 1x1 convolution (bn3(conv3(.)), the projection
# shortcut's BatchNorm) the backward apply pass  dy = c1*g + c2*y + c3  is not run: the convolution's dgrad and wgrad
# form dy on their operand loads (cn_conv2d_dgrad_lazy / cn_conv2d_wgrad_lazy) - one write and one read of the
# largest tensors of the step less on the critical chain.  For BN inputs that every pass streams from HBM
# (flags.LAZY_MIN_BYTES: 0.6 of the Infinity Cache; the smaller maps keep the LDS-DMA weight-gradient kernels).
LAZY_DY = flags.on('lazy_dy')
LAZY_DY_MIN_MB = float(flags.get('lazy_min_mb'))
# Junction behind a projection shortcut (round 3): the shortcut BatchNorm only finalises its statistics; its apply runs
# inside the junction BatchNorm's apply pass (cn_bn_apply_dual), so the normalised shortcut tensor is neither written nor
# re-read.  Bit-identical.
DUAL_BN = flags.on('dual_bn')
# "Lazy z" (round 3): a residual junction whose output feeds a 1x1 / stride-1 convolution of at most 128 output channels
# (the next bottleneck's conv1) is finalised but not applied; that convolution forms z = relu(bn(y) + residual) on its
# operand load and stores it (cn_conv2d_fwd_lazyz): the junction's apply pass (read y, read residual, write z) and the
# convolution's re-read of z become one read of y and the residual and one write of z.  Bit-identical.  Only inside a
# model forward that guarantees the convolution runs next (LAZY_Z_SCOPE, set by ResNetImagenet.features) and for
# junction tensors of at least LAZY_Z_MIN_MB (same size rule as lazy dy).
LAZY_Z = flags.on('lazy_z')
LAZY_Z_MIN_MB = float(flags.get('lazy_min_mb'))
LAZY_Z_SCOPE = [0]
# Junction pair (round 3): where lazy dy applies and the convolution has an instantiated shape (64 -> 256 channels: conv3
# and the projection of ResNet-50's first stage), its data gradient and weight gradient run as ONE kernel on the backward
# chain (cn_conv2d_bwd1x1_lazy): g and y are read once instead of twice.  dx bit-identical, dW differs by fp32
# summation order.
JPAIR = flags.on('jpair')
# ... and where the lazy dy's y is this convolution's own output (y = conv1x1(x, w), no bias: every site of the model), the
# kernel does not read y but recomputes it per tile from x and w with the forward kernel's instructions
# (cn_conv2d_bwd1x1_lazy_ry): one junction-sized read less, dx and dW bit-identical.  The call site says so by running
# conv2d_bwd1x1_lazy inside `bn_y_is_output_of(w_krsc)`; callers with an arbitrary bn_y keep the kernel that reads it.
JPAIR_RECOMPUTE = flags.on('jpair_recompute')
_BN_Y_PRODUCER = [None]


@contextlib.contextmanager
def bn_y_is_output_of(w_krsc):
    """Inside: the bn_y handed to conv2d_bwd1x1_lazy is conv1x1(x, w) of ITS x, with w_krsc the filter's [K][C] copy."""
    prev, _BN_Y_PRODUCER[0] = _BN_Y_PRODUCER[0], w_krsc
    try:
        yield
    finally:
        _BN_Y_PRODUCER[0] = prev


# Streaming junction kernel (round 3): the fused junction data gradient (conv1's dgrad + shortcut gradient + ReLU mask +
# BatchNorm-backward sums) of the instantiated large shapes runs as one persistent streaming kernel
# (cn_conv2d_dgrad_junction, csrc/junction.hip) instead of the tiled GEMM kernel's epilogue.  g bit-identical, the
# partial sums in another fp32 association.
JDGRAD = flags.on('jdgrad')
# 1 = a convolution's backward launches its data gradient (main stream) before it hands the weight gradient to the side stream
DGRAD_FIRST = flags.on('dgrad_first')


# how often each BatchNorm path ran (tests assert that the fused paths really are the ones in use)
COUNTERS = {'bn_fwd_fused': 0, 'bn_fwd_plain': 0, 'bn_bwd_fused': 0, 'bn_bwd_plain': 0, 'bn_bwd_lazy': 0}


class _PendingStats(object):
    """BatchNorm statistics partials a convolution emitted for its output tensor.  They travel ON that tensor
    object (attribute `_cn_stats`, set by the producing convolution): the BatchNorm that consumes the very same
    object takes them, a copy / view / re-materialised tensor has none and falls back to the statistics pass, and
    the partial buffer dies with the tensor.  No module-level table, nothing keyed by id()."""
    __slots__ = ('partial', 'rows', 'pivot')   # pivot: data_ptr of the running mean the sums are centred on (or None)


def _stats_partial(want, K, device, rows_fn, *dims):
    """(partial, rows) for a convolution that emits the statistics partials of its K output channels - rows_fn(*dims) is
    the kernel's own row count - or (None, 0) when nobody wants them."""
    if not want:
        return None, 0
    rows = rows_fn(*dims)
    return torch.empty((rows, 2 * K), dtype=torch.float32, device=device), rows


def _park_stats(y, partial, rows, pivot=None):
    if partial is None:
        return
    ps = _PendingStats()
    ps.partial, ps.rows = partial, rows
    ps.pivot = pivot.data_ptr() if pivot is not None else None
    y._cn_stats = ps


def take_pending_stats(y):
    """The partials emitted for exactly this tensor object (taken: a second call returns None), else None."""
    ps = getattr(y, '_cn_stats', None)
    if ps is not None:
        del y._cn_stats
    return ps


def _wants_stats(mod):
    """This convolution's epilogue emits the statistics partials of the BatchNorm behind it (model wiring: feeds_batchnorm)."""
    return FUSE_BN_STATS and mod.training and getattr(mod, 'feeds_batchnorm', False)


# ---- per-step hand-offs between layers: a layer parks a half-finished result on the neighbouring module whose kernel
# finishes it.  One record per hand-off (plain tuples in positional order: the raw kernel wrappers take any sequence of
# that length) and ONE mailbox, _park / _take: the record sits in the module's instance dict under the slot's name beside
# its owner tensor's (address, shape, dtype).  A new per-step hand-off is a record plus a name in _SLOTS.
_T, _OptT = torch.Tensor, typing.Optional[torch.Tensor]
# _lazy_z, on the consumer conv: the junction z = relu?(bn(y) + residual) it forms on its operand load and stores
# (res_stats set: behind a projection shortcut, whose BatchNorm is applied to `residual` here too)
LazyZ = typing.NamedTuple('LazyZ', [('y', _T), ('residual', _T), ('stats', _T), ('res_stats', _OptT), ('z', _T),
                                    ('mask', _OptT), ('relu', bool)])
# _lazy_a, on the consumer conv: the inner BatchNorm output a = relu?(bn(bn_y)) it forms on its operand path and stores
LazyA = typing.NamedTuple('LazyA', [('bn_y', _T), ('stats', _T), ('a', _T), ('relu', bool)])
# _lazy_dy, on the producer conv: its upstream gradient dy = c1*g + c2*bn_y + c3, left unformed by the BatchNorm behind it
LazyDy = typing.NamedTuple('LazyDy', [('g', _T), ('bn_y', _T), ('coef', _T)])
# _bwd_partials, on the BatchNorm: its backward reduction partials out of the consumer conv's dgrad epilogue
BwdPartials = typing.NamedTuple('BwdPartials', [('partial', _T), ('rows', int)])
# _deferred, on the projection shortcut's BatchNorm: finalised statistics that the junction's apply pass applies
DeferredBN = typing.NamedTuple('DeferredBN', [('stats', _T)])
# _q_stash, on a quantised block's conv1: the block input's row min / max and quantised copy, for the projection (quant.py)
QStash = typing.NamedTuple('QStash', [('bits', int), ('mm', _T), ('qx', _T)])
# conv2d_dgrad's bn= argument: the forward state of the BatchNorm whose backward reduction the epilogue does
BnBwdOperands = typing.NamedTuple('BnBwdOperands', [('y', _T), ('mask', _OptT), ('stats', _T), ('relu', bool)])
_SLOTS = ('_lazy_z', '_lazy_a', '_lazy_dy', '_bwd_partials', '_deferred', '_q_stash')
# what a strict _take raises for an entry that belongs to another tensor (the other slots' takers fall back silently)
_MISMATCH = {'_lazy_z': 'lazy z: the parked junction is not this convolution\'s input',
             '_lazy_a': 'lazy a: the parked BatchNorm output is not this convolution\'s input',
             '_lazy_dy': 'lazy dy: the parked gradient does not belong to this convolution\'s output '
                         '(stale mailbox entry or a second consumer)',
             '_deferred': 'deferred shortcut BatchNorm met a junction that cannot apply it'}


def _owner_key(t):
    return t.data_ptr(), tuple(t.shape), t.dtype


def _park(mod, slot, owner, record):
    """Leave `record` on `mod` for the operator that will hold the tensor `owner`."""
    if slot not in _SLOTS:
        raise _lib.ConvNetHipError('unknown per-step mailbox slot %r' % (slot,))
    mod.__dict__[slot] = (_owner_key(owner), record)


def _take(mod, slot, owner=None, strict=True):
    """The record parked in `slot` (taken: a second call returns None).  owner: the tensor - or its _owner_key - the entry
    must have been parked for; an entry of another tensor raises the slot's message when strict, else it is dropped."""
    entry = mod.__dict__.pop(slot, None)
    if entry is None:
        return None
    if owner is not None and entry[0] != (owner if isinstance(owner, tuple) else _owner_key(owner)):
        if strict:
            raise _lib.ConvNetHipError(_MISMATCH[slot])
        return None
    return entry[1]


def _refuse_parked(mod, who):
    """For an operator that takes part in no fusion: whatever was parked on its module is an error."""
    for slot in _SLOTS:
        if mod.__dict__.get(slot) is not None:
            raise _lib.ConvNetHipError('%s: a %s hand-off was parked for it (it takes part in no fusion)' % (who, slot[1:]))


def stats_pivot(conv_mod):
    """The running mean of the BatchNorm that consumes this convolution's output (wired by the model as
    conv.stats_bn): the pivot of the centred statistics the epilogue emits.  None: plain sums."""
    bn = getattr(conv_mod, 'stats_bn', None)
    if bn is None or not CENTERED_STATS or not getattr(bn, 'track_running_stats', False) \
            or getattr(bn, 'running_mean', None) is None or _sync_group(bn) is not None:
        return None
    # fp32 storage only: with 16-bit storage y itself carries 2^-8 (2^-11) of relative rounding, so once |mean| >> sigma
    # the information is gone before any sum is taken, and the epilogue's pivot loads cost the bf16 step 0.3 %
    if getattr(conv_mod, 'compute_dtype', None) != torch.float32 and CENTERED_STATS != 'all':
        return None
    return bn.running_mean


def _halo3x3_ok(x, C, K, R, S, stride, pad):
    return (CONV3X3_HALO and (R, S) == (3, 3) and tuple(stride) == (1, 1) and tuple(pad) == (1, 1)
            and _L().cn_conv3x3_c64_ok(x.shape[1], x.shape[2], C, K, dtype_code(x.dtype)))


def conv2d_fwd(x, w_krsc, bias, K, R, S, stride, pad, out_f32=False, relu=False, bn_stats=False, pivot=None):
    N, H, W, C = x.shape
    P, Q = conv_out_hw(H, W, R, S, stride, pad)
    y = torch.empty((N, P, Q, K), dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    if CONV1X1_STREAM and bias is None and not out_f32 and not relu and pivot is None and (R, S) == (1, 1) \
            and tuple(stride) == (1, 1) and tuple(pad) == (0, 0) \
            and _L().cn_conv1x1_stream_fwd_ok(C, K, dtype_code(x.dtype)):
        L = _L()
        partial, rows = _stats_partial(bn_stats, K, x.device, L.cn_conv1x1_stream_fwd_rows, N, H, W, K)
        PROFILER.run(_last_kernel(), 1, 2.0 * N * P * Q * K * C,
                     x.numel() * _esize(x) + y.numel() * _esize(y) + K * C * _esize(x),
                     lambda: L.cn_conv1x1_stream_fwd(ptr(x), ptr(w_krsc), ptr(y), N, H, W, C, K, dtype_code(x.dtype),
                                                     ptr(partial), rows, stream_of(x)),
                     x.device, detail=_conv_detail('fwd', C, H, K, R, stride))
        _park_stats(y, partial, rows)
        return y
    if bias is None and not out_f32 and not relu and pivot is None and _halo3x3_ok(x, C, K, R, S, stride, pad):
        L = _L()
        partial, rows = _stats_partial(bn_stats, K, x.device, L.cn_conv3x3_c64_rows, N, H)
        PROFILER.run(_last_kernel(), 1, 2.0 * N * P * Q * K * C * R * S,
                     x.numel() * _esize(x) + y.numel() * _esize(y) + K * R * S * C * _esize(x),
                     lambda: L.cn_conv3x3_c64(ptr(x), ptr(w_krsc), ptr(y), N, H, W, dtype_code(x.dtype), 0,
                                              ptr(partial), rows, stream_of(x)),
                     x.device, detail=_conv_detail('fwd', C, H, K, R, stride))
        _park_stats(y, partial, rows)
        return y
    if bn_stats and not out_f32:
        L = _L()
        partial, rows = _stats_partial(True, K, x.device, L.cn_conv2d_bnstats_rows, N * P * Q)
        PROFILER.run(_last_kernel(),
                     1, 2.0 * N * P * Q * K * C * R * S,
                     x.numel() * _esize(x) + y.numel() * _esize(y) + K * R * S * C * _esize(x) + partial.numel() * 4,
                     (lambda: L.cn_conv2d_fwd_bnstats(ptr(x), ptr(w_krsc), ptr(y), ptr(bias), N, H, W, C, K, R, S,
                                                      stride[0], stride[1], pad[0], pad[1], dtype_code(x.dtype),
                                                      int(relu), ptr(partial), rows, stream_of(x))) if pivot is None else
                     (lambda: L.cn_conv2d_fwd_bnstats_centered(ptr(x), ptr(w_krsc), ptr(y), ptr(bias), N, H, W, C,
                                                               K, R, S, stride[0], stride[1], pad[0], pad[1],
                                                               dtype_code(x.dtype), int(relu), ptr(partial), rows,
                                                               ptr(pivot), stream_of(x))),
                     x.device, detail=_conv_detail('fwd', C, H, K, R, stride))
        _park_stats(y, partial, rows, pivot)
        return y
    PROFILER.run(_last_kernel(),
                 1, 2.0 * N * P * Q * K * C * R * S,
                 x.numel() * _esize(x) + y.numel() * _esize(y) + K * R * S * C * _esize(x),
                 lambda: _L().cn_conv2d_fwd(ptr(x), ptr(w_krsc), ptr(y), ptr(bias), N, H, W, C, K, R, S,
                                            stride[0], stride[1], pad[0], pad[1], dtype_code(x.dtype),
                                            int(out_f32), int(relu), stream_of(x)),
                 x.device, detail=_conv_detail('fwd', C, H, K, R, stride))
    return y


def conv2d_fwd_lazyz(lz, w_krsc, K, bn_stats=False, pivot=None):
    """conv1x1(z) with z = relu(bn(y) + residual) formed on the operand load and stored by the kernel
    (cn_conv2d_fwd_lazyz).  lz: the junction's parked state (BatchNormActFunction.forward)."""
    y3, res, stats, res_stats, z, mask, relu = LazyZ(*lz)
    N, H, W, C = y3.shape
    out = torch.empty((N, H, W, K), dtype=y3.dtype, device=y3.device)
    L = _L()
    partial, rows = _stats_partial(bn_stats, K, y3.device, L.cn_conv2d_bnstats_rows, N * H * W)
    nb = y3.numel() * _esize(y3)
    PROFILER.run(_last_kernel(' [lazy z]'), 1, 2.0 * N * H * W * K * C,
                 3 * nb + (mask.numel() if mask is not None else 0) + out.numel() * _esize(out) + K * C * _esize(y3)
                 + (partial.numel() * 4 if partial is not None else 0),
                 lambda: L.cn_conv2d_fwd_lazyz(ptr(y3), ptr(res), ptr(stats), ptr(res_stats), int(relu), ptr(z),
                                               ptr(mask), ptr(w_krsc), ptr(out), N, H, W, C, K, dtype_code(y3.dtype),
                                               ptr(partial), rows, ptr(pivot), stream_of(y3)),
                 y3.device, detail=_conv_detail('fwd', C, H, K, 1, (1, 1)))
    _park_stats(out, partial, rows, pivot)
    return out


# "Lazy a" (round 3, third session): an INNER BatchNorm (no residual, ReLU) whose consumer is a 1x1 convolution on the
# streaming forward kernel only finalises its statistics; the convolution forms a = relu(y * scale + shift) on its
# operand path and writes it as a side output (cn_conv1x1_stream_fwd_lazya): the apply pass - one read of y, one write
# of a - and the convolution's read of a become one read of y and one write of a.  Same scope rule as lazy z (the
# consumer runs next by construction of the block's forward).
LAZY_A = flags.on('lazy_a')
LAZY_A_3X3 = flags.text('lazy_a') != '1x1'      # ('1x1': the streaming 1x1 consumers only)


def lazy_a_consumer_ok(conv, y):
    """conv (the module behind an inner BatchNorm whose input is y, NHWC) will run on the streaming 1x1 forward kernel
    or on the 64-channel 3x3 halo kernel."""
    C, dtype = y.shape[-1], y.dtype
    if conv is None or getattr(conv, 'bias', None) is not None or not conv.training or getattr(conv, 'out_f32', False) \
            or conv.in_channels != C or stats_pivot(conv) is not None or dtype not in (torch.bfloat16, torch.float16) \
            or getattr(conv, 'stride', None) != (1, 1):
        return False
    if getattr(conv, 'kernel_size', None) == (1, 1) and conv.padding == (0, 0):
        return (CONV1X1_STREAM
                and bool(_L().cn_conv1x1_stream_fwd_ok(C, conv.out_channels, dtype_code(dtype))))
    if getattr(conv, 'kernel_size', None) == (3, 3) and conv.padding == (1, 1):
        return (CONV3X3_HALO and LAZY_A_3X3 and bool(_L().cn_conv3x3_c64_ok(y.shape[1], y.shape[2], C, conv.out_channels, dtype_code(dtype))))
    return False


def conv2d_fwd_lazya(la, w_krsc, K, bn_stats=False, kernel=(1, 1)):
    """la = (bn_y, stats, a, relu) parked by BatchNormActFunction: y = conv(relu?(bn_y * scale + shift)), a written
    (1x1: the streaming kernel; 3x3: the 64-channel halo kernel)."""
    bn_y, stats, a, relu = LazyA(*la)
    N, H, W, C = bn_y.shape
    L = _L()
    y = torch.empty((N, H, W, K), dtype=bn_y.dtype, device=bn_y.device)
    if tuple(kernel) == (3, 3):
        partial, rows = _stats_partial(bn_stats, K, bn_y.device, L.cn_conv3x3_c64_rows, N, H)
        PROFILER.run(_last_kernel(' [lazy a]'), 1, 2.0 * N * H * W * K * C * 9,
                     2 * bn_y.numel() * _esize(bn_y) + y.numel() * _esize(y) + K * 9 * C * _esize(bn_y),
                     lambda: L.cn_conv3x3_c64_lazya(ptr(bn_y), ptr(stats), int(relu), ptr(a), ptr(w_krsc), ptr(y),
                                                    N, H, W, dtype_code(bn_y.dtype), ptr(partial), rows,
                                                    stream_of(bn_y)),
                     bn_y.device, detail=_conv_detail('fwd', C, H, K, 3, (1, 1)))
        _park_stats(y, partial, rows)
        return y
    partial, rows = _stats_partial(bn_stats, K, bn_y.device, L.cn_conv1x1_stream_fwd_rows, N, H, W, K)
    PROFILER.run(_last_kernel(' [lazy a]'), 1, 2.0 * N * H * W * K * C,
                 2 * bn_y.numel() * _esize(bn_y) + y.numel() * _esize(y) + K * C * _esize(bn_y),
                 lambda: L.cn_conv1x1_stream_fwd_lazya(ptr(bn_y), ptr(stats), int(relu), ptr(a), ptr(w_krsc), ptr(y),
                                                       N, H, W, C, K, dtype_code(bn_y.dtype), ptr(partial), rows,
                                                       stream_of(bn_y)),
                 bn_y.device, detail=_conv_detail('fwd', C, H, K, 1, (1, 1)))
    _park_stats(y, partial, rows)
    return y


def lazy_z_consumer_ok(conv):
    """conv can take an unapplied junction as its input (cn_conv2d_fwd_lazyz's shape limits)."""
    return (conv is not None and getattr(conv, 'kernel_size', None) == (1, 1) and getattr(conv, 'stride', None) == (1, 1)
            and getattr(conv, 'padding', None) == (0, 0) and getattr(conv, 'bias', None) is None
            and conv.out_channels <= 128 and conv.in_channels <= 512 and conv.training
            and not getattr(conv, 'out_f32', False))


def conv2d_dgrad(dy, w_crsk, x_shape, K, R, S, stride, pad, addend=None, bn=None, addend_sub=1):
    """dx (NHWC).  With bn = (bn_y, bn_mask_or_None, bn_stats[4C], relu) the epilogue also does the
    reduction half of that BatchNorm's backward: returns (g = dx*relu_mask, partial, rows).
    addend_sub = 2: `addend` holds only the even (h, w) pixels of a gradient that is zero elsewhere."""
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    name = _last_kernel()
    detail = _conv_detail('dgrad', C, H, K, R, stride)
    flops = 2.0 * dy.numel() * C * R * S
    nbytes = dy.numel() * _esize(dy) + dx.numel() * _esize(dx) + K * R * S * C * _esize(dy) \
        + (addend.numel() * _esize(addend) if addend is not None else 0)
    if addend is not None and addend_sub == 2:
        assert tuple(addend.shape) == (N, (H + 1) // 2, (W + 1) // 2, C), 'subsampled addend shape'
    if bn is None and addend is None and _halo3x3_ok(dy, K, C, R, S, stride, pad) and tuple(dy.shape[1:3]) == (H, W):
        PROFILER.run(name, 1, flops, nbytes,
                     lambda: _L().cn_conv3x3_c64(ptr(dy), ptr(w_crsk), ptr(dx), N, H, W, dtype_code(dy.dtype), 1, None,
                                                 0, stream_of(dy)),
                     dy.device, detail=detail)
        return dx
    if bn is None:
        PROFILER.run(name, stride[0] * stride[1], flops, nbytes,
                     lambda: _L().cn_conv2d_dgrad_sa(ptr(dy), ptr(w_crsk), ptr(dx), ptr(addend), int(addend_sub), N, H,
                                                     W, C, K, R, S, stride[0], stride[1], pad[0], pad[1],
                                                     dtype_code(dy.dtype), 0, stream_of(dy)),
                     dy.device, detail=detail)
        return dx
    bn_y, bn_mask, bn_stats, bn_relu = BnBwdOperands(*bn)
    L = _L()
    if JDGRAD and (R, S) == (1, 1) and tuple(stride) == (1, 1) and tuple(pad) == (0, 0) and bn_mask is not None \
            and addend is not None and L.cn_conv2d_dgrad_junction_ok(C, K, dtype_code(dy.dtype)):
        rows = L.cn_conv2d_dgrad_junction_rows_k(N, H, W, C, K)
        partial = torch.empty((rows, 2 * C), dtype=torch.float32, device=dy.device)
        PROFILER.run(_last_kernel(), 1, flops, nbytes + dx.numel() * _esize(dx) + partial.numel() * 4,
                     lambda: L.cn_conv2d_dgrad_junction(ptr(dy), ptr(w_crsk), ptr(dx), ptr(addend), int(addend_sub), N,
                                                        H, W, C, K, dtype_code(dy.dtype), ptr(bn_y), ptr(bn_mask),
                                                        ptr(bn_stats), ptr(partial), rows, stream_of(dy)),
                     dy.device, detail=detail)
        COUNTERS['jdgrad'] = COUNTERS.get('jdgrad', 0) + 1
        return dx, partial, rows
    rows = L.cn_conv2d_dgrad_bnbwd_rows(N, H, W, C, stride[0], stride[1])
    partial = torch.empty((rows, 2 * C), dtype=torch.float32, device=dy.device)
    PROFILER.run(name, stride[0] * stride[1], flops, nbytes + dx.numel() * _esize(dx) + partial.numel() * 4,
                 lambda: L.cn_conv2d_dgrad_bnbwd_sa(ptr(dy), ptr(w_crsk), ptr(dx), ptr(addend), int(addend_sub), N, H,
                                                    W, C, K, R, S, stride[0], stride[1], pad[0], pad[1],
                                                    dtype_code(dy.dtype), ptr(bn_y), ptr(bn_mask), ptr(bn_stats),
                                                    int(bn_relu), ptr(partial), rows, stream_of(dy)),
                 dy.device, detail=detail)
    return dx, partial, rows


def _wgrad_two_phase(call, device, flops, bytes_partial, bytes_reduce, detail, suffix=''):
    """A weight-gradient entry point whose call() makes two launches: partial products, then the fixed-order reduction of
    the splits.  Profiled, the two are timed separately - measurement-only knob "wgrad_phase" - so each is reported under
    its own kernel name."""
    if not (PROFILER.enabled and device.type == 'cuda'):
        return call()
    L = _L()
    L.cn_set_option(b'wgrad_phase', 1)
    try:
        PROFILER.run(_last_kernel(suffix), 1, flops, bytes_partial, call, device, detail=detail)
        L.cn_set_option(b'wgrad_phase', 2)
        PROFILER.run('wgrad_reduce_kernel', 1, 0.0, bytes_reduce, call, device, detail=detail + ' [reduce]')
    finally:
        L.cn_set_option(b'wgrad_phase', 0)


def conv2d_wgrad(x, dy, dw_krsc, c_real, K, R, S, stride, pad, beta=1.0, scale=1.0, tag='main'):
    """dw_krsc (fp32, [K][R][S][c_real] memory order) = beta*dw + scale*wgrad."""
    N, H, W, C = x.shape
    code = dtype_code(x.dtype)
    L = _L()
    need = L.cn_conv2d_wgrad_workspace(N, H, W, C, K, R, S, stride[0], stride[1], pad[0], pad[1], code)
    ws = workspace(need, x.device, tag)

    def call():
        L.cn_conv2d_wgrad(ptr(x), ptr(dy), ptr(dw_krsc), c_real, N, H, W, C, K, R, S, stride[0], stride[1],
                          pad[0], pad[1], code, beta, scale, ptr(ws), ws.numel() * 4, stream_of(x))
    _wgrad_two_phase(call, x.device, 2.0 * dy.numel() * C * R * S,
                     x.numel() * _esize(x) + dy.numel() * _esize(dy) + float(need), float(need) + K * R * S * c_real * 4,
                     _conv_detail('wgrad', C, H, K, R, stride))


def conv2d_dgrad_lazy(g, bn_y, coef, w_crsk, x_shape, K, R, S, stride, pad):
    """dgrad whose upstream gradient dy = c1*g + c2*bn_y + c3 is formed on the operand load (cn_conv2d_dgrad_lazy)."""
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
    if (R, S) == (1, 1) and tuple(stride) == (1, 1) and tuple(pad) == (0, 0) and tuple(g.shape[1:3]) == (H, W) \
            and _L().cn_conv2d_dgrad_lazy_stream_ok(C, K, dtype_code(g.dtype)):
        PROFILER.run(_last_kernel(' [lazy dy]'), 1, 2.0 * g.numel() * C,
                     2 * g.numel() * _esize(g) + dx.numel() * _esize(dx) + K * C * _esize(g),
                     lambda: _L().cn_conv2d_dgrad_lazy_stream(ptr(g), ptr(bn_y), ptr(coef), ptr(w_crsk), ptr(dx), N, H, W,
                                                              C, K, dtype_code(g.dtype), stream_of(g)),
                     g.device, detail=_conv_detail('dgrad', C, H, K, R, stride))
        return dx
    PROFILER.run(_last_kernel(' [lazy dy]'), stride[0] * stride[1], 2.0 * g.numel() * C * R * S,
                 2 * g.numel() * _esize(g) + dx.numel() * _esize(dx) + K * R * S * C * _esize(g),
                 lambda: _L().cn_conv2d_dgrad_lazy(ptr(g), ptr(bn_y), ptr(coef), ptr(w_crsk), ptr(dx), N, H, W, C, K,
                                                   R, S, stride[0], stride[1], pad[0], pad[1], dtype_code(g.dtype),
                                                   stream_of(g)),
                 g.device, detail=_conv_detail('dgrad', C, H, K, R, stride))
    return dx


def conv2d_wgrad_lazy(x, g, bn_y, coef, dw_krsc, c_real, K, R, S, stride, pad, beta=1.0, scale=1.0, tag='main'):
    """wgrad whose dy operand is formed on load from (g, bn_y, coef) (cn_conv2d_wgrad_lazy)."""
    N, H, W, C = x.shape
    code = dtype_code(x.dtype)
    L = _L()
    need = L.cn_conv2d_wgrad_workspace(N, H, W, C, K, R, S, stride[0], stride[1], pad[0], pad[1], code)
    ws = workspace(need, x.device, tag)
    PROFILER.run(_last_kernel(' [lazy dy] (+wgrad_reduce)'), 2, 2.0 * g.numel() * C * R * S,
                 x.numel() * _esize(x) + 2 * g.numel() * _esize(g) + float(need),
                 lambda: L.cn_conv2d_wgrad_lazy(ptr(x), ptr(g), ptr(bn_y), ptr(coef), ptr(dw_krsc), c_real, N, H, W, C,
                                                K, R, S, stride[0], stride[1], pad[0], pad[1], code, beta, scale,
                                                ptr(ws), ws.numel() * 4, stream_of(x)),
                 x.device, detail=_conv_detail('wgrad', C, H, K, R, stride))


def conv2d_bwd1x1_lazy(x, g, bn_y, coef, w_crsk, dw_krsc, K, beta=1.0, scale=1.0):
    """dx and the weight gradient of a 1x1 / stride-1 convolution for the lazy upstream gradient (g, bn_y, coef), one
    pass over g and bn_y (cn_conv2d_bwd1x1_lazy)."""
    N, H, W, C = x.shape
    code = dtype_code(x.dtype)
    L = _L()
    need = L.cn_conv2d_bwd1x1_lazy_workspace(N, H, W, C, K)
    ws = workspace(need, x.device, 'main')
    dx = torch.empty_like(x)
    w_krsc = _BN_Y_PRODUCER[0]      # bn_y = conv1x1(x, w): recomputed, not read (its FLOPs are not algorithmic work)

    def call():
        if w_krsc is not None:
            L.cn_conv2d_bwd1x1_lazy_ry(ptr(x), ptr(g), ptr(coef), ptr(w_crsk), ptr(w_krsc), ptr(dx), ptr(dw_krsc), N, H,
                                       W, C, K, code, beta, scale, ptr(ws), ws.numel() * 4, stream_of(x))
        else:
            L.cn_conv2d_bwd1x1_lazy(ptr(x), ptr(g), ptr(bn_y), ptr(coef), ptr(w_crsk), ptr(dx), ptr(dw_krsc), N, H, W, C,
                                    K, code, beta, scale, ptr(ws), ws.numel() * 4, stream_of(x))
    _wgrad_two_phase(call, x.device, 4.0 * g.numel() * C,
                     (1 if w_krsc is not None else 2) * g.numel() * _esize(g) + 2 * x.numel() * _esize(x) + float(need),
                     float(need) + K * C * 4, _conv_detail('dgrad+wgrad', C, H, K, 1, (1, 1)), suffix=' [lazy dy]')
    return dx


# grouped 3x3 convolutions (csrc/gconv.hip): filter w [K][3][3][C/g] in the compute dtype (the KRSC copy), stride 1 or 2,
# padding 1.  FLOPs are the true grouped ones (2 * 9 * C/g per output element), bytes the algorithmic traffic.
def gconv2d_ok(C, K, groups, kernel_size, stride, padding, dtype):
    return bool(_L().cn_gconv2d_ok(C, K, groups, kernel_size[0], kernel_size[1], stride[0], stride[1], padding[0],
                                   padding[1], dtype_code(dtype)))


def gconv2d_fwd(x, w, K, groups, stride):
    N, H, W, C = x.shape
    P, Q = conv_out_hw(H, W, 3, 3, (stride, stride), (1, 1))
    y = torch.empty((N, P, Q, K), dtype=x.dtype, device=x.device)
    cg = C // groups
    PROFILER.run(_last_kernel(), 1, 2.0 * N * P * Q * K * 9 * cg,
                 x.numel() * _esize(x) + y.numel() * _esize(y) + K * 9 * cg * _esize(x),
                 lambda: _L().cn_gconv2d_fwd(ptr(x), ptr(w), ptr(y), N, H, W, C, K, groups, stride,
                                             dtype_code(x.dtype), stream_of(x)),
                 x.device, detail=_conv_detail('gfwd', C, H, K, 3, (stride, stride)))
    return y


def gconv2d_dgrad(dy, w, x_shape, K, groups, stride):
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    PROFILER.run(_last_kernel(), 1, 2.0 * dy.numel() * 9 * (C // groups),
                 dy.numel() * _esize(dy) + dx.numel() * _esize(dx) + K * 9 * (C // groups) * _esize(dy),
                 lambda: _L().cn_gconv2d_dgrad(ptr(dy), ptr(w), ptr(dx), N, H, W, C, K, groups, stride,
                                               dtype_code(dy.dtype), stream_of(dy)),
                 dy.device, detail=_conv_detail('gdgrad', C, H, K, 3, (stride, stride)))
    return dx


def gconv2d_wgrad(x, dy, dw, K, groups, stride, beta=1.0, scale=1.0, tag='main'):
    """dw (fp32, [K][3][3][C/g] memory order) = beta*dw + scale*wgrad."""
    N, H, W, C = x.shape
    code = dtype_code(x.dtype)
    L = _L()
    need = L.cn_gconv2d_wgrad_workspace(N, H, W, C, K, groups, stride, code)
    ws = workspace(need, x.device, tag)
    PROFILER.run(_last_kernel(), 2, 2.0 * dy.numel() * 9 * (C // groups),
                 x.numel() * _esize(x) + dy.numel() * _esize(dy) + 2.0 * need + K * 9 * (C // groups) * 4,
                 lambda: L.cn_gconv2d_wgrad(ptr(x), ptr(dy), ptr(dw), N, H, W, C, K, groups, stride, code, beta,
                                            scale, ptr(ws), ws.numel() * 4, stream_of(x)),
                 x.device, detail=_conv_detail('gwgrad', C, H, K, 3, (stride, stride)))


# depthwise 3x3 convolutions (csrc/dwconv.hip): filter w_rsc [3][3][C] in the compute dtype (the tap-major copy), bias [C]
# fp32 or None, stride 1 or 2, padding 1.  2 * 9 FLOPs per output element, bytes the algorithmic traffic.
DWCONV = flags.on('dwconv')


def dwconv_ok(C, kernel_size, stride, padding, dtype):
    return bool(_L().cn_dwconv3x3_ok(C, kernel_size[0], kernel_size[1], stride[0], stride[1], padding[0], padding[1],
                                     dtype_code(dtype)))


def dwconv_fwd(x, w_rsc, bias, stride):
    N, H, W, C = x.shape
    P, Q = conv_out_hw(H, W, 3, 3, (stride, stride), (1, 1))
    y = torch.empty((N, P, Q, C), dtype=x.dtype, device=x.device)
    PROFILER.run(_last_kernel(), 1, 2.0 * y.numel() * 9,
                 x.numel() * _esize(x) + y.numel() * _esize(y) + C * 9 * _esize(x),
                 lambda: _L().cn_dwconv3x3_fwd(ptr(x), ptr(w_rsc), ptr(bias), ptr(y), N, H, W, C, stride,
                                               dtype_code(x.dtype), stream_of(x)),
                 x.device, detail=_conv_detail('dwfwd', C, H, C, 3, (stride, stride)))
    return y


def dwconv_dgrad(dy, w_rsc, x_shape, stride):
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    PROFILER.run(_last_kernel(), 1, 2.0 * dy.numel() * 9,
                 dy.numel() * _esize(dy) + dx.numel() * _esize(dx) + C * 9 * _esize(dy),
                 lambda: _L().cn_dwconv3x3_dgrad(ptr(dy), ptr(w_rsc), ptr(dx), N, H, W, C, stride,
                                                 dtype_code(dy.dtype), stream_of(dy)),
                 dy.device, detail=_conv_detail('dwdgrad', C, H, C, 3, (stride, stride)))
    return dx


def dwconv_wgrad_split(x_shape, stride, dtype):
    """Number of pixel slabs (workspace partials) the weight gradient of this shape is split into."""
    N, H, W, C = x_shape
    return _L().cn_dwconv3x3_wgrad_workspace(N, H, W, C, stride, dtype_code(dtype)) // (C * 10 * 4)


def dwconv_wgrad(x, dy, dw, dbias, stride, beta=1.0, scale=1.0, tag='main'):
    """dw (fp32, [C][3][3] memory order: the parameter's own) = beta*dw + scale*wgrad; dbias (fp32 [C] or None) likewise."""
    N, H, W, C = x.shape
    code = dtype_code(x.dtype)
    L = _L()
    need = L.cn_dwconv3x3_wgrad_workspace(N, H, W, C, stride, code)
    ws = workspace(need, x.device, tag)
    PROFILER.run(_last_kernel(' (+wgrad_reduce)'), 3 if dbias is not None else 2, 2.0 * dy.numel() * 10,
                 x.numel() * _esize(x) + dy.numel() * _esize(dy) + 2.0 * need + C * 10 * 4,
                 lambda: L.cn_dwconv3x3_wgrad(ptr(x), ptr(dy), ptr(dw), ptr(dbias), N, H, W, C, stride, code, beta, scale,
                                              ptr(ws), ws.numel() * 4, stream_of(x)),
                 x.device, detail=_conv_detail('dwwgrad', C, H, C, 3, (stride, stride)))


def weight_prep(w_master_krsc, w_krsc, w_crsk, Co, taps, c_real, c_pad):
    PROFILER.run('weight_prep', 1, 0.0, Co * taps * c_real * 4 + Co * taps * c_pad * _esize(w_krsc) * (2 if w_crsk is not None else 1),
                 lambda: _L().cn_weight_prep(ptr(w_master_krsc), ptr(w_krsc), ptr(w_crsk), Co, taps, c_real,
                                             c_pad, dtype_code(w_krsc.dtype), stream_of(w_krsc)), w_krsc.device)


def colsum(x2d, out, beta=1.0, scale=1.0):
    M, C = x2d.shape
    L = _L()
    ws = workspace(L.cn_colsum_workspace(C), x2d.device, 'colsum')
    L.cn_colsum(ptr(x2d), ptr(out), M, C, dtype_code(x2d.dtype), beta, scale, ptr(ws), stream_of(x2d))


def nchw_to_nhwc(x_nchw, dtype, c_pad=None):
    """fp32 NCHW (the loader / reference layout) -> NHWC compute dtype, channels zero-padded."""
    N, C, H, W = x_nchw.shape
    ch = _lib.chunk_elems(dtype)
    if c_pad is None:
        c_pad = (C + ch - 1) // ch * ch
    x_nchw = x_nchw.contiguous()
    if x_nchw.dtype != torch.float32:
        raise _lib.ConvNetHipError('nchw_to_nhwc expects float32 input, got %s' % x_nchw.dtype)
    y = torch.empty((N, H, W, c_pad), dtype=dtype, device=x_nchw.device)
    PROFILER.run('nchw_to_nhwc', 1, 0.0, x_nchw.numel() * 4 + y.numel() * _esize(y),
                 lambda: _L().cn_nchw_to_nhwc(ptr(x_nchw), ptr(y), N, C, H, W, c_pad, dtype_code(dtype),
                                              stream_of(x_nchw)), x_nchw.device)
    return y


def normalize_lut(mean, std):
    """lut[c][u] = ToTensor + Normalize of byte u in channel c, with the reference pipeline's own fp32 operations
    (`.float().div_(255)`, then `(t - mean) / std`): what cn_u8_nhwc_to_nchw_lut looks up."""
    u = torch.arange(256, dtype=torch.uint8).float().div_(255.0).view(1, 256)
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1)
    return ((u - m) / s).contiguous()


def resize_crops(batch):
    """A device_resize loader's batch (data.collate_crops, already on the device) -> uint8 [B, S, S, C]: PIL's BILINEAR
    resize of every crop, bit for bit (cn_resize_u8_crops), mirrored where the loader drew a horizontal flip."""
    px, meta, tables = batch['crops'], batch['meta'], batch['tables']
    row_owner, row_off = batch['row_owner'], batch['row_off']
    S, C = (int(v) for v in batch['size'].tolist())
    B, rows = meta.shape[0], row_owner.shape[0]
    tmp = torch.empty(rows * S * C, dtype=torch.uint8, device=px.device)
    out = torch.empty((B, S, S, C), dtype=torch.uint8, device=px.device)
    PROFILER.run('resize_u8_crops', 2, 0.0, px.numel() + 2 * tmp.numel() + out.numel(),
                 lambda: _L().cn_resize_u8_crops(ptr(px), ptr(meta), ptr(tables), ptr(row_owner), ptr(row_off), ptr(tmp),
                                                 ptr(out), B, rows, S, C, stream_of(px)), px.device)
    return out


def resize_views(batch):
    """A device_resize loader's batch with duplicates > 1 (data.collate_views, already on the device) -> uint8
    [B * D, S, S, C], sample-major: every view is PIL's BILINEAR resize of its own box of the sample's shared source region,
    bit for bit (cn_resize_u8_views), mirrored where the loader drew a flip.  `meta_host` (the meta table in host memory,
    which the entry point checks the views' bounds on) travels with the batch; a host batch's own meta serves."""
    px, meta, tables, row_owner = batch['views'], batch['meta'], batch['tables'], batch['row_owner']
    meta_host = batch.get('meta_host')
    if meta_host is None:
        if meta.is_cuda:
            raise _lib.ConvNetHipError('resize_views: a device batch needs meta_host (the meta table in host memory)')
        meta_host = meta
    S, C = (int(v) for v in batch['size'].tolist()[:2])
    meta_host = meta_host.contiguous()
    if meta_host.is_cuda or meta_host.dtype != torch.int64 or tuple(meta_host.shape) != tuple(meta.shape) or meta.dim() != 2 \
            or meta.shape[1] != 10:
        raise _lib.ConvNetHipError('resize_views: meta / meta_host must be int64 [V, 10], got %s / %s'
                                   % (tuple(meta.shape), tuple(meta_host.shape)))
    V, rows = meta.shape[0], row_owner.shape[0]
    tmp = torch.empty(rows * S * C, dtype=torch.uint8, device=px.device)
    out = torch.empty((V, S, S, C), dtype=torch.uint8, device=px.device)
    PROFILER.run('resize_u8_views', 2, 0.0, px.numel() + 2 * tmp.numel() + out.numel(),
                 lambda: _L().cn_resize_u8_views(ptr(px), ptr(meta), ptr(tables), ptr(row_owner), ptr(tmp), ptr(out),
                                                 ptr(meta_host), px.numel(), tables.numel(), V, rows, S, C, stream_of(px)),
                 px.device)
    return out


def u8_nhwc_to_nchw(x_u8, lut):
    """uint8 [N, H, W, C] crops -> the normalised fp32 [N, C, H, W] batch (device-side ToTensor + Normalize)."""
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 4:
        raise _lib.ConvNetHipError('u8_nhwc_to_nchw expects uint8 [N, H, W, C], got %s %s' % (x_u8.dtype, tuple(x_u8.shape)))
    N, H, W, C = x_u8.shape
    x_u8 = x_u8.contiguous()
    lut = lut.to(device=x_u8.device, dtype=torch.float32).contiguous()
    if tuple(lut.shape) != (C, 256):
        raise _lib.ConvNetHipError('u8_nhwc_to_nchw: lut %s for %d channels' % (tuple(lut.shape), C))
    y = torch.empty((N, C, H, W), dtype=torch.float32, device=x_u8.device)
    PROFILER.run('u8_nhwc_to_nchw', 1, 0.0, x_u8.numel() + y.numel() * 4,
                 lambda: _L().cn_u8_nhwc_to_nchw_lut(ptr(x_u8), ptr(y), N, H, W, C, ptr(lut), stream_of(x_u8)), x_u8.device)
    return y


AUGMENT_PARAMS = 8      # == CN_AUGMENT_PARAMS of include/convnet_hip.h: top, left, flip, y1, y2, x1, x2, 0


def check_crop_params(idx, params, N, S, pad):
    """Range check of a crop_flip_normalize batch on its HOST copies (idx int32 [V], params int32 [V, AUGMENT_PARAMS]):
    raises before anything is uploaded or launched."""
    if idx.is_cuda or params.is_cuda:
        raise _lib.ConvNetHipError('crop_flip_normalize: idx / params are checked on their host copies')
    if idx.dtype != torch.int32 or params.dtype != torch.int32 or idx.dim() != 1 or params.dim() != 2 \
            or params.shape[0] != idx.shape[0] or params.shape[1] != AUGMENT_PARAMS or idx.shape[0] == 0:
        raise _lib.ConvNetHipError('crop_flip_normalize: idx must be int32 [V] and params int32 [V, %d], got %s %s / %s %s'
                                   % (AUGMENT_PARAMS, idx.dtype, tuple(idx.shape), params.dtype, tuple(params.shape)))
    if int(idx.min()) < 0 or int(idx.max()) >= N:
        raise _lib.ConvNetHipError('crop_flip_normalize: idx out of range [0, %d)' % N)
    top_left, flip = params[:, 0:2], params[:, 2]
    if int(top_left.min()) < 0 or int(top_left.max()) > 2 * pad:
        raise _lib.ConvNetHipError('crop_flip_normalize: params out of range: top / left must lie in [0, %d]' % (2 * pad))
    if int(flip.min()) < 0 or int(flip.max()) > 1:
        raise _lib.ConvNetHipError('crop_flip_normalize: params out of range: flip must be 0 or 1')
    rect = params[:, 3:7]
    if int(rect.min()) < 0 or int(rect.max()) > S or bool((rect[:, 0] > rect[:, 1]).any()) or bool((rect[:, 2] > rect[:, 3]).any()):
        raise _lib.ConvNetHipError('crop_flip_normalize: params out of range: the cutout rectangle must be clipped to '
                                   '[0, %d] with y1 <= y2, x1 <= x2' % S)


def crop_flip_normalize(data, idx, params, lut, dtype=torch.float32, form='nchw', pad=4, host=None):
    """RandomCrop(S, padding=pad) -> RandomHorizontalFlip -> ToTensor -> Normalize -> Cutout of the reference's CIFAR
    pipeline on a dataset resident in device memory (cn_augment_crop_flip): data uint8 [N, S, S, 3], one view per entry
    of idx / params.  form 'nchw': the loader's fp32 [V, 3, S, S] batch, equal to the host pipeline value for value;
    form 'nhwc': [V, S, S, c_pad] in `dtype` with zero pad channels, the bits nchw_to_nhwc makes of the former.
    idx / params are host tensors (checked here, then uploaded); `host` = (idx, params) in host memory when the
    caller has already uploaded them (the loader: one pinned copy on its own stream)."""
    if data.dtype != torch.uint8 or data.dim() != 4 or data.shape[1] != data.shape[2] or data.shape[3] != 3:
        raise _lib.ConvNetHipError('crop_flip_normalize expects uint8 [N, S, S, 3] data, got %s %s' % (data.dtype, tuple(data.shape)))
    if form not in ('nchw', 'nhwc'):
        raise ValueError("crop_flip_normalize: form must be 'nchw' or 'nhwc', got %r" % (form,))
    if form == 'nchw' and dtype != torch.float32:
        raise _lib.ConvNetHipError('crop_flip_normalize: the nchw form is float32 (the loader batch), got %s' % dtype)
    code = dtype_code(dtype)
    _lib.require_device(data, 'data')
    N, S = data.shape[0], data.shape[1]
    pad = int(pad)
    if pad < 0 or pad > S:
        raise _lib.ConvNetHipError('crop_flip_normalize: pad %d for %d x %d images' % (pad, S, S))
    if tuple(lut.shape) != (3, 256):
        raise _lib.ConvNetHipError('crop_flip_normalize: lut %s, expected (3, 256)' % (tuple(lut.shape),))
    h_idx, h_params = (idx, params) if host is None else host
    check_crop_params(h_idx, h_params, N, S, pad)
    if host is None:
        idx, params = idx.to(data.device), params.to(data.device)
    elif idx.device != data.device or params.device != data.device or tuple(idx.shape) != tuple(h_idx.shape) \
            or tuple(params.shape) != tuple(h_params.shape) or idx.dtype != torch.int32 or params.dtype != torch.int32:
        raise _lib.ConvNetHipError('crop_flip_normalize: the uploaded idx / params do not match their host copies')
    idx, params = idx.contiguous(), params.contiguous()
    lut = lut.to(device=data.device, dtype=torch.float32).contiguous()
    V = idx.shape[0]
    c_pad = _lib.chunk_elems(dtype)
    out = torch.empty((V, 3, S, S) if form == 'nchw' else (V, S, S, c_pad), dtype=dtype, device=data.device)
    PROFILER.run('augment_crop_flip', 1, 0.0, V * S * S * 3 + out.numel() * _esize(out),
                 lambda: _L().cn_augment_crop_flip(ptr(data), data.numel(), ptr(idx), ptr(params), ptr(lut), ptr(out), N, V, S,
                                                   pad, c_pad, code, 0 if form == 'nchw' else 1, stream_of(data)), data.device)
    return out


def nchw_to_pairs(x_nchw, pad):
    """fp32 NCHW (C <= 4) -> zero-padded bf16 pixel-pair image [N, H+2ph, (W+2pw)/2, 8] (cn_nchw_to_pairs)."""
    N, C, H, W = x_nchw.shape
    x_nchw = x_nchw.contiguous()
    if x_nchw.dtype != torch.float32:
        raise _lib.ConvNetHipError('nchw_to_pairs expects float32 input, got %s' % x_nchw.dtype)
    y = torch.empty((N, H + 2 * pad[0], (W + 2 * pad[1]) // 2, 8), dtype=torch.bfloat16, device=x_nchw.device)
    PROFILER.run('nchw_to_pairs', 1, 0.0, x_nchw.numel() * 4 + y.numel() * 2,
                 lambda: _L().cn_nchw_to_pairs(ptr(x_nchw), ptr(y), N, C, H, W, pad[0], pad[1],
                                               stream_of(x_nchw)), x_nchw.device)
    return y


def nhwc_to_nchw(x_nhwc, C=None):
    N, H, W, Cp = x_nhwc.shape
    C = C or Cp
    y = torch.empty((N, C, H, W), dtype=torch.float32, device=x_nhwc.device)
    _L().cn_nhwc_to_nchw(ptr(x_nhwc), ptr(y), N, C, H, W, Cp, dtype_code(x_nhwc.dtype), stream_of(x_nhwc))
    return y


def add_(a, b):
    PROFILER.run('eltwise_add', 1, 0.0, 3 * a.numel() * _esize(a),
                 lambda: _L().cn_eltwise(0, ptr(a), ptr(b), None, a.numel(), dtype_code(a.dtype),
                                         stream_of(a)), a.device)
    return a


def cast_from_f32(x, dtype):
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    _L().cn_cast_from_f32(ptr(x), ptr(y), x.numel(), dtype_code(dtype), stream_of(x))
    return y


def fill_f32_(x, v=0.0):
    _L().cn_fill_f32(ptr(x), x.numel(), float(v), stream_of(x))
    return x


# ---------------------------------------------------------------------------------------------
# autograd Functions.  Parameter gradients are accumulated *by the kernels* straight into the flat
# gradient arena (`mod.grad_view(name)`), so the Functions return None for parameters and autograd
# never runs an accumulation kernel of its own; `mod._notify_grad_ready()` lets the data-parallel
# bucket manager start the all-reduce of a finished bucket while backward continues.

def _input_bn_state(conv_mod, x):
    """(bn module, BnBwdOperands) of the BatchNorm whose output *is* the convolution input `x`
    (wired by the model as conv.input_bn), when that BatchNorm's forward state is still alive and
    belongs to this very tensor; else None."""
    bn_mod = getattr(conv_mod, 'input_bn', None)
    if bn_mod is None:
        return None
    ref = getattr(bn_mod, '_fwd_ctx', None)
    bctx = ref() if ref is not None else None
    if bctx is None or getattr(bctx, 'out_ptr', None) != x.data_ptr():
        return None
    try:
        saved = bctx.saved_tensors
    except RuntimeError:      # already released
        return None
    y, stats = saved[0], saved[1]
    mask = saved[2] if len(saved) > 2 else None
    if tuple(y.shape) != tuple(x.shape) or y.dtype != x.dtype:
        return None
    if bctx.has_res and bctx.relu and mask is None:
        return None
    if y.shape[-1] % _lib.chunk_elems(y.dtype) != 0:
        return None
    return bn_mod, BnBwdOperands(y, mask, stats, bctx.relu)


_ZEROS = {}


def _zero_like_placeholder(x):
    """A storage-free all-zero tensor of x's shape (one cached zero element, expanded): what autograd is handed when the
    real gradient travels through a ResGradHolder."""
    key = (x.device, x.dtype)
    z = _ZEROS.get(key)
    if z is None:
        z = _ZEROS[key] = torch.zeros(1, dtype=x.dtype, device=x.device)
    return z.expand(x.shape)


def _is_zero_placeholder(t):
    z = _ZEROS.get((t.device, t.dtype))
    return z is not None and t.data_ptr() == z.data_ptr() and t.dim() > 0 and all(st == 0 for st in t.stride())


def _submit_wgrad(mod, run, held, dy):
    """A layer's weight gradient run(tag): on the side stream when that is in use - it waits for `dy`'s producer, and
    `held` (the operands; held[0] tells the device) plus whatever scratch run() returns stay referenced until the join -
    else right here; then the gradient is reported ready."""
    x = held[0]
    if SIDE.active(x):
        SIDE.submit(x.device, lambda: held + (run('side') or ()), mod._notify_grad_ready, dy)
    else:
        run('main')
        mod._notify_grad_ready()


class Conv2dFunction(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        mod.ensure_prepared()
        lz, la = _take(mod, '_lazy_z', x), _take(mod, '_lazy_a', x)
        if bias is not None and (lz is not None or la is not None):
            raise _lib.ConvNetHipError(_MISMATCH['_lazy_z' if lz is not None else '_lazy_a'])
        if lz is not None:    # x is a junction output that exists only as (y, residual, statistics): this kernel writes it
            y = conv2d_fwd_lazyz(lz, mod.w_krsc, mod.out_channels, bn_stats=_wants_stats(mod), pivot=stats_pivot(mod))
            COUNTERS['lazy_z'] = COUNTERS.get('lazy_z', 0) + 1
        elif la is not None:   # x is an inner BatchNorm's output that exists only as (y, statistics)
            y = conv2d_fwd_lazya(la, mod.w_krsc, mod.out_channels, bn_stats=_wants_stats(mod), kernel=mod.kernel_size)
            COUNTERS['lazy_a'] = COUNTERS.get('lazy_a', 0) + 1
        else:
            y = conv2d_fwd(x, mod.w_krsc, bias, mod.out_channels, mod.kernel_size[0], mod.kernel_size[1],
                           mod.stride, mod.padding, out_f32=mod.out_f32, bn_stats=_wants_stats(mod),
                           pivot=stats_pivot(mod))
        ctx.mod = mod
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x)
        # the lazy-dy mailbox is matched against THIS output in backward; an entry left by an aborted backward dies here
        ctx.out_key = _owner_key(y)
        _take(mod, '_lazy_dy')
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        lazy = _take(mod, '_lazy_dy', ctx.out_key)     # the BatchNorm behind this conv left dy unformed
        holder = getattr(mod, '_res_holder', None)
        R, S = mod.kernel_size
        if lazy is None and _is_zero_placeholder(dy):
            raise _lib.ConvNetHipError('lazy dy: the gradient placeholder reached a convolution with an empty mailbox '
                                       '(the BatchNorm that parked the gradient is not this convolution\'s consumer)')
        if lazy is not None:
            g, bn_y, coef = lazy
            if tuple(g.shape) != tuple(dy.shape):
                raise _lib.ConvNetHipError(_MISMATCH['_lazy_dy'])
            if JPAIR and (R, S) == (1, 1) and mod.stride == (1, 1) and mod.padding == (0, 0) and ctx.needs_input_grad[0] \
                    and mod.in_channels == x.shape[-1] \
                    and _L().cn_conv2d_bwd1x1_lazy_ok(x.shape[-1], mod.out_channels, dtype_code(x.dtype)):
                # junction pair: both gradients of this convolution in one pass over (g, bn_y), on the backward chain
                if holder is not None and holder.dres is not None:
                    raise _lib.ConvNetHipError('lazy dy met a fused-addend dgrad: the junction layout changed')
                # (the mailbox entry was matched against this convolution's output: without a bias bn_y IS conv1x1(x, w))
                own = JPAIR_RECOMPUTE and not ctx.has_bias and _owner_key(bn_y) == ctx.out_key
                with bn_y_is_output_of(mod.w_krsc if own else None):
                    dx = conv2d_bwd1x1_lazy(x, g, bn_y, coef, mod.w_crsk, mod.grad_view('weight'), mod.out_channels)
                mod._notify_grad_ready()
                COUNTERS['jpair'] = COUNTERS.get('jpair', 0) + 1
                if holder is not None:
                    holder.park(dx)
                return dx, None, None, None
            _submit_wgrad(mod, lambda tag: conv2d_wgrad_lazy(x, g, bn_y, coef, mod.grad_view('weight'), mod.in_channels,
                                                             mod.out_channels, R, S, mod.stride, mod.padding, tag=tag),
                          (x, g, bn_y, coef), coef)
            if not ctx.needs_input_grad[0]:
                return None, None, None, None
            if holder is not None and holder.dres is not None:
                raise _lib.ConvNetHipError('lazy dy met a fused-addend dgrad: the junction layout changed')
            if holder is not None and SUBSAMPLED_SHORTCUT_GRAD and (R, S) == (1, 1) and mod.stride == (2, 2) \
                    and mod.padding == (0, 0):
                N_, H_, W_, C_ = x.shape
                compact = conv2d_dgrad_lazy(g, bn_y, coef, mod.w_crsk, (N_, (H_ + 1) // 2, (W_ + 1) // 2, C_),
                                            mod.out_channels, 1, 1, (1, 1), (0, 0))
                holder.park(compact, 2)
                return _zero_like_placeholder(x), None, None, None
            dx = conv2d_dgrad_lazy(g, bn_y, coef, mod.w_crsk, x.shape, mod.out_channels, R, S, mod.stride, mod.padding)
            if holder is not None:
                holder.park(dx)
            return dx, None, None, None
        dy = dy.contiguous()
        if dy.dtype != x.dtype:  # fp32 logits gradient -> compute dtype
            dy = cast_from_f32(dy, x.dtype)
        if ctx.has_bias:
            colsum(dy.view(-1, mod.out_channels), mod.grad_view('bias'))

        def submit_wgrad():
            _submit_wgrad(mod, lambda tag: conv2d_wgrad(x, dy, mod.grad_view('weight'), mod.in_channels, mod.out_channels,
                                                        R, S, mod.stride, mod.padding, tag=tag), (x, dy), dy)

        def dgrad_part():
            dx = None
            if ctx.needs_input_grad[0]:
                addend, addend_sub = None, 1
                if holder is not None and holder.dres is not None and holder.dres.dtype == dy.dtype \
                        and (holder.dres.shape == x.shape if holder.sub == 1 else
                             tuple(holder.dres.shape) == (x.shape[0], (x.shape[1] + 1) // 2, (x.shape[2] + 1) // 2, x.shape[3])):
                    addend, addend_sub = holder.claim()   # the other branch's gradient, folded into this dgrad epilogue
                elif holder is not None and holder.dres is None and SUBSAMPLED_SHORTCUT_GRAD \
                        and (R, S) == (1, 1) and mod.stride == (2, 2) and mod.padding == (0, 0):
                    # stride-2 1x1 projection shortcut, first of the two gradients that meet at the block input: its input
                    # gradient is zero off the even pixels - compute those on the coarse grid (a stride-1 dgrad), park
                    # them, and hand autograd a storage-free placeholder (ForkFunction returns the other branch's sum)
                    N_, H_, W_, C_ = x.shape
                    compact = conv2d_dgrad(dy, mod.w_crsk, (N_, (H_ + 1) // 2, (W_ + 1) // 2, C_), mod.out_channels, 1, 1,
                                           (1, 1), (0, 0))
                    holder.park(compact, 2)
                    return _zero_like_placeholder(x), None, None, None
                # this dgrad is the last contribution to the gradient of x when x has no other consumer
                # (inner convs) or when the other branch's gradient is being added right here
                final = holder is None or addend is not None
                bn_args = _input_bn_state(mod, x) if (final and FUSE_BN_BWD) else None
                if bn_args is not None and holder is None:
                    bn_args = None      # junctions only (see FUSE_BN_BWD)
                if bn_args is not None:
                    bn_mod, bn = bn_args
                    dx, partial, rows = conv2d_dgrad(dy, mod.w_crsk, x.shape, mod.out_channels, R, S, mod.stride,
                                                     mod.padding, addend=addend, bn=bn, addend_sub=addend_sub)
                    _park(bn_mod, '_bwd_partials', dx, BwdPartials(partial, rows))
                else:
                    dx = conv2d_dgrad(dy, mod.w_crsk, x.shape, mod.out_channels, R, S, mod.stride, mod.padding,
                                      addend=addend, addend_sub=addend_sub)
                if holder is not None and addend is None:
                    holder.park(dx)   # first producer of the fork gradient: park it for the other
            return dx, None, None, None

        # The data gradient is the backward chain's next kernel; the weight gradient only has to start some time.  Launching
        # the chain's kernel FIRST keeps the host-side cost of the side-stream hand-off (fork / mark wait + a second ctypes
        # call, ~40 us) off the chain where the host runs only just ahead of the device (the late, small layers): the
        # rocprofv3 trace showed 10-14 us of idle main queue in front of 26 of these data gradients.  Untraced the effect is at
        # the noise level (14871 vs 14819 img/s, three interleaved rounds); kept because it is the natural order (flag dgrad_first).
        if not DGRAD_FIRST:
            submit_wgrad()
        out = dgrad_part()
        if DGRAD_FIRST:
            submit_wgrad()
        return out


class GroupedConv2dFunction(Function):
    """A grouped 3x3 convolution (ResNeXt's conv2).  It takes part in no fusion: no BatchNorm statistics in its epilogue,
    no lazy operands, no junction pairing - the BatchNorms beside it run their standalone passes.  The weight gradient
    goes to the side stream exactly like Conv2dFunction's."""
    @staticmethod
    def forward(ctx, x, weight, mod):
        mod.ensure_prepared()
        _refuse_parked(mod, 'grouped convolution')
        y = gconv2d_fwd(x, mod.w_krsc, mod.out_channels, mod.groups, mod.stride[0])
        ctx.mod = mod
        ctx.save_for_backward(x)
        COUNTERS['gconv'] = COUNTERS.get('gconv', 0) + 1
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        _refuse_parked(mod, 'grouped convolution')
        if _is_zero_placeholder(dy):
            raise _lib.ConvNetHipError('grouped convolution: a lazy gradient reached it (grouped convs take no fusion)')
        dy = dy.contiguous()
        K, g, st = mod.out_channels, mod.groups, mod.stride[0]

        def submit_wgrad():
            _submit_wgrad(mod, lambda tag: gconv2d_wgrad(x, dy, mod.grad_view('weight'), K, g, st, tag=tag), (x, dy), dy)

        if not DGRAD_FIRST:
            submit_wgrad()
        dx = gconv2d_dgrad(dy, mod.w_krsc, x.shape, K, g, st) if ctx.needs_input_grad[0] else None
        if DGRAD_FIRST:
            submit_wgrad()
        return dx, None, None


class DepthwiseConv2dFunction(Function):
    """A depthwise 3x3 convolution (MobileNet's per-channel filter, with or without bias) on csrc/dwconv.hip.  Like the
    grouped convolution it takes part in no fusion.  The weight AND bias gradients come from one pass (dwconv_wgrad) on the
    side stream; the data gradient is launched first (dgrad_first) and skipped when the input needs none."""
    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        mod.ensure_prepared()
        _refuse_parked(mod, 'depthwise convolution')
        y = dwconv_fwd(x, mod.w_crsk, bias, mod.stride[0])
        ctx.mod = mod
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x)
        COUNTERS['dwconv'] = COUNTERS.get('dwconv', 0) + 1
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        _refuse_parked(mod, 'depthwise convolution')
        if _is_zero_placeholder(dy):
            raise _lib.ConvNetHipError('depthwise convolution: a lazy gradient reached it (depthwise convs take no fusion)')
        dy = dy.contiguous()
        st = mod.stride[0]
        db = mod.grad_view('bias') if ctx.has_bias else None

        def submit_wgrad():
            _submit_wgrad(mod, lambda tag: dwconv_wgrad(x, dy, mod.grad_view('weight'), db, st, tag=tag), (x, dy), dy)

        if not DGRAD_FIRST:
            submit_wgrad()
        need_dx = ctx.needs_input_grad[0] and getattr(mod, 'needs_dgrad', True)
        dx = dwconv_dgrad(dy, mod.w_crsk, x.shape, st) if need_dx else None
        if DGRAD_FIRST:
            submit_wgrad()
        return dx, None, None, None


def _sync_group(mod):
    """(process group, world size) when this BatchNorm synchronises its batch statistics across ranks
    (nn.convert_sync_batchnorm + an initialised process group of more than one rank), else None."""
    sg = getattr(mod, 'sync_group', None)
    if sg is None or not dist.is_available() or not dist.is_initialized():
        return None
    group = None if sg is True else sg
    world = dist.get_world_size(group)
    return (group, world) if world > 1 else None


def _sync_all_reduce(t, group, world):
    """SyncBatchNorm statistics exchange: one in-stream RCCL all-reduce on the compute stream when the
    direct communicator spans this group (no stream hop, no host-side work object), else torch.distributed."""
    from . import comm as _comm
    c = _comm.default()
    if c is not None and t.is_cuda and c.world == world and (group is None or group is c.pg):
        c.allreduce_(t)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


class StemPairConvFunction(Function):
    """The stride-2 stem convolution on the pixel-pair image (ops.nchw_to_pairs): same result as
    Conv2dFunction on the channel-padded NHWC image, with ceil(S/2) instead of S reduction chunks per
    filter row and no bounds tests.  The network input needs no gradient, so backward is wgrad only."""

    @staticmethod
    def forward(ctx, x_pairs, weight, mod):
        K, (R, S) = mod.out_channels, mod.kernel_size
        S2 = (S + 1) // 2
        L = _L()
        wp = torch.empty(K * R * S2 * 8, dtype=torch.bfloat16, device=x_pairs.device)
        L.cn_weight_prep_pairs(ptr(mod.master_view('weight')), ptr(wp), K, R, S, mod.in_channels,
                               stream_of(x_pairs))
        want_stats = _wants_stats(mod)
        N_, Hp_, Jp_, _ = x_pairs.shape
        if STEM_HALO and want_stats and stats_pivot(mod) is None and mod.stride[0] == 2 and x_pairs.dtype == torch.bfloat16 \
                and L.cn_stem_fwd_ok(K, R, S2, Jp_, dtype_code(x_pairs.dtype)):
            P_, Q_ = (Hp_ - R) // 2 + 1, Jp_ - S2 + 1
            y = torch.empty((N_, P_, Q_, K), dtype=x_pairs.dtype, device=x_pairs.device)
            partial, rows = _stats_partial(True, K, x_pairs.device, L.cn_stem_fwd_rows, N_, P_)
            PROFILER.run(_last_kernel(), 1, 2.0 * N_ * P_ * Q_ * K * 8 * R * S2,
                         x_pairs.numel() * 2 + y.numel() * 2 + wp.numel() * 2 + partial.numel() * 4,
                         lambda: L.cn_stem_fwd(ptr(x_pairs), ptr(wp), ptr(y), N_, Hp_, Jp_, dtype_code(x_pairs.dtype),
                                               ptr(partial), rows, stream_of(x_pairs)),
                         x_pairs.device, detail=_conv_detail('fwd', 8, Hp_, K, R, (2, 1)))
            _park_stats(y, partial, rows)
        else:
            y = conv2d_fwd(x_pairs, wp, None, K, R, S2, (mod.stride[0], 1), (0, 0), bn_stats=want_stats,
                           pivot=stats_pivot(mod))
        ctx.mod = mod
        ctx.save_for_backward(x_pairs)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        dy = dy.contiguous()
        K, (R, S) = mod.out_channels, mod.kernel_size
        S2 = (S + 1) // 2
        L = _L()

        def run(tag):
            tmp = torch.empty(K * R * S2 * 8, dtype=torch.float32, device=x.device)
            N_, Hp_, Jp_, _ = x.shape
            code = dtype_code(x.dtype)
            if STEM_HALO and mod.stride[0] == 2 and x.dtype == torch.bfloat16 and L.cn_stem_wgrad_ok(K, R, S2, Jp_, code):
                need = L.cn_stem_wgrad_workspace(N_, Hp_)
                ws = workspace(need, x.device, tag)

                def call():
                    L.cn_stem_wgrad(ptr(x), ptr(dy), ptr(tmp), N_, Hp_, Jp_, code, 0.0, 1.0, ptr(ws), ws.numel() * 4,
                                    stream_of(x))
                _wgrad_two_phase(call, x.device, 2.0 * dy.numel() * 8 * R * S2, x.numel() * 2 + dy.numel() * 2 + float(need),
                                 float(need) + tmp.numel() * 4, _conv_detail('wgrad', 8, Hp_, K, R, (2, 1)))
            else:
                conv2d_wgrad(x, dy, tmp, 8, K, R, S2, (mod.stride[0], 1), (0, 0), beta=0.0, tag=tag)
            L.cn_wgrad_unpack_pairs(ptr(tmp), ptr(mod.grad_view('weight')), K, R, S, mod.in_channels, 1.0,
                                    stream_of(x))
            return (tmp,)

        _submit_wgrad(mod, run, (x, dy), dy)
        return None, None, None


def _lazy_dy_ok(bn_mod, y):
    """This junction BatchNorm's backward apply can be left to the convolution that produced its input."""
    conv = getattr(bn_mod, 'producer_conv', None)
    if not LAZY_DY or conv is None:
        return False
    if getattr(conv, 'junction_conv1', False):
        return False    # conv1 of a block: its data gradient is the junction kernel (addend + reduction), not a lazy consumer
    if getattr(conv, 'kernel_size', None) != (1, 1) or getattr(conv, 'bias', None) is not None:
        return False
    if y.shape[-1] > 512 or y.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        return False
    return y.numel() * _esize(y) >= LAZY_DY_MIN_MB * 2 ** 20


def _running_ptrs(mod):
    """Pointers to (running_mean, running_var, num_batches_tracked) for the kernels that update them; NULLs for a
    BatchNorm that tracks no running statistics."""
    if not mod.track_running_stats:
        return None, None, None
    return ptr(mod.running_mean), ptr(mod.running_var), ptr(mod.num_batches_tracked)


class BatchNormActFunction(Function):
    """z = act(BN(y) + residual), training mode (batch statistics)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, mod, relu, defer_apply=False, res_bn=None):
        N, H, W, C = y.shape
        M = N * H * W
        L = _L()
        code = dtype_code(y.dtype)
        ws = workspace(L.cn_bn_workspace(M, C, code), y.device)
        # defer_apply (a projection shortcut's BatchNorm, DUAL_BN): statistics only, the junction applies them; the
        # "output" handed to autograd is the input itself (the junction reads it through this BatchNorm's stats)
        defer = bool(defer_apply) and residual is None and not relu and _sync_group(mod) is None
        # res_bn: `residual` is that BatchNorm's deferred input
        dual = None
        if res_bn is not None:
            d = _take(res_bn, '_deferred', residual)
            if d is not None and residual is not None and _sync_group(mod) is None \
                    and tuple(residual.shape) == tuple(y.shape) and residual.dtype == y.dtype:
                dual = d.stats
            elif d is not None:
                raise _lib.ConvNetHipError(_MISMATCH['_deferred'])
        z = None if defer else torch.empty_like(y)
        # lazy z: the junction is finalised here and applied by the 1x1 convolution that consumes it (LAZY_Z)
        cons = getattr(mod, 'consumer_conv', None)
        lazyz = (LAZY_Z and LAZY_Z_SCOPE[0] > 0 and not defer and relu and residual is not None and C <= 512
                 and _sync_group(mod) is None and y.numel() * _esize(y) >= LAZY_Z_MIN_MB * 2 ** 20
                 and tuple(residual.shape) == tuple(y.shape) and residual.dtype == y.dtype and lazy_z_consumer_ok(cons)
                 and cons.in_channels == C)
        icons = getattr(mod, 'inner_consumer_conv', None)
        lazya = (LAZY_A and LAZY_Z_SCOPE[0] > 0 and not defer and relu and residual is None and _sync_group(mod) is None
                 and mod.training and lazy_a_consumer_ok(icons, y))
        zk = None if (defer or dual is not None or lazyz or lazya) else z     # what the statistics call applies itself
        stats = torch.empty(4 * C, dtype=torch.float32, device=y.device)
        mask = None
        if relu and residual is not None:   # 1 bit per output instead of re-reading z in backward
            mask = torch.empty(M * (C // _lib.chunk_elems(y.dtype)), dtype=torch.uint8, device=y.device)
        momentum = mod.effective_momentum()
        track = mod.track_running_stats
        nb = y.numel() * _esize(y)
        ps = take_pending_stats(y)
        if ps is not None and ps.pivot is not None and not (track and ps.pivot == mod.running_mean.data_ptr()):
            ps = None     # sums centred on something that is not this BatchNorm's running mean: take the statistics pass
        COUNTERS['bn_fwd_fused' if ps is not None else 'bn_fwd_plain'] += 1
        sync = _sync_group(mod)
        ctx.sync = sync
        if sync is not None:
            # nn.SyncBatchNorm semantics (main.py:190-191): statistics over the batch of every rank.  Each
            # rank reduces its rows to 2*C doubles, one small all-reduce, then normalise with global stats.
            # Equal per-rank batch sizes (DistributedSampler pads to that) give the global row count.
            group, world = sync
            sums = torch.empty(2 * C, dtype=torch.float64, device=y.device)
            L.cn_bn_local_sums(ptr(y), M, C, code, ptr(ps.partial) if ps is not None else None,
                               ps.rows if ps is not None else 0, ptr(sums), ptr(ws), ws.numel() * 4,
                               stream_of(y))
            _sync_all_reduce(sums, group, world)
            L.cn_bn_fwd_train_sums(ptr(y), ptr(residual), ptr(z), ptr(mask), ptr(gamma), ptr(beta),
                                   *_running_ptrs(mod), momentum, mod.eps, ptr(stats), M, C, int(relu), code, ptr(sums),
                                   M * world, stream_of(y))
        elif ps is not None:   # statistics came out of the producing convolution's epilogue: no pass over y
            PROFILER.run('bn_finalize+bn_apply (stats from conv epilogue)' if zk is not None
                         else 'bn_finalize (stats from conv epilogue; applied by the junction)',
                         (2 if ps.rows <= 512 else 3) - (0 if zk is not None else 1), 0.0,
                         (nb * (3 if residual is not None else 2) + (mask.numel() if mask is not None else 0)
                          if zk is not None else 0) + ps.partial.numel() * 4,
                         lambda: (L.cn_bn_fwd_train_partials if ps.pivot is None else L.cn_bn_fwd_train_partials_centered)(
                             ptr(y), ptr(residual) if zk is not None else None, ptr(zk), ptr(mask) if zk is not None else None,
                             ptr(gamma), ptr(beta), *_running_ptrs(mod), momentum, mod.eps, ptr(stats), M, C, int(relu), code,
                             ptr(ps.partial), ps.rows, ptr(ws), ws.numel() * 4, stream_of(y)),
                         y.device)
        elif getattr(mod, 'batch_pivot', False) and y.dtype == torch.float32:
            # statistics centred on an estimate of the batch mean (nn.BatchNorm2d.batch_pivot).  fp32 storage only: behind
            # the 2^-9 rounding of a 16-bit y the 1e-5 this buys cannot be seen, and the extra launch can
            pivot = torch.empty(C, dtype=torch.float32, device=y.device)
            PROFILER.run('bn_pivot+bn_stats+bn_finalize+bn_apply' if zk is not None else 'bn_pivot+bn_stats+bn_finalize',
                         4 if zk is not None else 3, 0.0,
                         nb * (4 if residual is not None else 3) + (mask.numel() if mask is not None else 0)
                         if zk is not None else nb,
                         lambda: L.cn_bn_fwd_train_pivot(
                             ptr(y), ptr(residual) if zk is not None else None, ptr(zk), ptr(mask) if zk is not None else None,
                             ptr(gamma), ptr(beta), *_running_ptrs(mod), momentum, mod.eps, ptr(stats), ptr(pivot), M, C,
                             int(relu), code, ptr(ws), ws.numel() * 4, stream_of(y)),
                         y.device)
        else:
            PROFILER.run('bn_stats+bn_finalize+bn_apply' if zk is not None else 'bn_stats+bn_finalize', 3 if zk is not None else 2, 0.0,
                         nb * (4 if residual is not None else 3) + (mask.numel() if mask is not None else 0)
                         if zk is not None else nb,
                         lambda: L.cn_bn_fwd_train(
                             ptr(y), ptr(residual) if zk is not None else None, ptr(zk), ptr(mask) if zk is not None else None,
                             ptr(gamma), ptr(beta), *_running_ptrs(mod), momentum, mod.eps, ptr(stats), M, C, int(relu), code,
                             ptr(ws), ws.numel() * 4, stream_of(y)),
                         y.device)
        if lazyz:
            _park(cons, '_lazy_z', z, LazyZ(y, residual.contiguous(), stats, dual, z, mask, relu))
        elif lazya:
            _park(icons, '_lazy_a', z, LazyA(y, stats, z, relu))
        elif dual is not None:    # both BatchNorms finalised: one apply pass reads y and the shortcut's raw input
            PROFILER.run('bn_apply (junction + projection-shortcut BatchNorm)', 1, 0.0,
                         nb * 3 + (mask.numel() if mask is not None else 0),
                         lambda: L.cn_bn_apply_dual(ptr(y), ptr(residual), ptr(z), ptr(mask), ptr(stats), ptr(dual),
                                                    M, C, int(relu), code, stream_of(y)),
                         y.device)
            COUNTERS['bn_fwd_dual'] = COUNTERS.get('bn_fwd_dual', 0) + 1
        ctx.mod = mod
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.out_ptr = z.data_ptr() if z is not None else None
        mod._fwd_ctx = weakref.ref(ctx)      # lets the consumer conv's dgrad fuse this BN's backward reduction
        if mask is not None:
            ctx.save_for_backward(y, stats, mask)
        else:
            ctx.save_for_backward(y, stats)
        if defer:
            _park(mod, '_deferred', y, DeferredBN(stats))
            return y     # (autograd hands back an alias of the input: same storage, this node as its grad_fn)
        return z

    @staticmethod
    def backward(ctx, dz):
        saved = ctx.saved_tensors
        y, stats = saved[0], saved[1]
        zmask = saved[2] if len(saved) > 2 else None
        mod = ctx.mod
        N, H, W, C = y.shape
        M = N * H * W
        L = _L()
        code = dtype_code(y.dtype)
        dz = dz.contiguous()
        ws = workspace(L.cn_bn_workspace(M, C, code), y.device)
        dy = torch.empty_like(y)
        want_res = ctx.has_res and ctx.needs_input_grad[3]
        coef = torch.empty(3 * C, dtype=torch.float32, device=y.device)
        nb = y.numel() * _esize(y)
        pp = _take(mod, '_bwd_partials', dz, strict=False)   # (another tensor's entry: not fused, the plain passes run)
        fused_in = pp is not None and dz.dtype == y.dtype
        if ctx.sync is not None:
            group, world = ctx.sync
            COUNTERS['bn_bwd_fused' if fused_in else 'bn_bwd_plain'] += 1
            local = torch.empty(2 * C, dtype=torch.float64, device=y.device)
            L.cn_bn_bwd_local_sums(ptr(dz), ptr(y), ptr(zmask), ptr(stats), M, C, int(ctx.relu), code,
                                   ptr(pp.partial) if fused_in else None, pp.rows if fused_in else 0, ptr(local),
                                   ptr(ws), ws.numel() * 4, stream_of(y))
            glob = local.clone()
            _sync_all_reduce(glob, group, world)
            if fused_in:
                dres = dz if want_res else None
            else:
                dres = torch.empty_like(y) if want_res else None
            L.cn_bn_bwd_sums(ptr(dz), ptr(y), ptr(zmask), ptr(mod.weight), ptr(stats), ptr(dy),
                             None if fused_in else ptr(dres), ptr(mod.grad_view('weight')),
                             ptr(mod.grad_view('bias')), 1.0, 1.0, ptr(coef), M, C, int(ctx.relu),
                             int(fused_in), code, ptr(local), ptr(glob), M * world, stream_of(y))
        elif fused_in and _lazy_dy_ok(mod, y):
            # ... and the apply pass is left to the consumers: finalize only, dy = c1*g + c2*y + c3 is formed on the
            # operand loads of the producing convolution's dgrad / wgrad (see LAZY_DY)
            partial, rows = pp
            COUNTERS['bn_bwd_fused'] += 1
            COUNTERS['bn_bwd_lazy'] = COUNTERS.get('bn_bwd_lazy', 0) + 1
            dres = dz if want_res else None
            with SIDE.mark(coef):
                PROFILER.run('bn_bwd_finalize (lazy dy)', 1 if rows <= 512 else 2, 0.0, partial.numel() * 4,
                             lambda: L.cn_bn_bwd_partials(ptr(dz), ptr(y), ptr(mod.weight), ptr(stats), None,
                                                          ptr(mod.grad_view('weight')), ptr(mod.grad_view('bias')),
                                                          1.0, 1.0, ptr(coef), M, C, code, ptr(partial), rows,
                                                          ptr(ws), ws.numel() * 4, stream_of(y)),
                             y.device)
            _park(mod.producer_conv, '_lazy_dy', y, LazyDy(dz, y, coef))
            dy = _zero_like_placeholder(y)
        elif fused_in:
            # dz arrived masked (g) with its reduction partials from the producing dgrad's epilogue
            partial, rows = pp
            COUNTERS['bn_bwd_fused'] += 1
            dres = dz if want_res else None       # the residual branch's gradient is g itself
            with SIDE.mark(dy):
                PROFILER.run('bn_bwd_finalize+bn_bwd_apply (reduce in dgrad epilogue)', 2 if rows <= 512 else 3, 0.0,
                             nb * 3 + partial.numel() * 4,
                             lambda: L.cn_bn_bwd_partials(ptr(dz), ptr(y), ptr(mod.weight), ptr(stats), ptr(dy),
                                                          ptr(mod.grad_view('weight')), ptr(mod.grad_view('bias')),
                                                          1.0, 1.0, ptr(coef), M, C, code, ptr(partial), rows,
                                                          ptr(ws), ws.numel() * 4, stream_of(y)),
                             y.device)
        elif not ctx.relu and not want_res and zmask is None and _lazy_dy_ok(mod, y):
            # a BatchNorm with no activation behind it (the projection shortcut's): reduce + finalize, apply left to the
            # producing convolution's dgrad / wgrad (dz needs no mask)
            COUNTERS['bn_bwd_plain'] += 1
            COUNTERS['bn_bwd_lazy'] = COUNTERS.get('bn_bwd_lazy', 0) + 1
            dres = None
            with SIDE.mark(coef):
                PROFILER.run('bn_bwd_reduce+bn_bwd_finalize (lazy dy)', 2, 0.0, nb * 2,
                             lambda: L.cn_bn_bwd(ptr(dz), ptr(y), None, ptr(mod.weight), ptr(stats), None,
                                                 None, ptr(mod.grad_view('weight')), ptr(mod.grad_view('bias')),
                                                 1.0, 1.0, ptr(coef), M, C, 0, code, ptr(ws),
                                                 ws.numel() * 4, stream_of(y)),
                             y.device)
            _park(mod.producer_conv, '_lazy_dy', y, LazyDy(dz, y, coef))
            dy = _zero_like_placeholder(y)
        else:
            COUNTERS['bn_bwd_plain'] += 1
            dres = torch.empty_like(y) if want_res else None
            with SIDE.mark(dy):
                PROFILER.run('bn_bwd_reduce+bn_bwd_finalize+bn_bwd_apply', 3, 0.0,
                             nb * (5 + (1 if dres is not None else 0)) + (2 * zmask.numel() if zmask is not None else 0),
                             lambda: L.cn_bn_bwd(ptr(dz), ptr(y), ptr(zmask), ptr(mod.weight), ptr(stats), ptr(dy),
                                                 ptr(dres), ptr(mod.grad_view('weight')), ptr(mod.grad_view('bias')),
                                                 1.0, 1.0, ptr(coef), M, C, int(ctx.relu), code, ptr(ws),
                                                 ws.numel() * 4, stream_of(y)),
                             y.device)
        mod._notify_grad_ready()
        holder = getattr(mod, '_res_holder', None)
        if holder is not None:
            holder.park(dres)
        return dy, None, None, dres, None, None, None, None


def batch_norm_infer(y, residual, mod, relu):
    take_pending_stats(y)     # eval mode: the partials (if any) are not needed
    N, H, W, C = y.shape
    z = torch.empty_like(y)
    coeffs = torch.empty(2 * C, dtype=torch.float32, device=y.device)
    _L().cn_bn_fwd_infer(ptr(y), ptr(residual), ptr(z), ptr(mod.weight), ptr(mod.bias),
                         ptr(mod.running_mean), ptr(mod.running_var), mod.eps, ptr(coeffs), N * H * W, C,
                         int(relu), dtype_code(y.dtype), stream_of(y))
    return z


class L1BatchNormActFunction(Function):
    """z = act(L1BN(y) + residual), training mode (nn.L1BatchNorm2d on csrc/l1bn.hip).  Always the standalone passes: the
    forward reads y three times (mean, mean absolute deviation, apply), the backward is reduce + finalize + apply."""

    @staticmethod
    def forward(ctx, y, gamma, beta, residual, mod, relu):
        take_pending_stats(y)     # (sum / sum-of-squares partials of a producer are of no use to this norm)
        y = y.contiguous()
        N, H, W, C = y.shape
        M = N * H * W
        L = _L()
        code = dtype_code(y.dtype)
        if residual is not None:
            if tuple(residual.shape) != tuple(y.shape) or residual.dtype != y.dtype:
                raise _lib.ConvNetHipError('L1BatchNorm2d: residual %s %s does not match the input %s %s'
                                           % (tuple(residual.shape), residual.dtype, tuple(y.shape), y.dtype))
            residual = residual.contiguous()
        ws = workspace(L.cn_l1bn_workspace(M, C, code), y.device)
        z = torch.empty_like(y)
        stats = torch.empty(7 * C, dtype=torch.float32, device=y.device)
        mask = None
        if relu and residual is not None:   # 1 bit per output instead of re-reading z in backward
            mask = torch.empty(M * (C // _lib.chunk_elems(y.dtype)), dtype=torch.uint8, device=y.device)
        nb = y.numel() * _esize(y)
        COUNTERS['l1bn_fwd'] = COUNTERS.get('l1bn_fwd', 0) + 1
        PROFILER.run('l1bn_sum+l1bn_mean+l1bn_absdev+l1bn_finalize+l1bn_apply', 5, 0.0,
                     nb * (5 if residual is not None else 4) + (mask.numel() if mask is not None else 0),
                     lambda: L.cn_l1bn_fwd_train(ptr(y), ptr(residual), ptr(z), ptr(mask), ptr(gamma), ptr(beta),
                                                 ptr(mod.running_mean), ptr(mod.running_var), float(mod.momentum),
                                                 mod.eps, ptr(stats), M, C, int(relu), code, ptr(ws), ws.numel() * 4,
                                                 stream_of(y)),
                     y.device)
        ctx.mod = mod
        ctx.relu = relu
        ctx.has_res = residual is not None
        if mask is not None:
            ctx.save_for_backward(y, stats, mask)
        else:
            ctx.save_for_backward(y, stats)
        return z

    @staticmethod
    def backward(ctx, dz):
        saved = ctx.saved_tensors
        y, stats = saved[0], saved[1]
        zmask = saved[2] if len(saved) > 2 else None
        mod = ctx.mod
        N, H, W, C = y.shape
        M = N * H * W
        L = _L()
        code = dtype_code(y.dtype)
        dz = dz.contiguous()
        ws = workspace(L.cn_l1bn_workspace(M, C, code), y.device)
        dy = torch.empty_like(y)
        dres = torch.empty_like(y) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        coef = torch.empty(3 * C, dtype=torch.float32, device=y.device)
        nb = y.numel() * _esize(y)
        COUNTERS['l1bn_bwd'] = COUNTERS.get('l1bn_bwd', 0) + 1
        with SIDE.mark(dy):
            PROFILER.run('l1bn_bwd_reduce+l1bn_bwd_finalize+l1bn_bwd_apply', 3, 0.0,
                         nb * (5 + (1 if dres is not None else 0)) + (2 * zmask.numel() if zmask is not None else 0),
                         lambda: L.cn_l1bn_bwd(ptr(dz), ptr(y), ptr(zmask), ptr(mod.weight), ptr(stats), ptr(dy),
                                               ptr(dres), ptr(mod.grad_view('weight')), ptr(mod.grad_view('bias')),
                                               1.0, 1.0, ptr(coef), M, C, int(ctx.relu), code, ptr(ws),
                                               ws.numel() * 4, stream_of(y)),
                         y.device)
        mod._notify_grad_ready()
        return dy, None, None, dres, None, None


def l1_batch_norm_infer(y, residual, mod, relu):
    take_pending_stats(y)
    y = y.contiguous()
    N, H, W, C = y.shape
    z = torch.empty_like(y)
    coeffs = torch.empty(3 * C, dtype=torch.float32, device=y.device)
    _L().cn_l1bn_fwd_infer(ptr(y), ptr(residual.contiguous() if residual is not None else None), ptr(z), ptr(mod.weight),
                           ptr(mod.bias), ptr(mod.running_mean), ptr(mod.running_var), ptr(coeffs), N * H * W, C,
                           int(relu), dtype_code(y.dtype), stream_of(y))
    return z


def _se_shape(r, mod):
    N, H, W, C = r.shape
    Cr = mod.hidden_channels
    if C != mod.in_channels or C % _lib.chunk_elems(r.dtype) != 0:
        raise _lib.ConvNetHipError('SEBlock(%d) got an NHWC input %s in %s: the channels must match and be a multiple of the '
                                   'dtype\'s chunk' % (mod.in_channels, tuple(r.shape), r.dtype))
    return N, H * W, C, Cr


def _se_gate(r, mod, N, HW, C, Cr):
    """squeeze + excite of nn.SEBlock: (s, h, m), all fp32.  The squeeze is csrc/se.hip's own reduction: cn_avgpool_fwd
    rounds its means to the compute dtype."""
    L = _L()
    code = dtype_code(r.dtype)
    ws = workspace(L.cn_se_workspace(N, HW, C, Cr, code), r.device)
    s = torch.empty((N, C), dtype=torch.float32, device=r.device)
    h = torch.empty((N, Cr), dtype=torch.float32, device=r.device)
    m = torch.empty((N, C), dtype=torch.float32, device=r.device)
    lin1, lin2 = mod.transform[0], mod.transform[2]
    PROFILER.run('se_squeeze', 2, 0.0, r.numel() * _esize(r),
                 lambda: L.cn_se_squeeze(ptr(r), ptr(s), N, HW, C, code, ptr(ws), ws.numel() * 4, stream_of(r)), r.device)
    PROFILER.run('se_excite_fwd', 1, 4.0 * N * C * Cr, 8.0 * N * C * Cr,
                 lambda: L.cn_se_excite_fwd(ptr(s), ptr(lin1.master_view('weight')), ptr(lin1.master_view('bias')),
                                            ptr(lin2.master_view('weight')), ptr(lin2.master_view('bias')), ptr(h), ptr(m),
                                            N, C, Cr, stream_of(r)), r.device)
    return s, h, m


class SEScaleFunction(Function):
    """rs = r * m, m = sigmoid(W2 relu(W1 mean_hw(r) + b1) + b2) per sample and channel (nn.SEBlock on csrc/se.hip).
    forward: squeeze -> excite -> scale; backward: reduce (dm = sum_hw g*r) -> excite backward (ds and the four parameter
    gradients, accumulated into the arena: a module shared by the blocks of a stage receives their sum) -> apply
    (dr = g*m + ds/HW).  No host synchronisation, grow-only workspace: capturable."""

    @staticmethod
    def forward(ctx, r, w1, b1, w2, b2, mod):
        r = r.contiguous()
        N, HW, C, Cr = _se_shape(r, mod)
        s, h, m = _se_gate(r, mod, N, HW, C, Cr)
        rs = torch.empty_like(r)
        nb = r.numel() * _esize(r)
        PROFILER.run('se_scale_fwd', 1, 0.0, 2 * nb,
                     lambda: _L().cn_se_scale_fwd(ptr(r), ptr(m), ptr(rs), N, HW, C, dtype_code(r.dtype), stream_of(r)),
                     r.device)
        COUNTERS['se_fwd'] = COUNTERS.get('se_fwd', 0) + 1
        ctx.mod = mod
        ctx.save_for_backward(r, s, h, m)
        mod._pending_bwd += 1
        return rs

    @staticmethod
    def backward(ctx, g):
        r, s, h, m = ctx.saved_tensors
        mod = ctx.mod
        N, HW, C, Cr = _se_shape(r, mod)
        L = _L()
        code = dtype_code(r.dtype)
        g = g.contiguous()
        ws = workspace(L.cn_se_workspace(N, HW, C, Cr, code), r.device)
        lin1, lin2 = mod.transform[0], mod.transform[2]
        dm = torch.empty((N, C), dtype=torch.float32, device=r.device)
        ds = torch.empty((N, C), dtype=torch.float32, device=r.device)
        nb = r.numel() * _esize(r)
        COUNTERS['se_bwd'] = COUNTERS.get('se_bwd', 0) + 1
        PROFILER.run('se_scale_bwd_reduce', 2, 0.0, 2 * nb,
                     lambda: L.cn_se_scale_bwd_reduce(ptr(g), ptr(r), ptr(dm), N, HW, C, code, ptr(ws), ws.numel() * 4,
                                                      stream_of(r)), r.device)
        PROFILER.run('se_excite_bwd', 2, 8.0 * N * C * Cr, 16.0 * N * C * Cr,
                     lambda: L.cn_se_excite_bwd(ptr(dm), ptr(s), ptr(h), ptr(m), ptr(lin1.master_view('weight')),
                                                ptr(lin2.master_view('weight')), ptr(ds), ptr(lin1.grad_view('weight')),
                                                ptr(lin1.grad_view('bias')), ptr(lin2.grad_view('weight')),
                                                ptr(lin2.grad_view('bias')), 1.0, 1.0, N, C, Cr, ptr(ws), ws.numel() * 4,
                                                stream_of(r)), r.device)
        dr = None
        if ctx.needs_input_grad[0]:
            dr = torch.empty_like(r)
            PROFILER.run('se_scale_bwd_apply', 1, 0.0, 2 * nb,
                         lambda: L.cn_se_scale_bwd_apply(ptr(g), ptr(m), ptr(ds), None, ptr(dr), N, HW, C, code,
                                                         stream_of(r)), r.device)
        mod._pending_bwd -= 1
        if mod._pending_bwd <= 0:    # the last of the blocks that share this module: its gradients are complete
            mod._pending_bwd = 0
            lin1._notify_grad_ready()
            lin2._notify_grad_ready()
        return dr, None, None, None, None, None


def se_scale_infer(r, mod):
    r = r.contiguous()
    N, HW, C, Cr = _se_shape(r, mod)
    _, _, m = _se_gate(r, mod, N, HW, C, Cr)
    rs = torch.empty_like(r)
    _L().cn_se_scale_fwd(ptr(r), ptr(m), ptr(rs), N, HW, C, dtype_code(r.dtype), stream_of(r))
    return rs


class MaxPool2dFunction(Function):
    @staticmethod
    def forward(ctx, x, k, stride, pad):
        N, H, W, C = x.shape
        P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = torch.empty((N, P, Q, C), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, P, Q, C), dtype=torch.uint8, device=x.device)
        PROFILER.run('maxpool_fwd', 1, 0.0, x.numel() * _esize(x) + y.numel() * (_esize(y) + 1),
                     lambda: _L().cn_maxpool_fwd(ptr(x), ptr(y), ptr(idx), N, H, W, C, k, stride, pad,
                                                 dtype_code(x.dtype), stream_of(x)),
                     x.device)
        ctx.cfg = (N, H, W, C, k, stride, pad)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, H, W, C, k, stride, pad = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
        PROFILER.run('maxpool_bwd', 1, 0.0, dx.numel() * _esize(dx) + dy.numel() * (_esize(dy) + 1),
                     lambda: _L().cn_maxpool_bwd(ptr(dy), ptr(idx), ptr(dx), N, H, W, C, k, stride, pad,
                                                 dtype_code(dy.dtype), stream_of(dy)),
                     dy.device)
        return dx, None, None, None


class BnReluMaxPoolFunction(Function):
    """maxpool(relu(BN(y))) of the stem (models/resnet.py:228-230) without the normalised 112x112 map:
    forward = BatchNorm statistics / coefficients (from the conv epilogue partials when present) +
    one pooling pass over the pre-BN tensor; backward = cn_bn_bwd_maxpool (the pool's gather backward
    folded into both BatchNorm-backward passes).  Bit-identical to the unfused chain."""

    @staticmethod
    def forward(ctx, y, gamma, beta, mod, k, stride, pad):
        N, H, W, C = y.shape
        M = N * H * W
        L = _L()
        code = dtype_code(y.dtype)
        ws = workspace(L.cn_bn_workspace(M, C, code), y.device)
        stats = torch.empty(4 * C, dtype=torch.float32, device=y.device)
        momentum = mod.effective_momentum()
        track = mod.track_running_stats
        rm, rv, nbt = _running_ptrs(mod)
        ps = take_pending_stats(y)
        if ps is not None and ps.pivot is not None and not (track and ps.pivot == mod.running_mean.data_ptr()):
            ps = None
        COUNTERS['bn_fwd_fused' if ps is not None else 'bn_fwd_plain'] += 1
        P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        out = torch.empty((N, P, Q, C), dtype=y.dtype, device=y.device)
        idx = torch.empty((N, P, Q, C), dtype=torch.uint8, device=y.device)
        # the pre-BatchNorm value of every winning tap: the backward sums then run over the pooled map
        xmax = torch.empty_like(out) if (STEM_XMAX and ctx.needs_input_grad[0]) else None

        def run():
            if ps is not None:
                fn = L.cn_bn_fwd_train_partials if ps.pivot is None else L.cn_bn_fwd_train_partials_centered
                fn(ptr(y), None, None, None, ptr(gamma), ptr(beta), rm, rv, nbt, momentum, mod.eps, ptr(stats), M, C, 1, code,
                   ptr(ps.partial), ps.rows, ptr(ws), ws.numel() * 4, stream_of(y))
            else:
                L.cn_bn_fwd_train(ptr(y), None, None, None, ptr(gamma), ptr(beta), rm, rv, nbt, momentum, mod.eps,
                                  ptr(stats), M, C, 1, code, ptr(ws), ws.numel() * 4, stream_of(y))
            if xmax is not None:
                L.cn_maxpool_fwd_bnrelu_xmax(ptr(y), ptr(stats[2 * C:3 * C]), ptr(stats[3 * C:]), ptr(out), ptr(idx),
                                             ptr(xmax), N, H, W, C, k, stride, pad, code, stream_of(y))
            else:
                L.cn_maxpool_fwd_bnrelu(ptr(y), ptr(stats[2 * C:3 * C]), ptr(stats[3 * C:]), ptr(out), ptr(idx), N, H,
                                        W, C, k, stride, pad, code, stream_of(y))
        PROFILER.run('bn_finalize+maxpool_fwd_bnrelu (stem)', 3, 0.0,
                     y.numel() * _esize(y) * (1 if ps is not None else 2)
                     + out.numel() * (_esize(out) * (2 if xmax is not None else 1) + 1), run, y.device)
        ctx.mod = mod
        ctx.cfg = (N, H, W, C, k, stride, pad)
        ctx.has_xmax = xmax is not None
        if xmax is not None:
            ctx.save_for_backward(y, stats, idx, xmax)
        else:
            ctx.save_for_backward(y, stats, idx)
        return out

    @staticmethod
    def backward(ctx, dpool):
        y, stats, idx = ctx.saved_tensors[:3]
        xmax = ctx.saved_tensors[3] if ctx.has_xmax else None
        mod = ctx.mod
        N, H, W, C, k, stride, pad = ctx.cfg
        L = _L()
        code = dtype_code(y.dtype)
        dpool = dpool.contiguous()
        ws = workspace(L.cn_bn_workspace(N * H * W, C, code), y.device)
        dy = torch.empty_like(y)
        coef = torch.empty(3 * C, dtype=torch.float32, device=y.device)
        COUNTERS['bn_bwd_plain'] += 1
        with SIDE.mark(dy):
            PROFILER.run('bn_bwd_maxpool (stem)', 3, 0.0,
                         (y.numel() * _esize(y) * 3 + dpool.numel() * (_esize(dpool) + 1) * 2) if xmax is None else
                         (y.numel() * _esize(y) * 2 + dpool.numel() * (3 * _esize(dpool) + 1)),
                         (lambda: L.cn_bn_bwd_maxpool(ptr(dpool), ptr(idx), ptr(y), ptr(mod.weight), ptr(stats), ptr(dy),
                                                      ptr(mod.grad_view('weight')), ptr(mod.grad_view('bias')), 1.0, 1.0,
                                                      ptr(coef), N, H, W, C, k, stride, pad, code, ptr(ws),
                                                      ws.numel() * 4, stream_of(y)))
                         if xmax is None else
                         (lambda: L.cn_bn_bwd_maxpool_xmax(ptr(dpool), ptr(idx), ptr(y), ptr(xmax), ptr(mod.weight),
                                                           ptr(stats), ptr(dy), ptr(mod.grad_view('weight')),
                                                           ptr(mod.grad_view('bias')), 1.0, 1.0, ptr(coef), N, H, W, C,
                                                           k, stride, pad, code, ptr(ws), ws.numel() * 4,
                                                           stream_of(y))),
                         y.device)
        mod._notify_grad_ready()
        return dy, None, None, None, None, None, None


class GlobalAvgPoolFunction(Function):
    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        y = torch.empty((N, 1, 1, C), dtype=x.dtype, device=x.device)
        _L().cn_avgpool_fwd(ptr(x), ptr(y), N, H * W, C, dtype_code(x.dtype), stream_of(x))
        ctx.shape = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
        _L().cn_avgpool_bwd(ptr(dy), ptr(dx), N, H * W, C, dtype_code(dy.dtype), stream_of(dy))
        return dx


class ReLUFunction(Function):
    @staticmethod
    def forward(ctx, x):
        z = torch.empty_like(x)
        _L().cn_eltwise(1, ptr(z), ptr(x), None, x.numel(), dtype_code(x.dtype), stream_of(x))
        ctx.save_for_backward(z)
        return z

    @staticmethod
    def backward(ctx, dz):
        (z,) = ctx.saved_tensors
        dz = dz.contiguous()
        dx = torch.empty_like(dz)
        _L().cn_eltwise(2, ptr(dx), ptr(dz), ptr(z), dz.numel(), dtype_code(dz.dtype), stream_of(dz))
        return dx


class DropoutFunction(Function):
    """z = x * mask; `mask` (compute dtype, NHWC) already holds keep/(1-p)."""

    @staticmethod
    def forward(ctx, x, mask):
        z = torch.empty_like(x)
        _L().cn_eltwise(3, ptr(z), ptr(x), ptr(mask), x.numel(), dtype_code(x.dtype), stream_of(x))
        ctx.save_for_backward(mask)
        return z

    @staticmethod
    def backward(ctx, dz):
        (mask,) = ctx.saved_tensors
        dz = dz.contiguous()
        dx = torch.empty_like(dz)
        _L().cn_eltwise(3, ptr(dx), ptr(dz), ptr(mask), dz.numel(), dtype_code(dz.dtype), stream_of(dz))
        return dx, None


class SmallLinearFunction(Function):
    """Dense layer whose output width is not a multiple of the 16-byte chunk (MNIST's 10-way head)."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, mod):
        B, C = x2d.shape
        K = mod.out_channels
        y = torch.empty((B, K), dtype=torch.float32, device=x2d.device)
        _L().cn_small_linear(0, ptr(x2d), ptr(mod.master_view('weight')), ptr(bias), ptr(y), None, None, B, C,
                             K, dtype_code(x2d.dtype), stream_of(x2d))
        ctx.mod = mod
        ctx.save_for_backward(x2d)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x2d,) = ctx.saved_tensors
        mod = ctx.mod
        B, C = x2d.shape
        K = mod.out_channels
        dy = dy.contiguous().float()
        L = _L()
        code = dtype_code(x2d.dtype)
        db = mod.grad_view('bias') if mod.bias is not None else None
        L.cn_small_linear(2, ptr(x2d), None, None, ptr(dy), ptr(mod.grad_view('weight')), ptr(db), B, C, K, code,
                          stream_of(x2d))
        mod._notify_grad_ready()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2d)
            L.cn_small_linear(1, ptr(dy), ptr(mod.master_view('weight')), None, ptr(dx), None, None, B, C, K,
                              code, stream_of(x2d))
        return dx, None, None, None


class ForkFunction(Function):
    """Two aliases of one activation (block input -> conv branch + residual branch).  Backward sums
    the two incoming gradients with our own kernel, so autograd never launches its accumulate."""

    @staticmethod
    def forward(ctx, x, holder=None):
        ctx.holder = holder
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        first, sub, fused = ctx.holder.take() if ctx.holder is not None else (None, 1, False)
        if sub == 2 and not fused and first is not None:
            # a subsampled projection-shortcut gradient that no dgrad epilogue picked up (not the case in the ResNet
            # blocks: conv1 always does): scatter it into a dense tensor here (data movement only) and add
            dense = torch.zeros((first.shape[0], gb.shape[1], gb.shape[2], first.shape[3]), dtype=first.dtype,
                                device=first.device)
            dense[:, ::2, ::2, :] = first
            return (add_(ga.contiguous(), dense) if ga is not None else dense), None
        if ga is None:
            return gb, None
        if gb is None:
            return ga, None
        if fused:   # the later of the two branch gradients already contains the earlier one
            return (gb if (first is not None and first.data_ptr() == ga.data_ptr()) else ga), None
        ga = ga.contiguous()
        return add_(ga, gb.contiguous()), None


class ResGradHolder(object):
    """Per-block mailbox for the two gradients that meet at a residual block's input: whichever branch
    finishes first (the last BN's `dres` in identity blocks, one of the two convs in downsample
    blocks) parks its gradient here; the other branch's conv dgrad adds it in its epilogue (one pass
    instead of a separate add kernel), independent of autograd's execution order."""
    __slots__ = ('dres', 'fused', 'sub')   # sub = 2: dres holds only the even (h, w) pixels (stride-2 1x1 projection)

    def __init__(self):
        self.reset()

    def reset(self):
        self.dres, self.fused, self.sub = None, False, 1

    def park(self, t, sub=1):     # the first of the two gradients
        self.dres, self.sub, self.fused = t, sub, False

    def claim(self):              # (dres, sub) for the second branch's dgrad epilogue: the fork then passes that sum on
        self.fused = True
        return self.dres, self.sub

    def take(self):               # (dres, sub, fused) at the fork's backward; the holder is empty again
        out = (self.dres, self.sub, self.fused)
        self.reset()
        return out


class SoftmaxCrossEntropyFunction(Function):
    """loss = mean_b CE(logits_b, target_b) (+ label smoothing); also accumulates the reference's
    loss / prec@1 / prec@5 meters on the device (crit.meters) when a buffer is attached."""

    @staticmethod
    def forward(ctx, logits, target, crit):
        B, K = logits.shape
        logits = logits.contiguous()
        if logits.dtype != torch.float32:
            raise _lib.ConvNetHipError('criterion expects fp32 logits')
        target = target.contiguous()
        row = torch.empty(3 * B, dtype=torch.float32, device=logits.device)
        step_out = torch.empty(3, dtype=torch.float32, device=logits.device)
        _L().cn_softmax_ce(ptr(logits), ptr(target), None, _lib.F32, ptr(row), ptr(step_out),
                           ptr(crit.meters), B, K, 1.0, None, crit.smooth_eps, stream_of(logits))
        crit.last_step = step_out
        ctx.crit = crit
        ctx.save_for_backward(logits, target, row)
        return step_out[0]

    @staticmethod
    def backward(ctx, go):
        logits, target, row = ctx.saved_tensors
        B, K = logits.shape
        dlogits = torch.empty_like(logits)
        go = go.contiguous().to(torch.float32)
        _L().cn_softmax_ce(ptr(logits), ptr(target), ptr(dlogits), _lib.F32, ptr(row), None, None, B, K,
                           1.0 / B, ptr(go), ctx.crit.smooth_eps, stream_of(logits))
        return dlogits, None, None


class AverageDuplicatesFunction(Function):
    """trainer.py:32-41 _average_duplicates (batch_first): fp32 [B * D, K], the D rows of a sample consecutive -> their
    mean [B, K] (cn_avg_duplicates_fwd: ordered fp32 sum, true division); backward hands every row dmean / D."""

    @staticmethod
    def forward(ctx, logits, D):
        if logits.dim() != 2 or logits.dtype != torch.float32 or D < 1 or logits.shape[0] % D != 0:
            raise _lib.ConvNetHipError('average_duplicates expects fp32 [B * D, K] logits, got %s %s for D = %d'
                                       % (logits.dtype, tuple(logits.shape), D))
        logits = logits.contiguous()
        B, K = logits.shape[0] // D, logits.shape[1]
        mean = torch.empty((B, K), dtype=torch.float32, device=logits.device)
        PROFILER.run('avg_duplicates_fwd', 1, 0.0, (logits.numel() + mean.numel()) * 4,
                     lambda: _L().cn_avg_duplicates_fwd(ptr(logits), ptr(mean), B, D, K, stream_of(logits)), logits.device)
        ctx.D = D
        return mean

    @staticmethod
    def backward(ctx, dmean):
        return average_duplicates_bwd(dmean, ctx.D, torch.float32), None


def average_duplicates(logits, D):
    return AverageDuplicatesFunction.apply(logits, int(D))


def average_duplicates_bwd(dmean, D, grad_dtype=torch.float32):
    """dlogits[b * D + d][k] = dmean[b][k] / D in `grad_dtype` (the fp32 quotient rounded once)."""
    if dmean.dim() != 2 or D < 1:
        raise _lib.ConvNetHipError('average_duplicates_bwd expects [B, K] and D >= 1, got %s, D = %d' % (tuple(dmean.shape), D))
    dmean = dmean.contiguous().to(torch.float32)
    B, K = dmean.shape
    dlogits = torch.empty((B * D, K), dtype=grad_dtype, device=dmean.device)
    PROFILER.run('avg_duplicates_bwd', 1, 0.0, dmean.numel() * 4 + dlogits.numel() * _esize(dlogits),
                 lambda: _L().cn_avg_duplicates_bwd(ptr(dmean), ptr(dlogits), dtype_code(grad_dtype), B, D, K,
                                                    stream_of(dmean)), dmean.device)
    return dlogits


def accuracy_counts(logits, target):
    """Returns a device tensor [mean CE loss, prec@1 (%), prec@5 (%)] of this batch."""
    B, K = logits.shape
    logits = logits.contiguous().float()
    row = torch.empty(3 * B, dtype=torch.float32, device=logits.device)
    out = torch.empty(3, dtype=torch.float32, device=logits.device)
    _L().cn_softmax_ce(ptr(logits), ptr(target.contiguous()), None, _lib.F32, ptr(row), ptr(out), None, B, K,
                       1.0, None, 0.0, stream_of(logits))
    return out
