#!/usr/bin/env python
"""Optimizer kernels (csrc/optim.hip) over a ResNet-50-sized flat arena (25.6 M fp32 parameters): cn_sgd_momentum beside
cn_sgd_nesterov, cn_adam (Adam, AdamW), cn_rmsprop (with and without momentum) and the one-thread cn_optim_advance, in one
process on the same buffers, alternated, HIP events after a warm-up repeat.

Two timings per kernel.  warm: --iters calls back to back on the same buffers - the Infinity Cache (256 MB) then holds a
part of the working set, a larger part of SGD's three buffers (307 MB) than of Adam's four (410 MB), and the rates come out
above what HBM delivers.  cold: every timed call follows 1 GiB of unrelated writes, which is how the optimizer meets its
buffers at the end of a training step.

Printed per kernel and timing: median ms per call, min-max spread over the repeats, the achieved bytes/s of the nominal
traffic (4 B per buffer read or written per parameter: SGD 20 B, Adam 28 B, ...) and that rate relative to cn_sgd_momentum's."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convnet_amd as ca  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numel', type=int, default=25_610_000, help='arena length in floats (ResNet-50: 25.6 M)')
    ap.add_argument('--iters', type=int, default=10, help='calls per timed repeat')
    ap.add_argument('--repeats', type=int, default=7)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib = ca._lib
    L = lib.load()
    ptr = lib.ptr
    n = args.numel // 64 * 64
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 0.01
    b1, b2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    hyper = torch.tensor([1e-3, 0.9, 0.0, 0.0], device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    clip = torch.ones(1, device=dev)
    corr = hyper[2:]
    s = lib.stream_of(p)
    L.cn_optim_advance(ptr(step), ptr(corr), 0.1, 0.001, s)
    calls = [
        ('sgd_momentum', 20, lambda: L.cn_sgd_momentum(ptr(p), ptr(g), ptr(b1), n, 0.0, 0.0, 1e-4, 1.0, ptr(clip), ptr(hyper), s)),
        ('sgd_nesterov', 20, lambda: L.cn_sgd_nesterov(ptr(p), ptr(g), ptr(b1), n, 0.0, 0.0, 1e-4, 1.0, ptr(clip), ptr(hyper), s)),
        ('adam', 28, lambda: L.cn_adam(ptr(p), ptr(g), ptr(b1), ptr(b2), n, 0.0, 0.1, 0.999, 0.001, 1e-8, 1e-4, 0.0, 1.0,
                                       ptr(clip), ptr(hyper), ptr(corr), s)),
        ('adamw', 28, lambda: L.cn_adam(ptr(p), ptr(g), ptr(b1), ptr(b2), n, 0.0, 0.1, 0.999, 0.001, 1e-8, 1e-4, 1e-2, 1.0,
                                        ptr(clip), ptr(hyper), ptr(corr), s)),
        ('rmsprop', 20, lambda: L.cn_rmsprop(ptr(p), ptr(g), ptr(b2), None, n, 0.0, 0.0, 0.99, 0.01, 1e-8, 1e-4, 1.0,
                                             ptr(clip), ptr(hyper), s)),
        ('rmsprop+momentum', 28, lambda: L.cn_rmsprop(ptr(p), ptr(g), ptr(b2), ptr(b1), n, 0.0, 0.0, 0.9, 0.1, 1e-8, 1e-4,
                                                      1.0, ptr(clip), ptr(hyper), s)),
        ('optim_advance', 0, lambda: L.cn_optim_advance(ptr(step), ptr(corr), 0.1, 0.001, s)),
    ]
    flush = torch.empty(1 << 28, device=dev)      # 1 GiB
    times = {(name, kind): [] for name, _, _ in calls for kind in ('warm', 'cold')}
    for rep in range(args.repeats + 1):      # repeat 0 is the warm-up
        for name, _, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ev = []
            for _ in range(args.iters):
                flush.fill_(0.0)
                ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                ev[-1][0].record()
                fn()
                ev[-1][1].record()
            torch.cuda.synchronize()
            if rep:
                times[name, 'warm'].append(a.elapsed_time(b) / args.iters)
                times[name, 'cold'].append(sum(x.elapsed_time(y) for x, y in ev) / args.iters)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print('%s, arena %d floats (%.1f MB per buffer), %d repeats x %d calls' % (torch.cuda.get_device_name(0), n, n * 4 / 1e6,
                                                                               args.repeats, args.iters))
    print('kernel            | B/param | timing | ms (spread)       | GB/s  | rate / sgd_momentum')
    for kind in ('warm', 'cold'):
        sgd_rate = 20.0 * n / med['sgd_momentum', kind] / 1e6
        for name, bpp, _ in calls:
            v, m = times[name, kind], med[name, kind]
            if bpp:
                rate = bpp * n / m / 1e6
                print('%-17s | %7d | %-6s | %7.4f (%.4f)  | %5.0f | %.3f' % (name, bpp, kind, m, max(v) - min(v), rate,
                                                                             rate / sgd_rate))
            else:
                print('%-17s | %7s | %-6s | %7.4f (%.4f)  |       |' % (name, '-', kind, m, max(v) - min(v)))
    assert torch.isfinite(p).all()


if __name__ == '__main__':
    main()
