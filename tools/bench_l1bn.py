#!/usr/bin/env python
"""L1 batch norm kernels (csrc/l1bn.hip) beside the standalone BatchNorm passes (csrc/bn.hip) on the ResNet-50 shapes of
tools/bench_bn.py (B = 256, bf16): one process, the two alternated, HIP events after warm-up.

Per shape and operator three timed calls through the C ABI:
  stats   forward with z = NULL   L1: sum + mean + absdev + finalize (reads y twice)   BN: stats + finalize (reads y once)
  fwd     the whole forward       L1: reads y three times (+ residual), writes z      BN: reads y twice (+ residual), writes z
  bwd     the whole backward      both: reduce (dz, y) + finalize + apply (dz, y -> dy (+ dres))
Printed per line: median ms, min-max spread over the repeats and the achieved bytes/s of the nominal traffic."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convnet_amd as ca  # noqa: E402
from convnet_amd import ops  # noqa: E402
from bench_bn import SHAPES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--iters', type=int, default=5, help='calls per timed repeat')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib = ca._lib
    L = lib.load()
    ptr = lib.ptr
    code = ops.dtype_code(torch.bfloat16)
    tot = {}
    print('shape (count x [B,H,H,C], residual+relu) | call | L1: ms (spread) GB/s | BN: ms (spread) GB/s | L1 rate / BN rate')
    for cnt, C, H, res in SHAPES:
        M = args.batch * H * H
        y = torch.randn(M, C, device=dev).to(torch.bfloat16)
        r = torch.randn(M, C, device=dev).to(torch.bfloat16) if res else None
        dz = torch.randn(M, C, device=dev).to(torch.bfloat16)
        z, dy = torch.empty_like(y), torch.empty_like(y)
        dres = torch.empty_like(y) if res else None
        mask = torch.empty(M * (C // 8), dtype=torch.uint8, device=dev) if res else None
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbt = torch.zeros(1, dtype=torch.long, device=dev)
        st_l1, st_bn = torch.empty(7 * C, device=dev), torch.empty(4 * C, device=dev)
        coef = torch.empty(3 * C, device=dev)
        ws = ops.workspace(max(L.cn_l1bn_workspace(M, C, code), L.cn_bn_workspace(M, C, code)), dev, tag='bench_l1bn')
        wsb = ws.numel() * 4
        s = lib.stream_of(y)
        nb = y.numel() * 2
        mb = mask.numel() if mask is not None else 0

        def l1_fwd(zz):
            L.cn_l1bn_fwd_train(ptr(y), ptr(r) if zz is not None else None, ptr(zz), ptr(mask) if zz is not None else None,
                                ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5, ptr(st_l1), M, C, 1, code, ptr(ws), wsb, s)

        def bn_fwd(zz):
            L.cn_bn_fwd_train(ptr(y), ptr(r) if zz is not None else None, ptr(zz), ptr(mask) if zz is not None else None,
                              ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), 0.1, 1e-5, ptr(st_bn), M, C, 1, code,
                              ptr(ws), wsb, s)

        calls = {
            'stats': (lambda: l1_fwd(None), lambda: bn_fwd(None), 2 * nb, nb),
            'fwd': (lambda: l1_fwd(z), lambda: bn_fwd(z), nb * (5 if res else 4) + mb, nb * (4 if res else 3) + mb),
            'bwd': (lambda: L.cn_l1bn_bwd(ptr(dz), ptr(y), ptr(mask), ptr(gamma), ptr(st_l1), ptr(dy), ptr(dres), ptr(dg),
                                          ptr(db), 0.0, 1.0, ptr(coef), M, C, 1, code, ptr(ws), wsb, s),
                    lambda: L.cn_bn_bwd(ptr(dz), ptr(y), ptr(mask), ptr(gamma), ptr(st_bn), ptr(dy), ptr(dres), ptr(dg),
                                        ptr(db), 0.0, 1.0, ptr(coef), M, C, 1, code, ptr(ws), wsb, s),
                    nb * (6 if res else 5) + 2 * mb, nb * (6 if res else 5) + 2 * mb),
        }
        l1_fwd(z)
        bn_fwd(z)     # (statistics for the backward calls)
        for name, (f_l1, f_bn, bytes_l1, bytes_bn) in calls.items():
            times = {'l1': [], 'bn': []}
            for rep in range(args.repeats + 1):      # repeat 0 is the warm-up
                for which, fn in (('l1', f_l1), ('bn', f_bn)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.iters):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    if rep:
                        times[which].append(a.elapsed_time(b) / args.iters)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            spr = {k: max(v) - min(v) for k, v in times.items()}
            rate = {'l1': bytes_l1 / med['l1'] / 1e6, 'bn': bytes_bn / med['bn'] / 1e6}
            print('%2d x [%d,%3d,%3d,%4d] res=%d | %-5s | %7.4f (%.4f) %6.0f | %7.4f (%.4f) %6.0f | %.3f'
                  % (cnt, args.batch, H, H, C, res, name, med['l1'], spr['l1'], rate['l1'], med['bn'], spr['bn'], rate['bn'],
                     rate['l1'] / rate['bn']))
            t = tot.setdefault(name, [0.0, 0.0])
            t[0] += cnt * med['l1']
            t[1] += cnt * med['bn']
    for name, (a, b) in tot.items():
        print('per ResNet-50 step, %-5s: L1 %.3f ms   standalone BatchNorm %.3f ms   ratio %.3f' % (name, a, b, a / b))


if __name__ == '__main__':
    main()
