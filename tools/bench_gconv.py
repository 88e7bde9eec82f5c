"""Per-kernel timing of the grouped 3x3 convolution (csrc/gconv.hip) on every ResNeXt-50 32x4d grouped shape, bf16,
N = 256: forward, data gradient, weight gradient (median of HIP-event timings), algorithmic bytes and the fraction of
the 8 TB/s HBM peak; for comparison only, PyTorch's own grouped forward, input gradient and weight gradient
(conv2d / torch.nn.grad.conv2d_input / conv2d_weight, groups=32, channels-last) on the same device.

    python tools/bench_gconv.py [--n 256] [--iters 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
SHAPES = [(56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2), (14, 512, 1), (14, 1024, 2), (7, 1024, 1)]


def _time(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--groups', type=int, default=32)
    a = ap.parse_args()
    import convnet_amd as ca
    from convnet_amd import ops
    dev, dt, g, N = torch.device('cuda', 0), torch.bfloat16, a.groups, a.n
    rows = []
    for H, C, st in SHAPES:
        K, P = C, (H - 1) // st + 1
        x = torch.randn(N, H, H, C, device=dev).to(dt)
        w = (torch.randn(K * 9 * (C // g), device=dev) * 0.05).to(dt)
        dy = torch.randn(N, P, P, K, device=dev).to(dt)
        dw = torch.zeros(K * 9 * (C // g), device=dev)
        wb = K * 9 * (C // g) * 2
        fwd_b = x.numel() * 2 + dy.numel() * 2 + wb
        wg_b = x.numel() * 2 + dy.numel() * 2 + K * 9 * (C // g) * 4
        r = {'shape': '%dx%d C=K=%d g=%d s%d' % (H, H, C, g, st)}
        for name, fn, nb in (('fwd', lambda: ops.gconv2d_fwd(x, w, K, g, st), fwd_b),
                             ('dgrad', lambda: ops.gconv2d_dgrad(dy, w, x.shape, K, g, st), fwd_b),
                             ('wgrad', lambda: ops.gconv2d_wgrad(x, dy, dw, K, g, st, beta=0.0), wg_b)):
            us = _time(fn, a.iters)
            r[name] = {'us': round(us, 1), 'bytes': nb, 'hbm_frac': round(nb / (us * 1e-6) / PEAK, 3)}
        xt = x.permute(0, 3, 1, 2)             # channels-last NCHW view of the same data
        wt = w.view(K, 3, 3, C // g).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        r['torch_fwd_us'] = round(_time(lambda: torch.nn.functional.conv2d(xt, wt, stride=st, padding=1, groups=g),
                                        a.iters), 1)
        dyt = dy.permute(0, 3, 1, 2)
        r['torch_dgrad_us'] = round(_time(lambda: torch.nn.grad.conv2d_input(xt.shape, wt, dyt, stride=st, padding=1,
                                                                              groups=g), a.iters), 1)
        r['torch_wgrad_us'] = round(_time(lambda: torch.nn.grad.conv2d_weight(xt, wt.shape, dyt, stride=st, padding=1,
                                                                               groups=g), a.iters), 1)
        rows.append(r)
        print(json.dumps(r), flush=True)
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'n': N, 'dtype': 'bf16',
                      'lib': os.path.relpath(ca._lib.HIP_LIB, ROOT)}))


if __name__ == '__main__':
    main()
