"""Per-kernel timing of the depthwise 3x3 convolution (csrc/dwconv.hip) on every distinct depthwise shape of MobileNet-1.0
at 224, bf16, N = 256: forward (with bias), data gradient, weight + bias gradient - beside the route the same bias-free
layer took before, the grouped MFMA kernels with groups = C (ops.gconv2d_*, csrc/gconv.hip).  The two are alternated
call by call in one process (HIP-event timings; median and min..max), with the algorithmic bytes and the achieved bytes/s;
results of the two routes are compared first (rel-L2) on the same tensors.

    python tools/bench_dwconv.py [--n 256] [--iters 20] [--out profiles/mobilenet_dwconv_kernels.txt]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (H, C, stride); the 14 x 14 / 512 / stride-1 shape occurs five times in the model
SHAPES = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 2),
          (7, 1024, 1)]


def _time_pair(fa, fb, iters):
    """fa / fb alternated; per function (median, min, max) in microseconds."""
    for _ in range(3):
        fa()
        fb()
    ts = ([], [])
    for _ in range(iters):
        for k, fn in enumerate((fa, fb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    import convnet_amd as ca
    from convnet_amd import ops
    if not torch.cuda.is_available() or ca._lib.is_emulated():
        raise SystemExit('bench_dwconv.py measures on the GPU')
    dev, dt, N = torch.device('cuda', 0), torch.bfloat16, a.n
    lines = ['# %s' % json.dumps({'device': torch.cuda.get_device_name(0), 'n': N, 'dtype': 'bf16', 'iters': a.iters,
                                  'build': ca._lib.source_hash()}),
             '# us: median (min..max) of alternated calls; TB/s: algorithmic bytes (read x / dy once, write the result once)'
             ' over the median; ratio: gconv us / dwconv us',
             '%-22s %-6s %26s %7s %26s %7s %6s %9s' % ('shape', 'kernel', 'dwconv us', 'TB/s', 'gconv(groups=C) us', 'TB/s',
                                                     'ratio', 'rel-L2')]
    for H, C, st in SHAPES:
        P = (H - 1) // st + 1
        x = torch.randn(N, H, H, C, device=dev).to(dt)
        wk = (torch.randn(C, 9, device=dev) * 0.3).to(dt)             # [C][3][3][1]: the grouped kernels' copy
        wt = wk.t().contiguous()                                      # [3][3][C]: the depthwise kernels' copy
        bias = torch.randn(C, device=dev)
        dy = torch.randn(N, P, P, C, device=dev).to(dt)
        dw, db, dwg = torch.zeros(C * 9, device=dev), torch.zeros(C, device=dev), torch.zeros(C * 9, device=dev)
        fwd_b = x.numel() * 2 + dy.numel() * 2 + C * 9 * 2
        wg_b = x.numel() * 2 + dy.numel() * 2 + C * 10 * 4
        wkf = wk.reshape(-1)
        ops.dwconv_wgrad(x, dy, dw, None, st, beta=0.0)
        ops.gconv2d_wgrad(x, dy, dwg, C, C, st, beta=0.0)
        errs = {'fwd': _rel(ops.dwconv_fwd(x, wt, None, st), ops.gconv2d_fwd(x, wkf, C, C, st)),
                'dgrad': _rel(ops.dwconv_dgrad(dy, wt, x.shape, st), ops.gconv2d_dgrad(dy, wkf, x.shape, C, C, st)),
                'wgrad': _rel(dw, dwg)}
        for name, fa, fb, nb in (
                ('fwd', lambda: ops.dwconv_fwd(x, wt, bias, st), lambda: ops.gconv2d_fwd(x, wkf, C, C, st), fwd_b),
                ('dgrad', lambda: ops.dwconv_dgrad(dy, wt, x.shape, st),
                 lambda: ops.gconv2d_dgrad(dy, wkf, x.shape, C, C, st), fwd_b),
                ('wgrad', lambda: ops.dwconv_wgrad(x, dy, dw, db, st, beta=0.0),
                 lambda: ops.gconv2d_wgrad(x, dy, dwg, C, C, st, beta=0.0), wg_b)):
            (ma, la, ha), (mb, lb, hb) = _time_pair(fa, fb, a.iters)
            lines.append('%-22s %-6s %26s %7.2f %26s %7.2f %6.2f %9.2g' % (
                '%dx%d C=%d s%d' % (H, H, C, st), name, '%.1f (%.1f..%.1f)' % (ma, la, ha), nb / (ma * 1e-6) / 1e12,
                '%.1f (%.1f..%.1f)' % (mb, lb, hb), nb / (mb * 1e-6) / 1e12, mb / ma, errs[name]))
            print(lines[-1], flush=True)
        del x, dy
    text = '\n'.join(lines) + '\n'
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
