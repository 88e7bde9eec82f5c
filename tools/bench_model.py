"""Steady-state training steps of any registry model (plan on after warm-up, HIP events): img/s, ms/step, then one
profiled step's per-kernel table (every kernel alone: the side stream folded in).

    python tools/bench_model.py --model resnext --model-config "{'depth': 50}" -b 256 --dtype bf16 --steps 20 --warmup 5"""
import argparse
import ast
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='resnext')
    ap.add_argument('--model-config', default="{'depth': 50}")
    ap.add_argument('-b', '--batch-size', type=int, default=256)
    ap.add_argument('--input-size', type=int, default=224)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f16', 'f32'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--top', type=int, default=25)
    a = ap.parse_args()
    import convnet_amd as ca
    dt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[a.dtype]
    dev = torch.device('cuda', 0)
    torch.manual_seed(123)
    model = ca.models.__dict__[a.model](**ast.literal_eval(a.model_config))
    ncls = model.fc.out_features
    tr = ca.Trainer(model, ca.CrossEntropyLoss(), ca.OptimRegime(model, model.regime), device='cuda:0', dtype=dt,
                    print_freq=10 ** 9)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch_size, 3, a.input_size, a.input_size, generator=g).to(dev)
    t = torch.randint(0, ncls, (a.batch_size,), generator=g).to(dev)
    for _ in range(a.warmup):
        tr.train([(x, t)])
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.steps):
        r = tr.train([(x, t)])
    e.record()
    e.synchronize()
    ms = s.elapsed_time(e) / a.steps
    out = {'model': a.model, 'config': a.model_config, 'batch': a.batch_size, 'dtype': a.dtype, 'ms_per_step': round(ms, 3),
           'img_per_s': round(a.batch_size / ms * 1e3, 1), 'loss': float(r['loss']),
           # whether the timed steps replayed a recorded launch plan (the capture state, not the flag)
           'plan_ran': any(g['graph'] is not None and g['graph'].get('plan') is not None for g in tr._gstates.values())}
    print(json.dumps(out), flush=True)
    # one profiled step, every kernel alone
    ca.ops.PROFILER.enabled, ca.ops.PROFILER.records = True, []
    use = tr._use_graph
    tr._use_graph = False
    tr.train([(x, t)])
    tr._use_graph = use
    ca.ops.PROFILER.enabled = False
    agg = ca.ops.PROFILER.summary()
    total = sum(v['ms'] for v in agg.values())
    print('%-70s %6s %9s %7s %9s' % ('kernel', 'calls', 'ms', 'share', 'TB/s'))
    for name, v in sorted(agg.items(), key=lambda kv: -kv[1]['ms'])[:a.top]:
        print('%-70s %6d %9.3f %6.1f%% %9.2f' % (name[:70], v['calls'], v['ms'], 100 * v['ms'] / total,
                                               v['bytes'] / max(v['ms'], 1e-9) / 1e9))
    print('profiled step (kernels alone): %.3f ms' % total)


if __name__ == '__main__':
    main()
