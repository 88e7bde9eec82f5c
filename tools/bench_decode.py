#!/usr/bin/env python
"""Decode + augment throughput of the image-folder input pipeline (convnet.pytorch_amd/data.py: PIL decode,
RandomResizedCrop(224), flip, ToTensor, Normalize) on synthetic ImageNet-sized JPEGs, per worker count.
CPU only (measurement aid; SURVEY.md section 8f-3: the step needs ~12k img/s per GPU).
--duplicates D: D views per decoded image (rates are training images = samples * D per second).
--cost-split: instead of the loaders, the per-image worker cost in ONE process, split into decode / crop / resize /
ToTensor + Normalize for the host multi_transform path and decode / draw + region crop for the device-views path."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('CONVNET_AMD_EMULATE', '1')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=512)
    ap.add_argument('--workers', default='1,4,8')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--device-normalize', action='store_true', help='workers stop at the uint8 crop (ToTensor + Normalize on the device)')
    ap.add_argument('--device-resize', action='store_true', help='... and at the unresized crop (PIL resize on the device too)')
    ap.add_argument('--duplicates', type=int, default=1)
    ap.add_argument('--cost-split', action='store_true')
    args = ap.parse_args()
    from PIL import Image
    import torch
    from convnet_amd import data as D
    root = tempfile.mkdtemp()
    rng = np.random.RandomState(0)
    for c in range(4):
        os.makedirs(os.path.join(root, 'imagenet', 'train', 'c%d' % c))
    for i in range(args.images):     # ~500x375 photos-like noise + gradients (average ImageNet size ~110 KB)
        a = (rng.rand(375, 500, 3) * 60 + np.linspace(0, 180, 500)[None, :, None]).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(root, 'imagenet', 'train', 'c%d' % (i % 4), '%05d.jpg' % i), quality=90)
    if args.cost_split:
        return cost_split(root, args.duplicates, min(args.images, 256))
    for nw in [int(w) for w in args.workers.split(',')]:
        dr = D.DataRegime([{'epoch': 0}], defaults={'datasets_path': root, 'name': 'imagenet', 'split': 'train',
                                                     'augment': True, 'input_size': 224, 'batch_size': args.batch,
                                                     'shuffle': True, 'num_workers': nw, 'drop_last': True,
                                                     'duplicates': args.duplicates,
                                                     'device_normalize': args.device_normalize or args.device_resize,
                                                     'device_resize': args.device_resize})
        loader = dr.get_loader()
        n = 0
        for x, t in loader:     # warm-up epoch (worker start-up, page cache)
            n += t.shape[0]
        t0 = time.time()
        n = 0
        for x, t in loader:
            n += t.shape[0] * args.duplicates
        dt = time.time() - t0
        print('workers %2d: %7.1f img/s (%d images, %.2f s; %.1f img/s per worker)' % (nw, n / dt, n, dt, n / dt / max(nw, 1)))
        del loader, dr
    print('host: %d usable cores (torch threads %d)' % (len(os.sched_getaffinity(0)), torch.get_num_threads()))


def cost_split(root, dup, n):
    """ms per decoded image, one process, median over the images."""
    import torch
    from PIL import Image
    from convnet_amd import data as D
    ds = D.ImageFolder(os.path.join(root, 'imagenet', 'train'))
    rrc, views = D.RandomResizedCrop(224), D.RandomResizedCropViews(224, dup)
    tt, nz = D.ToTensor(), D.Normalize(**D._IMAGENET_STATS)
    rows = []
    torch.manual_seed(0)
    for i in range(n):
        path = ds.samples[i][0]
        t = [time.perf_counter()]
        with open(path, 'rb') as f:
            img = Image.open(f)
            img.load()
        t.append(time.perf_counter())
        boxes = [rrc.get_params(*img.size) for _ in range(dup)]
        crops = [img.crop((l, tp, l + w, tp + h)) for l, tp, w, h in boxes]
        t.append(time.perf_counter())
        small = [c.resize((224, 224), Image.BILINEAR) for c in crops]
        t.append(time.perf_counter())
        u8 = [np.array(s_, dtype=np.uint8) for s_ in small]
        t.append(time.perf_counter())
        _ = [nz(tt(s_)) for s_ in small]
        t.append(time.perf_counter())
        _ = views(img)
        t.append(time.perf_counter())
        rows.append([(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])])
    med = np.median(np.array(rows), axis=0)
    names = ['decode', 'draw + crop x D', 'resize x D', 'to uint8 x D', 'ToTensor + Normalize x D', 'views: draw + region crop + tables']
    print('duplicates %d, %d images, ms per decoded image (median):' % (dup, n))
    for k, v in zip(names, med):
        print('  %-38s %7.3f' % (k, v))
    host = med[0] + med[1] + med[2] + med[4]
    dn = med[0] + med[1] + med[2] + med[3]
    dv = med[0] + med[5]
    print('  host multi_transform %.3f ms, device-normalize %.3f ms, device-views %.3f ms per sample -> %.2fx / %.2fx fewer worker ms'
          % (host, dn, dv, host / dv, dn / dv))


if __name__ == '__main__':
    main()
