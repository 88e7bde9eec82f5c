"""ResNeXt (/root/reference models/resnext.py): ResNet_imagenet with width=[128, 256, 512, 1024], groups=[32]*4 and
expansion=2 as defaults, so every 3x3 convolution is grouped (ops.GroupedConv2dFunction on csrc/gconv.hip).  The ImageNet
variant only; resnext_se (SE blocks) is not registered."""
from .resnet import ResNetImagenet, _IMAGENET_DEPTHS

__all__ = ['resnext']

_RESNEXT_DEPTHS = (18, 34, 50, 101, 152)


def resnext(**config):
    """Factory with the reference's call shape: resnext(dataset=..., depth=..., **kw).  Unlike resnet(), depths 18 / 34
    keep expansion 2 (the reference's ResNeXt_imagenet default): both 3x3 convolutions of a BasicBlock are grouped."""
    dataset = config.pop('dataset', 'imagenet')
    if 'imagenet' not in dataset:
        raise NotImplementedError("only the ImageNet ResNeXt variant is built natively (dataset=%r)" % dataset)
    if config.pop('bn_norm', None):
        raise NotImplementedError("resnext(bn_norm=...) is not part of the MI355X hot path")
    config['quantize'] = bool(config.pop('quantize', False))
    config.setdefault('num_classes', 1000)
    depth = config.pop('depth', 50)
    if depth not in _RESNEXT_DEPTHS:
        raise ValueError('unsupported ResNeXt depth %r' % depth)
    kind, layers = _IMAGENET_DEPTHS[depth]
    config.update(block=kind, layers=layers)
    config.setdefault('width', [128, 256, 512, 1024])
    config.setdefault('groups', [32, 32, 32, 32])
    config.setdefault('expansion', 2)
    return ResNetImagenet(**config)
