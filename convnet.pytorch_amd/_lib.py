"""ctypes binding of libconvnet_hip.so (C ABI declared in include/convnet_hip.h).

This is the drop-in boundary: everything above it is Python host code mirroring the reference's
operator / trainer interface, everything below it is hand-written HIP for gfx950.  The library is
built in-tree by ``__graft_entry__.build()`` (or ``csrc/build.sh``).  The signatures are not written
down here: they are parsed from the header the library itself is compiled against (``parse_header``).

There is deliberately NO fallback: if the HIP library is missing, loading raises.  The only other
library this module can bind is the TEST-ONLY SIMT emulator build of the *same kernel sources*
(``libconvnet_emul.so``), and only when ``CONVNET_AMD_EMULATE=1`` is set explicitly (the CPU test
suite does that); it is refused whenever a GPU is visible.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CONVNET_AMD_HIP_LIB: alternative build of the same library for A/B measurement (csrc/build.sh CN_LIB_NAME)
HIP_LIB = os.path.join(_HERE, os.environ.get('CONVNET_AMD_HIP_LIB', 'libconvnet_hip.so'))
EMUL_LIB = os.path.join(_HERE, 'libconvnet_emul.so')

F32, BF16, F16 = 0, 1, 2

HEADER = os.path.join(_HERE, '..', 'include', 'convnet_hip.h')


class ConvNetHipError(RuntimeError):
    pass


# C type -> ctypes, for everything that is not a pointer (any pointer is a void*, except strings: see _ctype)
_CTYPES = {'int': ctypes.c_int, 'float': ctypes.c_float, 'long long': ctypes.c_longlong, 'size_t': ctypes.c_size_t,
           'unsigned long long': ctypes.c_ulonglong, 'cn_status': ctypes.c_int}
_DECL = re.compile(r'([A-Za-z_][A-Za-z0-9_ ]*?[ *]+)(cn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;')


def _ctype(ctype, what):
    ctype = ' '.join(ctype.replace('*', ' * ').split())
    if ctype == 'const char *':
        return ctypes.c_char_p
    if ctype.endswith('*'):
        return ctypes.c_void_p
    if ctype not in _CTYPES:
        raise ConvNetHipError('convnet_hip.h: unknown type %r in %s' % (ctype, what))
    return _CTYPES[ctype]


def parse_header(text):
    """The C ABI as declared: name -> (restype, argtypes, is_status) for every `ret cn_name(args);` of the header text.
    Raises on a type outside the ABI's vocabulary and on any `cn_name(` the declaration pattern did not account for."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    named = set(re.findall(r'\b(cn_[a-z0-9_]+)\s*\(', text))
    text = re.sub(r'^\s*(#|typedef\b|extern "C").*$', '', text, flags=re.M)
    sigs = {}
    for ret, name, args in _DECL.findall(text):
        args = [a.strip() for a in args.split(',')]
        if args == ['void']:
            args = []
        # a parameter is `type name`: the type is everything up to the last identifier
        argtypes = [_ctype(re.sub(r'[A-Za-z_][A-Za-z0-9_]*$', '', a), '%s(%s)' % (name, a)) for a in args]
        sigs[name] = (_ctype(ret, 'the return of ' + name), argtypes, ret.strip() == 'cn_status')
    if set(sigs) != named:
        raise ConvNetHipError('convnet_hip.h: not parsed as declarations: %s' % sorted(named ^ set(sigs)))
    return sigs


# name -> (restype, argtypes, is_status): include/convnet_hip.h is the only place the ABI is written down
with open(HEADER) as _f:
    _SIGNATURES = parse_header(_f.read())

EXPORTED_SYMBOLS = tuple(sorted(_SIGNATURES))

_lib = None
_emulated = False


def _raise_on_status(lib, name):
    def errcheck(rc, func, args):
        if rc != 0:
            msg = lib.cn_last_error()
            raise ConvNetHipError('%s failed (rc=%d): %s' % (name, rc, msg.decode() if msg else ''))
        return rc
    return errcheck


def _bind(path):
    lib = ctypes.CDLL(path)
    for name, (res, args, is_status) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = symbol missing: fail loudly
        fn.restype = res
        fn.argtypes = args
        if is_status:     # "0 or a negative CN_E* code": a failure raises under the entry point's own name
            fn.errcheck = _raise_on_status(lib, name)
    return lib


def emulation_requested():
    return os.environ.get('CONVNET_AMD_EMULATE', '0') == '1'


def load():
    """Load (once) and return the bound library."""
    global _lib, _emulated
    if _lib is not None:
        return _lib
    if emulation_requested():
        if torch.cuda.is_available():
            raise ConvNetHipError('CONVNET_AMD_EMULATE=1 is refused when a GPU is visible: '
                                  'the emulator is a CPU-only test harness, not a product path')
        if not os.path.exists(EMUL_LIB):
            raise ConvNetHipError('emulator library missing: run csrc/build.sh emul')
        _lib = _bind(EMUL_LIB)
        _emulated = True
        _apply_env_options(_lib)
        return _lib
    if not os.path.exists(HIP_LIB):
        raise ConvNetHipError(
            'libconvnet_hip.so not found at %s -- build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` (hipcc --offload-arch=gfx950).  There is no CPU / PyTorch fallback.' % HIP_LIB)
    _lib = _bind(HIP_LIB)
    _emulated = False
    _apply_env_options(_lib)
    return _lib


def _apply_env_options(lib):
    """CONVNET_AMD_OPTIONS="name=value,..." -> cn_set_option: kernel-variant tuning knobs for A/B
    measurement (results never change)."""
    for item in os.environ.get('CONVNET_AMD_OPTIONS', '').split(','):
        if '=' in item:
            k, v = item.split('=', 1)
            lib.cn_set_option(k.strip().encode(), int(v))


def source_hash():
    """Content hash of the library's sources + headers in THIS tree, by the recipe of csrc/build.sh (SRC_HASH): equal to
    the hash inside cn_build_info() exactly when the loaded binary was built from these files."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, 'csrc')
    srcs = re.search(r'^SRCS="([^"]+)"', open(os.path.join(csrc, 'build.sh')).read(), re.M).group(1).split()
    files = [os.path.join(csrc, f) for f in srcs] + sorted(glob.glob(os.path.join(csrc, '*.h'))) + \
        [HEADER]
    h = hashlib.sha1()
    for f in files:
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_hash():
    """The source hash compiled into the loaded library ('unknown' for a build that bypassed csrc/build.sh)."""
    info = load().cn_build_info().decode()
    return info.rsplit('src ', 1)[1] if 'src ' in info else 'unknown'


def is_emulated():
    load()
    return _emulated


def last_error():
    msg = load().cn_last_error()
    return msg.decode() if msg else ''


def check(rc, what=''):
    if rc != 0:
        msg = load().cn_last_error()
        raise ConvNetHipError('%s failed (rc=%d): %s' % (what, rc, msg.decode() if msg else ''))


def dtype_code(dtype):
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float16:
        return F16
    raise ConvNetHipError('unsupported compute dtype %s (float32 / bfloat16 / float16 only)' % dtype)


def chunk_elems(dtype):
    return 4 if dtype == torch.float32 else 8


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_of(t):
    """Raw hipStream_t of torch's current stream on the tensor's device (NULL for the emulator)."""
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    if not is_emulated():
        raise ConvNetHipError('tensor is on %s but the HIP library needs device memory' % t.device)
    return None


def require_device(t, name='tensor'):
    if not t.is_cuda and not is_emulated():
        raise ConvNetHipError('%s must live on a HIP device (got %s)' % (name, t.device))
    if not t.is_contiguous():
        raise ConvNetHipError('%s must be contiguous' % name)
