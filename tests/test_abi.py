"""The C-ABI library loads and exports every symbol include/convnet_hip.h declares (no compute
calls, so this runs without a GPU); the product loader refuses to fall back."""
import ctypes
import os
import re

import pytest

from helpers import ROOT

HIP_LIB = os.path.join(ROOT, 'convnet.pytorch_amd', 'libconvnet_hip.so')


def _header_symbols():
    txt = open(os.path.join(ROOT, 'include', 'convnet_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(cn_[a-z0-9_]+)\s*\(', txt)))


def test_header_and_binding_agree():
    import convnet_amd as ca
    assert _header_symbols() == list(ca._lib.EXPORTED_SYMBOLS)


def test_hip_library_exports_every_declared_symbol():
    if not os.path.exists(HIP_LIB):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(HIP_LIB)
    for name in _header_symbols():
        assert hasattr(lib, name), name
    lib.cn_is_emulator.restype = ctypes.c_int
    assert lib.cn_is_emulator() == 0
    lib.cn_build_info.restype = ctypes.c_char_p
    assert b'gfx950' in lib.cn_build_info()


def test_hip_library_was_built_from_this_tree():
    """cn_build_info() carries the content hash of the sources + headers the binary was compiled from (csrc/build.sh);
    _lib.source_hash() is the same recipe over the tree: a stale libconvnet_hip.so - which gpurun would ship to the GPU box
    and bench.py would measure - fails here (bench.py prints both hashes in its line)."""
    import convnet_amd as ca
    lib = ctypes.CDLL(HIP_LIB)
    lib.cn_build_info.restype = ctypes.c_char_p
    info = lib.cn_build_info().decode()
    if ca._lib.source_hash() not in info:
        import __graft_entry__ as g
        g.build()          # (rebuilt: the next process loads the fresh binary; this one checks the file again)
        import subprocess
        import sys
        out = subprocess.check_output([sys.executable, '-c', 'import ctypes; l = ctypes.CDLL(%r); '
                                       'l.cn_build_info.restype = ctypes.c_char_p; print(l.cn_build_info().decode())' % HIP_LIB])
        info = out.decode()
    assert ca._lib.source_hash() in info, (ca._lib.source_hash(), info)


def test_loader_fails_loudly_without_library(monkeypatch, tmp_path):
    import convnet_amd as ca
    monkeypatch.setattr(ca._lib, '_lib', None)
    monkeypatch.setattr(ca._lib, 'HIP_LIB', str(tmp_path / 'missing.so'))
    monkeypatch.setenv('CONVNET_AMD_EMULATE', '0')
    with pytest.raises(ca._lib.ConvNetHipError):
        ca._lib.load()


def test_ops_refuse_host_tensors_on_the_product_library():
    """With the real HIP library bound, CPU tensors are rejected instead of silently computed."""
    import torch
    import convnet_amd as ca
    if ca._lib.is_emulated():
        pytest.skip('emulator bound in this process')
    with pytest.raises(ca._lib.ConvNetHipError):
        ca.ops.nchw_to_nhwc(torch.zeros(1, 3, 4, 4), torch.float32)


# ---- the binding is parsed from the header (_lib.parse_header) -------------------------------------------------------

def test_parser_covers_the_header():
    import convnet_amd as ca
    txt = open(os.path.join(ROOT, 'include', 'convnet_hip.h')).read()
    assert sorted(ca._lib.parse_header(txt)) == _header_symbols()
    assert sorted(ca._lib._SIGNATURES) == _header_symbols()


def test_parsed_signatures_match_hand_written_ones():
    """Three declarations that span the type map, against literals copied from the hand-written table the parser
    replaced (size_t + floats; unsigned long long + long long; a string return)."""
    import convnet_amd as ca
    c_p, c_i, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    c_ll, c_sz, c_ull = ctypes.c_longlong, ctypes.c_size_t, ctypes.c_ulonglong
    want = {
        'cn_conv2d_wgrad': (c_i, [c_p, c_p, c_p, c_i] + [c_i] * 11 + [c_i, c_f, c_f, c_p, c_sz, c_p]),
        'cn_quantize': (c_i, [c_p, c_p, c_ll, c_i, c_p, c_p, c_i, c_p, c_i, c_ull, c_p]),
        'cn_build_info': (ctypes.c_char_p, []),
    }
    for name, (res, args) in want.items():
        got = ca._lib._SIGNATURES[name]
        assert (got[0], list(got[1])) == (res, args), name
    # the one string PARAMETER of the ABI stays a string, the opaque 128-byte id a plain pointer
    assert ca._lib._SIGNATURES['cn_set_option'][1] == [ctypes.c_char_p, c_i]
    assert ca._lib._SIGNATURES['cn_comm_init'][1] == [c_p, c_p, c_i, c_i]


@pytest.mark.parametrize('text', [
    'int cn_good(int a);\nint cn_bad(double v);',                 # a parameter type outside the ABI's vocabulary
    'struct cn_thing cn_bad(void);',                              # ... a return type
    'int cn_good(int a);\nint cn_bad(int (*callback)(int));',     # a declaration the pattern cannot account for
    'int cn_good(int a);\nint cn_bad(int a)\n',                   # ... (no terminating semicolon)
])
def test_parser_fails_loudly(text):
    import convnet_amd as ca
    with pytest.raises(ca._lib.ConvNetHipError):
        ca._lib.parse_header(text)
    assert list(ca._lib.parse_header('int cn_good(int a);')) == ['cn_good']


def test_status_return_raises_under_its_own_name():
    """A cn_status entry point raises from the binding itself, named after the symbol that failed: addend_sub = 3 is
    refused before any launch (no pointer is touched)."""
    import convnet_amd as ca
    L = ca._lib.load()
    with pytest.raises(ca._lib.ConvNetHipError) as e:
        L.cn_conv2d_dgrad_sa(None, None, None, None, 3, 1, 1, 1, 8, 8, 1, 1, 1, 1, 0, 0, 1, 0, None)
    assert str(e.value).startswith('cn_conv2d_dgrad_sa failed (rc=-'), str(e.value)


def test_value_return_still_returns_its_value():
    import convnet_amd as ca
    assert ca._lib.load().cn_conv2d_bnstats_rows(129) == 2
