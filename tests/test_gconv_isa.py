"""The grouped-convolution kernels in libconvnet_hip.so are what csrc/gconv.hip claims: MFMA kernels, no scratch spill
beyond the 16 bytes per lane the bf16 kernels of the step may use, LDS within the CU's 160 KB (no GPU needed)."""
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import isa_check  # noqa: E402

HIP_LIB = os.path.join(ROOT, 'convnet.pytorch_amd', 'libconvnet_hip.so')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(HIP_LIB):
        import __graft_entry__ as g
        g.build()
    return HIP_LIB


def test_gconv_kernels_are_mfma_and_fit(lib):
    table = isa_check.kernel_table(lib)
    res = isa_check.kernel_resources(lib)
    for kern in ('gconv_kernel<bf16_t, true>', 'gconv_kernel<bf16_t, false>', 'gconv_dw_kernel<bf16_t>',
                 'gconv_kernel<f16_t, true>', 'gconv_dw_kernel<f16_t>', 'gconv_kernel<float', 'gconv_dw_kernel<float>'):
        hits = [(k, v) for k, v in table.items() if kern in k]
        assert hits, kern
        assert all(v['mfma'] > 0 for _, v in hits), hits
        for k, r in ((k, res[k]) for k in res if kern in k):
            assert r['lds'] <= 160 * 1024, (k, r)
            if 'bf16_t' in k:
                assert r['scratch'] <= 16, (k, r)
