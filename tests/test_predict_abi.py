"""CPU checks of the prediction path's boundary: dd_ts_hist and dd_linear_sigmoid_gt refuse unsupported arguments on the host, before
any launch (the pointers here are never dereferenced), and the Python shims refuse CPU tensors."""
import ctypes

import pytest
import torch


def test_host_side_validation_of_the_prediction_entry_points():
    from driving_dirty_amd import _lib, ops
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    for bins, n, dtype in ((3, 8, 0), (2048, 8, 0), (1, 8, 0), (256, 6, 0), (256, 0, 0), (256, 8, 7)):
        assert lib.dd_ts_hist(fake, fake, dtype, n, bins, fake, None) == 1, (bins, n, dtype)
        assert b"ts_hist" in lib.dd_last_error()
    assert lib.dd_ts_hist(None, fake, 0, 8, 256, fake, None) == 2
    assert lib.dd_ts_hist(ctypes.c_void_p(4100), fake, 0, 8, 256, fake, None) == 2          # 16-byte loads
    assert lib.dd_linear_sigmoid_gt(fake, fake, None, 0.5, fake, 2, 64, 6, None) == 1       # K % 4
    assert lib.dd_linear_sigmoid_gt(fake, fake, None, 0.5, fake, 2, 64, 1024, None) == 1    # dd_linear_fwd would split K here
    assert b"splits K" in lib.dd_last_error()
    assert lib.dd_linear_sigmoid_gt(None, fake, None, 0.5, fake, 2, 64, 64, None) == 2
    assert lib.dd_linear_sigmoid_gt(fake, fake, None, 0.5, fake, 0, 64, 64, None) == 2
    with pytest.raises(_lib.HotpathError):
        ops.ts_histogram(torch.zeros(8), torch.zeros(8))
    with pytest.raises(_lib.HotpathError):
        ops.linear_sigmoid_gt(torch.zeros(2, 8), torch.zeros(4, 8), None, 0.5)
