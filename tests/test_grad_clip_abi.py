"""CPU checks of the gradient-norm / clipping boundary (csrc/gradnorm.hip and the ``_dev`` optimizer entry points): bad arguments are
refused on the host, before any launch, with the codes of the neighbouring functions (2: NULL pointer / bad size / misaligned,
1: unsupported shape, 4: workspace too small), and the workspace sizes are positive and monotone."""
import ctypes


def _lib_and_fake():
    from driving_dirty_amd import _lib
    return _lib, _lib.lib(), ctypes.c_void_p(4096)


def test_sqnorm_entry_points_refuse_bad_arguments_without_a_gpu():
    _lib, lib, fake = _lib_and_fake()
    assert lib.dd_sqnorm(None, 8, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm(fake, 8, None, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm(fake, 8, fake, None, 1 << 20, None) == 2
    assert lib.dd_sqnorm(fake, 0, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm(fake, -5, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm(ctypes.c_void_p(4100), 8, fake, fake, 1 << 20, None) == 2          # 16-byte loads
    assert lib.dd_sqnorm(fake, 1 << 22, fake, fake, 8, None) == 4
    assert b"workspace" in lib.dd_last_error()
    table = (_lib.AdamTensor * 2)(_lib.AdamTensor(None, fake, None, None, 32), _lib.AdamTensor(None, fake, None, None, 9216))
    assert lib.dd_sqnorm_multi(None, 2, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm_multi(table, 0, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm_multi(table, -1, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm_multi(table, 2, None, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm_multi(table, 2, fake, fake, 8, None) == 4
    bad = (_lib.AdamTensor * 2)(_lib.AdamTensor(None, fake, None, None, 32), _lib.AdamTensor(None, None, None, None, 16))
    assert lib.dd_sqnorm_multi(bad, 2, fake, fake, 1 << 20, None) == 2
    bad[1] = _lib.AdamTensor(None, fake, None, None, 0)
    assert lib.dd_sqnorm_multi(bad, 2, fake, fake, 1 << 20, None) == 2
    assert lib.dd_sqnorm_multi_workspace_bytes(bad, 2) == -1
    assert lib.dd_sqnorm_multi_workspace_bytes(None, 2) == -1


def test_rankb_sqnorm_and_clip_scale_refuse_bad_arguments_without_a_gpu():
    _lib, lib, fake = _lib_and_fake()
    big = 1 << 24
    assert lib.dd_rankb_sqnorm(None, fake, 32, 64, 260, 1, fake, fake, big, None) == 2
    assert lib.dd_rankb_sqnorm(fake, None, 32, 64, 260, 1, fake, fake, big, None) == 2
    assert lib.dd_rankb_sqnorm(fake, fake, 32, 64, 260, 1, None, fake, big, None) == 2
    assert lib.dd_rankb_sqnorm(fake, fake, 0, 64, 260, 1, fake, fake, big, None) == 2
    assert lib.dd_rankb_sqnorm(fake, fake, 32, 0, 260, 1, fake, fake, big, None) == 2
    assert lib.dd_rankb_sqnorm(fake, fake, 65, 64, 260, 1, fake, fake, big, None) == 1        # as dd_adam_step_rankb
    assert b"65" in lib.dd_last_error()
    assert lib.dd_rankb_sqnorm(fake, fake, 32, 64, 262, 1, fake, fake, big, None) == 1        # k % 4
    assert lib.dd_rankb_sqnorm(fake, fake, 32, 62, 260, 1, fake, fake, big, None) == 1        # n % 4
    assert lib.dd_rankb_sqnorm(ctypes.c_void_p(4100), fake, 32, 64, 260, 1, fake, fake, big, None) == 2
    assert lib.dd_rankb_sqnorm(fake, fake, 32, 64, 260, 1, fake, fake, 8, None) == 4
    assert lib.dd_clip_scale(None, 3, 1.0, 1.0, fake, None) == 2
    assert lib.dd_clip_scale(fake, 3, 1.0, 1.0, None, None) == 2
    assert lib.dd_clip_scale(fake, 0, 1.0, 1.0, fake, None) == 2
    assert lib.dd_clip_scale(fake, -3, 1.0, 1.0, fake, None) == 2


def test_device_scale_optimizer_entry_points_refuse_bad_arguments_without_a_gpu():
    _lib, lib, fake = _lib_and_fake()
    adam = (1e-3, 0.9, 0.999, 1e-8, 1)
    assert lib.dd_adam_step_dev(fake, fake, fake, fake, 16, *adam, None, None) == 2           # no scale
    assert lib.dd_adam_step_dev(None, None, None, None, 16, *adam, fake, None) == 2
    assert lib.dd_adam_step_dev(fake, fake, fake, fake, 0, *adam, fake, None) == 2
    assert lib.dd_adam_step_multi_dev(None, 0, *adam, fake, None) == 2
    table = (_lib.AdamTensor * 1)(_lib.AdamTensor(fake, fake, fake, fake, 32))
    assert lib.dd_adam_step_multi_dev(table, 1, *adam, None, None) == 2
    assert lib.dd_adam_step_multi_dev(table, 0, *adam, fake, None) == 2
    rankb = lambda rows, n, k, scale: lib.dd_adam_step_rankb_dev(fake, fake, fake, fake, fake, rows, n, k, None, None, None, *adam, scale, None)
    assert rankb(32, 64, 260, None) == 2
    assert rankb(65, 64, 260, fake) == 1
    assert rankb(32, 64, 262, fake) == 1
    assert rankb(0, 64, 260, fake) == 2
    assert lib.dd_adam_step_rankb_dev(None, fake, fake, fake, fake, 32, 64, 260, None, None, None, *adam, fake, None) == 2


def test_norm_workspace_sizes_are_positive_and_monotone():
    _lib, lib, fake = _lib_and_fake()
    assert lib.dd_sqnorm_workspace_bytes(0) == -1 and lib.dd_sqnorm_workspace_bytes(-1) == -1
    sizes = [lib.dd_sqnorm_workspace_bytes(n) for n in (1, 3, 4, 1027, 4 * 256 * 7 + 5, (1 << 21) + 7, 1 << 28, 1 << 33)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    ns = (1, 32, 288, 9216, 65536)
    table = (_lib.AdamTensor * 49)(*[_lib.AdamTensor(None, fake, None, None, ns[i % 5]) for i in range(49)])
    sizes = [lib.dd_sqnorm_multi_workspace_bytes(table, c) for c in (1, 2, 5, 48, 49)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert lib.dd_rankb_sqnorm_workspace_bytes(0, 64, 64) == -1 and lib.dd_rankb_sqnorm_workspace_bytes(65, 64, 64) == -1
    ws = lib.dd_rankb_sqnorm_workspace_bytes
    for series in ([ws(r, 128, 4096) for r in (1, 3, 16, 17, 32, 33, 64)], [ws(32, n, 64) for n in (4, 64, 132, 4100, 640000)],
                   [ws(32, 128, k) for k in (4, 260, 4100, 940032)]):
        assert all(s > 0 for s in series) and series == sorted(series) and series[0] < series[-1], series
