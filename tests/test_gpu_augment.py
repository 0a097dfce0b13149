"""The three augmentation kernels (csrc/augment.hip) against tests/_augment_ref.py: pure byte shuffling plus two fp32 operations,
so every comparison is on the raw bits.

Shapes: odd W (the mirror's centre column), W % 4 != 0 (a 16-byte store that crosses rows), both kernels of the view launchers --
H * W % 4 == 0 goes plane by plane ((4,5), (3,8), (16,22), 256 x 306), anything else over the flat array, where a store also crosses
planes, views and samples and an element count that is no multiple of 4 leaves a scalar tail ((1,1), (2,3)) --, batches on both
sides of the launcher's chunk (augment.CHUNK) for each of the two, one case at the cameras' 256 x 306."""
import pytest
import torch

import _augment_ref as ref

from driving_dirty_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (4, 5), (3, 8), (16, 22)]
MASK_SHAPES = [(1, 4), (3, 4), (8, 8), (5, 7), (800, 800)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import augment
    augment.lib()
    return torch.device("cuda:0")


def batches():
    from driving_dirty_amd.augment import CHUNK
    return [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def fp32_views(b, h, w):
    return synth.hash_uniform((b, 6, 3, h, w), synth.key_salt(f"augv{b}.{h}.{w}"))      # in [-0.5, 0.5]: both clamps are within reach


def u8_frames(b, h, w):
    return (synth.hash_uniform((b, 6, h, w, 3), synth.key_salt(f"augf{b}.{h}.{w}"), 0.0, 1.0) * 255).round().to(torch.uint8)


def mixed(b):
    """Per-sample mixed flags and colours: every second sample mirrored, every third with one view blanked, views with the identity
    colour beside views whose gain and bias push values past both clamps."""
    from driving_dirty_amd.augment import FLAG_MIRROR, flag_blank
    flags = torch.tensor([(FLAG_MIRROR if i % 2 == 0 else 0) | (flag_blank((i + 4) % 6) if i % 3 == 0 else 0) for i in range(b)])
    color = torch.tensor([[[1.0, 0.0], [3.0, 0.25], [0.625, -0.125], [1.0, 0.0], [2.5, -0.5], [1.0, 0.375]][(i + v) % 6]
                          for i in range(b) for v in range(6)]).reshape(b, 6, 2)
    return flags, color


def identity(b):
    return torch.zeros(b, dtype=torch.int64), torch.tensor([1.0, 0.0]).expand(b, 6, 2).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    return torch.equal(bits(got), bits(want))


def forms(x, dev):
    x = x.to(dev)
    return {"stacked": x, "tuple": tuple(x)}


def check_views(x_cpu, flags, color, dev):
    from driving_dirty_amd import augment
    want = ref.views(x_cpu, flags, color)
    for form, sample in forms(x_cpu, dev).items():
        got = augment.augment_views(sample, flags, color)
        assert got.is_contiguous() and got.data_ptr() % 16 == 0
        assert same_bits(got, want), (form, tuple(x_cpu.shape))
    return want


@pytest.mark.parametrize("make", [fp32_views, u8_frames], ids=["fp32", "uint8"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_views_shapes_with_mixed_flags(dev, make, h, w):
    check_views(make(3, h, w), *mixed(3), dev)


@pytest.mark.parametrize("make", [fp32_views, u8_frames], ids=["fp32", "uint8"])
@pytest.mark.parametrize("h,w", [(2, 3), (2, 4)], ids=["2x3-flat", "2x4-planes"])      # one shape per kernel of the launcher
@pytest.mark.parametrize("b", range(5), ids=["1", "CHUNK-1", "CHUNK", "CHUNK+1", "2CHUNK+1"])
def test_views_across_the_chunk_boundary(dev, make, b, h, w):
    b = batches()[b]
    check_views(make(b, h, w), *mixed(b), dev)


@pytest.mark.parametrize("make", [fp32_views, u8_frames], ids=["fp32", "uint8"])
def test_views_at_camera_size(dev, make):
    check_views(make(2, 256, 306), *mixed(2), dev)


@pytest.mark.parametrize("h,w", [(4, 5), (16, 22)])
def test_identity_is_the_plain_stack(dev, h, w):
    """Identity flags and colour: the fp32 views as they are; uint8 frames as ToTensor's /255 and the permute, bit for bit."""
    from driving_dirty_amd import augment
    x, f = fp32_views(3, h, w), u8_frames(3, h, w)
    flags, color = identity(3)
    assert same_bits(augment.augment_views(tuple(x.to(dev)), flags, color), torch.stack(tuple(x)))
    assert same_bits(augment.augment_views(tuple(f.to(dev)), flags, color), f.permute(0, 1, 4, 2, 3).float().div(255).contiguous())


def test_mirror_alone_is_a_pure_permutation(dev):
    from driving_dirty_amd import augment
    x = fp32_views(2, 4, 5)
    flags, color = identity(2)
    flags[0] = augment.FLAG_MIRROR
    got = augment.augment_views(x.to(dev), flags, color).cpu()
    assert torch.equal(bits(got[0]).flatten().sort().values, bits(x[0]).flatten().sort().values)
    assert same_bits(got[0], x[0][list(augment.MIRROR_VIEWS)].flip(-1).contiguous()) and same_bits(got[1], x[1])


@pytest.mark.parametrize("make", [fp32_views, u8_frames], ids=["fp32", "uint8"])
def test_jitter_is_mul_add_clamp_in_fp32(dev, make):
    """Against v.mul(g).add(b).clamp(0, 1) on the CPU, with gains and biases that push values past both clamps."""
    from driving_dirty_amd import augment
    x = make(2, 16, 22)
    v = x if x.dtype == torch.float32 else x.permute(0, 1, 4, 2, 3).float().div(255)
    color = torch.tensor([[3.0, 0.25], [0.3, 0.9], [1.7, -0.6], [1.0, 0.125], [0.999, 0.0], [4.0, -1.5]]).expand(2, 6, 2).contiguous()
    want = torch.stack([torch.stack([v[b, k].mul(color[b, k, 0]).add(color[b, k, 1]).clamp(0, 1) for k in range(6)]) for b in range(2)])
    got = augment.augment_views(x.to(dev), torch.zeros(2, dtype=torch.int64), color)
    assert same_bits(got, want)
    assert bool((want == 0).any()) and bool((want == 1).any()) and bool(((want > 0) & (want < 1)).any())


@pytest.mark.parametrize("make", [fp32_views, u8_frames], ids=["fp32", "uint8"])
def test_blanked_views_are_plus_zero(dev, make):
    from driving_dirty_amd import augment
    x = make(3, 4, 5)
    _, color = mixed(3)
    flags = torch.tensor([augment.flag_blank(0) | augment.flag_blank(5) | augment.FLAG_MIRROR, 0x3F << 8, augment.flag_blank(2)])
    got = augment.augment_views(x.to(dev), flags, color)
    assert same_bits(got, ref.views(x, flags, color))
    g = bits(got)
    for b, views in ((0, (0, 5)), (1, range(6)), (2, (2,))):
        for v in range(6):
            assert bool((g[b, v] == 0).all()) == (v in views), (b, v)


@pytest.mark.parametrize("make", [fp32_views, u8_frames], ids=["fp32", "uint8"])
def test_wide_image_of_a_mirrored_batch_is_the_blockwise_column_reversal(dev, make):
    """Pins M against the view order [0,1,2,5,4,3] independently of the reference: in the wide image the mirror reverses columns
    [0, 3W) as a block and columns [3W, 6W) likewise."""
    from driving_dirty_amd import augment, ops
    w = 22
    x = make(2, 16, w).to(dev)
    flags, color = identity(2)
    flags[:] = augment.FLAG_MIRROR
    wide = ops.wide_image(x).cpu()                                          # [B,H,6W,4]
    wide_m = ops.wide_image(augment.augment_views(x, flags, color)).cpu()
    want = torch.cat([wide[:, :, :3 * w].flip(2), wide[:, :, 3 * w:].flip(2)], dim=2)
    assert same_bits(wide_m, want)


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8], ids=["bool", "uint8"])
@pytest.mark.parametrize("h,w", MASK_SHAPES)
def test_masks(dev, dtype, h, w):
    from driving_dirty_amd import augment
    for b in ((3,) if h == 800 else (3, augment.CHUNK + 1)):      # across the chunk boundary at the small sizes
        u = synth.hash_uniform((b, h, w), synth.key_salt(f"augm{b}.{h}.{w}"), 0.0, 1.0)
        m = (u < 0.3) if dtype == torch.bool else (u * 255).round().to(torch.uint8)      # uint8: any byte, copied as it is
        flags = torch.tensor([i % 2 for i in range(b)]) | (0x3F << 8) * torch.tensor([i % 3 == 0 for i in range(b)])
        want = ref.masks(m, flags)
        for form, road in forms(m, dev).items():
            got = augment.augment_masks(road, flags)
            assert isinstance(got, tuple) and len(got) == b
            assert all(t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (h, w) for t in got)
            assert got[1].data_ptr() - got[0].data_ptr() == h * w, "views of ONE stacked tensor"
            assert torch.equal(torch.stack(got).cpu().view(torch.uint8), want.view(torch.uint8)), (form, b)
        if b == 3 and h >= 8:
            assert torch.equal(want[0], m[0]) and not torch.equal(want[1], m[1])      # sample 1 is the mirrored one


def test_refusals_reach_python_with_the_message(dev):
    from driving_dirty_amd import augment
    x = fp32_views(2, 2, 3).to(dev)
    _, color = identity(2)
    with pytest.raises(augment.HotpathError, match=r"flags\[1\]"):
        augment.augment_views(x, torch.tensor([0, 4]), color)
    with pytest.raises(ValueError):
        augment.augment_views(x, torch.tensor([0]), color)
    with pytest.raises(augment.HotpathError):
        augment.augment_views(x.cpu(), torch.tensor([0, 0]), color)
