"""GPU tests of the kernels of include/dd_ema.h (csrc/libdd_ema.so) against the fp64 reference and the derived bounds of
tests/_ema_ref.py.

The tensors of a table are slices of ONE allocation at 16-byte aligned offsets with live words between them, so a wrong prefix or a
wrong piece-to-tensor search shows as a neighbour's values, and a store outside a tensor as a changed word between two of them."""
import pytest
import torch

import _ema_ref as ref

pytestmark = pytest.mark.gpu

ALPHAS = (0.001, 0.1, 1.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from driving_dirty_amd import ema
    ema.lib()
    return torch.device("cuda:0")


TABLE_NAMES = ("n1", "n3", "n4", "n5", "nCHUNK-1", "nCHUNK", "nCHUNK+1", "n2CHUNK+7", "mixed", "split")


def table_counts(name):
    """Element counts of a table: the one-tensor tables around the vector width and the piece size, the mixed table (a wrong prefix
    shows as a neighbour's values), and one tensor more than a launch holds (the split launch)."""
    from driving_dirty_amd import ema
    c = ema.CHUNK
    return {"n1": (1,), "n3": (3,), "n4": (4,), "n5": (5,), "nCHUNK-1": (c - 1,), "nCHUNK": (c,), "nCHUNK+1": (c + 1,),
            "n2CHUNK+7": (2 * c + 7,), "mixed": (2 * c + 7, 1, 1, 1, 1, 1, c), "split": (5,) * (ema.TABLE_MAX + 1)}[name]


class Slab:
    """``values`` (fp32, CPU, the tensors one after the other) laid into one device allocation: each tensor at a 16-byte aligned
    offset, 4 to 7 live words behind it."""

    def __init__(self, dev, counts, values, salt):
        from driving_dirty_amd import synth
        self.offsets, at = [], 4
        for n in counts:
            self.offsets.append(at)
            at += (n + 3) // 4 * 4 + 4
        host = synth.hash_uniform((at,), synth.key_salt("ema_slab_" + salt), -3.0, 3.0)
        self.inside = torch.zeros(at, dtype=torch.bool)
        src = 0
        words, given = host.view(torch.int32), values.contiguous().view(torch.int32)      # moved as words: NaN payloads survive
        for o, n in zip(self.offsets, counts):
            words[o:o + n] = given[src:src + n]
            self.inside[o:o + n] = True
            src += n
        self.buf = host.to(dev)
        self.before = ref.bits(self.buf)
        self.views = [self.buf[o:o + n] for o, n in zip(self.offsets, counts)]

    def gather(self):
        """The tensors one after the other, on the CPU."""
        return self.buf.view(torch.int32).cpu()[self.inside].view(torch.float32)

    def assert_outside_untouched(self, what):
        now = ref.bits(self.buf)
        assert torch.equal(now[~self.inside], self.before[~self.inside]), f"{what}: a word between two tensors changed"

    def assert_unchanged(self, what):
        assert torch.equal(ref.bits(self.buf), self.before), f"{what}: changed"


def slabs(dev, counts, name, equal=False):
    e, w = ref.pair(sum(counts), name)
    if equal:
        w = e.clone()
    return Slab(dev, counts, e, "e"), Slab(dev, counts, w, "w"), e, w


def update(es, ws, alpha):
    from driving_dirty_amd import ema
    ema.launch("dd_ema_update_ptrs", *ema.pointer_tables(es.views, ws.views), float(alpha))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_update_is_within_the_one_step_bound_of_fp64(dev, name, alpha):
    counts = table_counts(name)
    es, ws, e, w = slabs(dev, counts, name)
    update(es, ws, alpha)
    torch.cuda.synchronize()
    ref.assert_within(es.gather(), ref.update(e, w, alpha), ref.one_step_bound(ref.magnitude(e, w)), f"{name} alpha {alpha}")
    es.assert_outside_untouched("the averages' allocation")
    ws.assert_unchanged("w")


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_alpha_zero_and_equal_operands_keep_every_bit(dev, name):
    counts = table_counts(name)
    es, ws, e, w = slabs(dev, counts, name)
    update(es, ws, 0.0)
    torch.cuda.synchronize()
    es.assert_unchanged("e at alpha 0")
    ws.assert_unchanged("w at alpha 0")
    es, ws, e, w = slabs(dev, counts, name, equal=True)
    es.buf[es.offsets[0]] = -0.0      # a signed zero on both sides: fmaf(alpha, +0, -0) would be +0
    ws.buf[ws.offsets[0]] = -0.0
    es.before, ws.before = ref.bits(es.buf), ref.bits(ws.buf)
    for alpha in ALPHAS:
        update(es, ws, alpha)
        torch.cuda.synchronize()
        es.assert_unchanged(f"e == w at alpha {alpha}")
        ws.assert_unchanged(f"w at alpha {alpha}")


@pytest.mark.parametrize("name", ("n5", "n2CHUNK+7", "mixed"))
def test_a_nonfinite_parameter_reaches_its_element_only(dev, name):
    counts = table_counts(name)
    total = sum(counts)
    e, w = ref.pair(total, name)
    at = sorted({0, total // 2, total - 1, min(total - 1, 4), max(0, total - 5)})[:5]
    for i, v in zip(at, (float("nan"), float("inf"), float("-inf"), float("nan"), float("inf"))):
        w[i] = v
    es, ws = Slab(dev, counts, e, "e"), Slab(dev, counts, w, "w")
    update(es, ws, 0.1)
    torch.cuda.synchronize()
    got = es.gather()
    hit = torch.zeros(total, dtype=torch.bool)
    hit[at] = True
    assert bool(torch.isfinite(got[~hit]).all()) and not bool(torch.isfinite(got[hit]).any())
    for i in at:
        assert (torch.isnan(got[i]) and torch.isnan(w[i])) or float(got[i]) == float(w[i]), (i, got[i], w[i])
    fine = ~hit
    ref.assert_within(got[fine], ref.update(e, w, 0.1)[fine], ref.one_step_bound(ref.magnitude(e, w))[fine], name)
    es.assert_outside_untouched("the averages' allocation")
    ws.assert_unchanged("w")


def test_fifty_updates_follow_the_recurrence(dev):
    """alpha 0.1, w takes a small random step each time; the fp64 recurrence is never rounded on the way."""
    from driving_dirty_amd import synth
    counts = table_counts("mixed")
    total = sum(counts)
    es, ws, e, w = slabs(dev, counts, "steps")
    want, m_run = e.double(), torch.zeros(total, dtype=torch.float64)
    for k in range(50):
        w = w + synth.hash_uniform((total,), synth.key_salt("ema_walk", k), -1e-2, 1e-2)
        ws = Slab(dev, counts, w, "w")
        m_run = torch.maximum(m_run, torch.maximum(es.gather().double().abs(), w.double().abs()))
        update(es, ws, 0.1)
        want = ref.update(want, w, 0.1)
    torch.cuda.synchronize()
    ref.assert_within(es.gather(), want, ref.k_step_bound(m_run, 0.1), "50 updates")
    es.assert_outside_untouched("the averages' allocation")


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_swap_exchanges_words_and_twice_is_the_identity(dev, name):
    from driving_dirty_amd import ema
    counts = table_counts(name)
    total = sum(counts)
    a, b = ref.word_patterns(total, "a" + name), ref.word_patterns(total, "b" + name).flip(0).contiguous()
    sa, sb = Slab(dev, counts, a, "a"), Slab(dev, counts, b, "b")
    table = ema.pointer_tables(sa.views, sb.views)
    ema.launch("dd_ema_swap_ptrs", *table)
    torch.cuda.synchronize()
    assert torch.equal(ref.bits(sa.gather()), ref.bits(b)) and torch.equal(ref.bits(sb.gather()), ref.bits(a))
    sa.assert_outside_untouched("a's allocation")
    sb.assert_outside_untouched("b's allocation")
    ema.launch("dd_ema_swap_ptrs", *table)
    torch.cuda.synchronize()
    sa.assert_unchanged("a after two calls")
    sb.assert_unchanged("b after two calls")
