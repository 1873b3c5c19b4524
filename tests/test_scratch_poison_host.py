"""The poison harness itself (tests/scratch_poison.py), on the CPU: what it intercepts, what it leaves alone, that it puts
the originals back, and that it detects the thing it is built for."""
import math

import pytest
import torch

import scratch_poison as SP


def _cpu(value):
    return SP.poisoned(value, device_type="cpu", caches=False)


def _all_are(t, value):
    if value != value:
        return bool(torch.isnan(t).all())
    return bool((t == value).all())


@pytest.mark.parametrize("value", SP.POISONS + (SP.CLEAN,), ids=SP.label)
def test_all_four_entry_points_are_intercepted(value):
    like = torch.zeros(3, 5)
    with _cpu(value):
        made = {
            "empty": torch.empty(7, 3),
            "empty(size tuple, kwargs)": torch.empty((2, 3), dtype=torch.float64, device="cpu", pin_memory=False),
            "empty(memory_format)": torch.empty((1, 2, 4, 4), memory_format=torch.channels_last),
            "empty_like": torch.empty_like(like),
            "empty_like(dtype)": torch.empty_like(like, dtype=torch.float64, memory_format=torch.preserve_format),
            "empty_strided": torch.empty_strided((4, 3), (1, 4)),
            "new_empty": like.new_empty((2, 9)),
            "new_empty(dtype)": like.new_empty(6, dtype=torch.float64),
        }
        out = torch.zeros(4)
        back = torch.empty(4, out=out)
    assert back is out and _all_are(out, value)
    for k, t in made.items():
        assert _all_are(t, value), (k, t)
    # the arguments went through
    assert made["empty(size tuple, kwargs)"].dtype == torch.float64
    assert made["empty(memory_format)"].is_contiguous(memory_format=torch.channels_last)
    assert made["empty_strided"].stride() == (1, 4)
    assert made["new_empty(dtype)"].dtype == torch.float64 and made["new_empty"].shape == (2, 9)


def test_integer_and_bool_tensors_are_left_as_allocated():
    """an integer may be an index: the harness never writes one.  Seen from outside: the real allocator hands a freed block
    back unchanged, so the marker written before is still there (a fill would have replaced it)."""
    calls = []
    real_fill = torch.Tensor.fill_
    try:
        torch.Tensor.fill_ = lambda self, *a, **k: (calls.append(self.dtype), real_fill(self, *a, **k))[1]
        with _cpu(math.nan):
            for dt in (torch.int32, torch.int64, torch.uint8, torch.int16, torch.bool):
                torch.empty(16, dtype=dt)
                torch.empty_like(torch.zeros(4, dtype=dt))
                torch.empty_strided((2, 2), (2, 1), dtype=dt)
                torch.zeros(3).new_empty(5, dtype=dt)
            torch.empty(4)
    finally:
        del torch.Tensor.fill_          # (inherited from the C base class again)
    assert torch.Tensor.fill_ is real_fill
    assert calls == [torch.float32], calls


def test_other_devices_are_left_alone():
    # (freshly allocated memory is whatever it is, so only the absence of the poison is asserted, through a value no
    # allocator produces by itself)
    with SP.poisoned(-1e30, device_type="cuda", caches=False):
        v = torch.empty(4096)
        w = torch.empty_like(v)
    assert not bool((v == -1e30).any()) and not bool((w == -1e30).any())


def test_16_bit_tensors_get_the_rounded_value():
    with _cpu(1e5):
        h = torch.empty(5, dtype=torch.float16)
        b = torch.empty(5, dtype=torch.bfloat16)
        f = torch.empty(5)
    assert bool(torch.isinf(h).all()) and bool((h > 0).all())          # beyond fp16's 65504
    assert _all_are(b, float(torch.tensor(1e5).bfloat16())) and float(b[0]) == 99840.0
    assert _all_are(f, 1e5)
    with _cpu(-1e30):
        h = torch.empty(5, dtype=torch.float16)
        b = torch.empty(5, dtype=torch.bfloat16)
    assert bool(torch.isinf(h).all()) and bool((h < 0).all())
    assert bool(torch.isfinite(b).all()) and abs(float(b[0]) / -1e30 - 1.0) < 2.0 ** -8
    with _cpu(math.nan):
        assert bool(torch.isnan(torch.empty(3, dtype=torch.float16)).all())
        assert bool(torch.isnan(torch.empty(3, dtype=torch.bfloat16)).all())
    assert SP.rounded(1e5, torch.float16) == math.inf and SP.rounded(1e5, torch.float32) == 1e5


def test_leaf_tensors_that_require_grad_are_filled_too():
    with _cpu(2.5):
        t = torch.empty(3, requires_grad=True)
    assert t.requires_grad and t.is_leaf and _all_are(t.detach(), 2.5)


def _originals():
    return (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)


def test_originals_are_back_after_a_normal_exit_and_after_an_exception():
    before = _originals()
    with _cpu(1.0):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.empty_strided is not before[2]
        assert torch.Tensor.new_empty is not before[3]
    assert _originals() == before

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with _cpu(math.inf):
            assert torch.empty is not before[0]
            raise Boom()
    assert _originals() == before
    # nested blocks unwind in order
    with _cpu(1.0):
        with _cpu(2.0):
            assert _all_are(torch.empty(3), 2.0)
        assert _all_are(torch.empty(3), 1.0)
    assert _originals() == before


def _sum_of_buffer(x, written):
    """the bug class the harness exists for: a scratch buffer of which only a prefix is written, all of it read"""
    buf = torch.empty(x.numel() + 5)
    buf[:written] = x[:written] if written <= x.numel() else torch.cat([x, torch.ones(written - x.numel())])
    return buf.sum()


def test_canary_a_partly_written_buffer_is_detected_a_fully_written_one_is_not():
    x = torch.arange(11, dtype=torch.float32)
    res = {}
    for v in (SP.CLEAN,) + SP.POISONS:
        with _cpu(v):
            res[SP.label(v)] = (_sum_of_buffer(x, 11), _sum_of_buffer(x, 16))
    clean_part, clean_full = res[SP.label(SP.CLEAN)]
    assert float(clean_part) == 55.0 and float(clean_full) == 60.0
    for v in SP.POISONS:
        part, full = res[SP.label(v)]
        # bit-equality, as the GPU tests compare: NaN differs from everything
        assert not torch.equal(part, clean_part), (SP.label(v), float(part))
        assert torch.equal(full, clean_full), (SP.label(v), float(full))
    assert not torch.equal(res[SP.label(-1e30)][0], res[SP.label(1e5)][0])


def test_same_bits_compares_shape_dtype_and_bit_pattern():
    nan = torch.tensor([1.0, math.nan, math.inf, -math.inf])
    assert SP.same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())          # NaN against the same NaN
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        assert SP.same_bits(nan.to(dt), nan.to(dt).clone()), dt
    assert not SP.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))                    # torch.equal calls these equal
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    other_nan = nan.clone().view(torch.int32)
    other_nan[1] ^= 1                                                                     # another payload: other bits
    assert not SP.same_bits(nan, other_nan.view(torch.float32))
    assert not SP.same_bits(torch.zeros(2, 3), torch.zeros(3, 2))
    assert not SP.same_bits(torch.zeros(3), torch.zeros(3, dtype=torch.float64))
    assert not SP.same_bits(torch.zeros(3), torch.zeros(3, dtype=torch.int32))
    assert not SP.same_bits(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0000002]))
    # integer, bool and empty tensors; views that are not contiguous; None
    assert SP.same_bits(torch.arange(5), torch.arange(5)) and not SP.same_bits(torch.arange(5), torch.arange(5) + 1)
    assert SP.same_bits(torch.tensor([True, False]), torch.tensor([True, False]))
    assert SP.same_bits(torch.zeros(0, 3), torch.zeros(0, 3)) and not SP.same_bits(torch.zeros(0, 3), torch.zeros(0, 2))
    m = torch.arange(12.0).reshape(3, 4)
    assert SP.same_bits(m.t(), m.t().contiguous())
    assert SP.same_bits(None, None) and not SP.same_bits(None, torch.zeros(1)) and not SP.same_bits(torch.zeros(1), None)


def test_same_bits_names_lists_the_tensors_that_differ():
    a = dict(x=torch.tensor([math.nan, 1.0]), y=torch.arange(3), z=torch.tensor([0.0]))
    b = dict(x=torch.tensor([math.nan, 1.0]), y=torch.arange(3), z=torch.tensor([-0.0]))
    assert SP.same_bits_names(a, b) == ["z"] and SP.same_bits_names(a, a) == []
    with pytest.raises(AssertionError):
        SP.same_bits_names(a, dict(x=a["x"]))


class _FakeModule:
    def __init__(self):
        self.cache = {"k": torch.ones(2)}
        self.other = {"kept": 1}


def test_the_listed_caches_are_dropped_on_entry_and_on_exit():
    fake, fake2 = _FakeModule(), _FakeModule()
    held = fake.cache
    with SP.poisoned(1.0, device_type="cpu", caches=[(fake, "cache"), (fake2, "cache")]):
        assert fake.cache is held and not held and not fake2.cache          # cleared in place, on entry
        fake.cache["made inside"] = torch.empty(3)
        assert _all_are(fake.cache["made inside"], 1.0)
    assert not fake.cache and fake.other == {"kept": 1} and fake2.other == {"kept": 1}      # the poisoned copy does not outlive the block
    with pytest.raises(KeyError):
        with SP.poisoned(1.0, device_type="cpu", caches=[(fake, "cache")]):
            fake.cache["x"] = 1
            raise KeyError("boom")
    assert not fake.cache
    # caches=False touches nothing
    fake.cache["stays"] = 1
    with _cpu(1.0):
        pass
    assert fake.cache == {"stays": 1}


def test_module_caches_lists_every_module_level_cache_that_holds_device_tensors():
    """the list drop_caches clears by default; every entry is a dict of its module (no library is loaded by the imports)"""
    got = {(m.__name__.split(".")[-1], n) for m, n in SP.module_caches()}
    assert got == {("mlp", "_TN_WS"), ("mlp", "_CHAIN_MEMO"), ("blend", "_uv_scale"), ("patch_metric", "_win_cache")}
    assert all(isinstance(getattr(m, n), dict) for m, n in SP.module_caches())
