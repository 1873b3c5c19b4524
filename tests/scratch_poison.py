"""Poisoned allocations: run a piece of the hot path with every unwritten byte of its floating-point buffers set to a chosen
value, so that a result which depends on memory nobody wrote shows up as a DIFFERENCE between two runs.

`poisoned(value)` replaces torch.empty, torch.empty_like, torch.empty_strided and torch.Tensor.new_empty for its duration: the
wrappers call the real function and fill the result with `value` rounded to the tensor's type (it becomes Inf where it
overflows: 1e5 in fp16).  Only floating-point tensors on `device_type` are filled.  INTEGER AND BOOL TENSORS ARE LEFT AS
ALLOCATED, on purpose: a poisoned integer could be used as an index, and provoking a fault is not what these tests do.  A float
reaches an address only through a conversion, and those conversions were read before the first poisoned run (blend taps, bin
searches, ray batching: all clamp or test the index).

The clean baseline is `poisoned(0.0)`: both legs of a comparison take the same allocation path, so the property under test --
the same bits whatever the scratch held -- is exact and needs no tolerance.

  value    what it exposes
  NaN      arithmetic leaks: anything that adds, multiplies or compares an unwritten element into a live result
  +Inf     the maxima that do not test for it (fmaxf drops a NaN operand, not an infinite one)
  -1e30    everything that guards only against non-finite values: finite, passes `amax < 3e38`, and as a tile or operand
           maximum sets a scale so small that the live adjoints underflow in the fp16 planes
  1e5      finite in fp32 but beyond fp16's range: becomes Inf in the f16x2 split and in 16-bit stored state

Caches cleared on entry and again on exit (what the project keeps across calls, so that it is re-allocated under the poison
and the poisoned copy does not outlive the block):
  * mlp._TN_WS        the weight-gradient GEMMs' reduction workspace, one torch.empty buffer per device
  * mlp._CHAIN_MEMO   filled chain descriptors per call site (they hold addresses, not buffers; dropped so that both legs
                      fill their descriptors afresh)
  * blend._uv_scale   small per-image-size constants on the device
  * of every engine passed as `engines`: the packed weights W / W^T / inv_norm (torch.empty) and every fragment-ordered copy,
    the pack-descriptor memos that hold their addresses, and the fragment-kind cache
"""
import contextlib
import math

import torch

POISONS = (math.nan, math.inf, -1e30, 1e5)
CLEAN = 0.0
_NAMES = ("empty", "empty_like", "empty_strided")


def rounded(value, dtype):
    """`value` as the tensor type holds it (Python float; Inf where it overflows)"""
    return float(torch.tensor(float(value), dtype=torch.float64).to(dtype))


def label(value):
    return "nan" if value != value else repr(float(value))


def drop_caches(engines=()):
    from neuraludf_amd import mlp
    from neuraludf_amd.models import blend
    mlp._TN_WS.clear()
    mlp._CHAIN_MEMO.clear()
    blend._uv_scale.clear()
    for eng in engines:
        for pl in eng._all():
            pl.invalidate()
            pl.W = pl.Wt = pl.inv_norm = None
            pl.__dict__.pop("_group_memo", None)
            pl.__dict__.pop("_pack_descs", None)
        eng._kinds_cache.clear()


@contextlib.contextmanager
def poisoned(value, device_type="cuda", engines=(), caches=True):
    """every floating-point torch.empty / empty_like / empty_strided / Tensor.new_empty result on `device_type` is filled with
    `value` inside the block.  caches = False leaves the project's caches alone (the host tests: no library needed)."""
    fills = {}

    def fill(t):
        if isinstance(t, torch.Tensor) and t.is_floating_point() and t.device.type == device_type and t.numel():
            v = fills.get(t.dtype)
            if v is None:
                v = fills[t.dtype] = rounded(value, t.dtype)
            with torch.no_grad():
                t.fill_(v)
        return t

    def wrap(real):
        def wrapper(*args, **kwargs):
            return fill(real(*args, **kwargs))
        wrapper.__wrapped__ = real
        wrapper.__name__ = getattr(real, "__name__", "empty")
        return wrapper

    real = {n: getattr(torch, n) for n in _NAMES}
    own_new_empty = "new_empty" in torch.Tensor.__dict__          # (normally inherited from torch._C.TensorBase)
    real_new_empty = torch.Tensor.new_empty
    if caches:
        drop_caches(engines)
    try:
        for n in _NAMES:
            setattr(torch, n, wrap(real[n]))
        torch.Tensor.new_empty = wrap(real_new_empty)
        yield
    finally:
        for n in _NAMES:
            setattr(torch, n, real[n])
        if own_new_empty:
            torch.Tensor.new_empty = real_new_empty
        else:
            del torch.Tensor.new_empty
        if caches:
            drop_caches(engines)
