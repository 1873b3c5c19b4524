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

`same_bits(a, b)` is the comparison for results that legitimately hold NaN or Inf (the mesh tools: a distance beyond `bound`, a
pixel nothing was drawn into, the mean edge length of an empty mesh): shape, dtype and bit pattern, where torch.equal would call
a NaN different from itself.

Caches cleared on entry and again on exit (what the project keeps across calls, so that it is re-allocated under the poison
and the poisoned copy does not outlive the block):
  * mlp._TN_WS        the weight-gradient GEMMs' reduction workspace, one torch.empty buffer per device
  * mlp._CHAIN_MEMO   filled chain descriptors per call site (they hold addresses, not buffers; dropped so that both legs
                      fill their descriptors afresh)
  * blend._uv_scale   small per-image-size constants on the device
  * patch_metric._win_cache   the Gaussian window of the patch loss per (patch size, device)
    (`module_caches()` lists these four; the mesh and evaluation modules keep no module-level cache, their indices and
    trees live in objects the tests build inside the block)
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


def same_bits(a, b):
    """shape, dtype and bit pattern: a floating tensor is compared as the integer type of its width, so that NaN equals the
    same NaN (mesh outputs legitimately hold NaN and Inf) and +0.0 differs from -0.0.  None equals None only."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        as_int = _INT_OF_WIDTH[a.element_size()]
        a, b = a.contiguous().view(as_int), b.contiguous().view(as_int)
    return torch.equal(a, b)


def same_bits_names(a, b):
    """names of the tensors of two {name: tensor} results that do not hold the same bits (the `differ` of
    test_gpu_scratch_poison._legs for results that may hold NaN)"""
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    return [k for k in a if not same_bits(a[k], b[k])]


_INT_OF_WIDTH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def module_caches():
    """every module-level cache of the package that holds a device tensor (or addresses of some) -> [(module, name)].  The
    mesh and evaluation modules keep none: what they cache lives in the objects the caller builds (MeshIndex, the winding
    tree, sparse grids), which a test builds inside the poisoned block."""
    from neuraludf_amd import mlp
    from neuraludf_amd.loss import patch_metric
    from neuraludf_amd.models import blend
    return [(mlp, "_TN_WS"), (mlp, "_CHAIN_MEMO"), (blend, "_uv_scale"), (patch_metric, "_win_cache")]


def drop_caches(engines=(), caches=None):
    """caches: the [(module, name)] to clear (default module_caches(); the host tests pass fakes)"""
    for mod, name in (module_caches() if caches is None else caches):
        getattr(mod, name).clear()
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
    `value` inside the block.  caches = False leaves the project's caches alone (the host tests: no library needed); a list
    of (module, name) is cleared in place of module_caches()."""
    fills = {}
    which = None if caches is True else caches

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
    if caches is not False:
        drop_caches(engines, which)
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
        if caches is not False:
            drop_caches(engines, which)
