"""CPU: the host-side validation of nudf_mlp_chain refusing the step kind that fuses two sweeps into one launch
(NUDF_CH_SEED) out of place.  The refusal cases pass made-up addresses, which is safe only where a descriptor that slipped
through could not be launched: they run on machines without a GPU.  (The step limit and the enum values of include/nudf.h
against the ctypes mirror, and the descriptor inside the 4 KB kernel-argument segment: tests/test_abi.py.)"""
import ctypes as C

import pytest
import torch


def _chain(P=128):
    from neuraludf_amd import _lib
    c = _lib.Chain()
    c.P, c.init, c.k0, c.x_div, c.tile_rows = P, _lib.CH_INIT["LOAD"], 256, 1, 0
    c.A0, c.lda0 = 4096, 256                      # fake 16-byte aligned addresses: a refused descriptor is never dereferenced
    return c


def _step(s, epi, K=256, N=256, prec=4, **kw):
    from neuraludf_amd import _lib
    s.epi, s.K, s.N, s.prec, s.act_write, s.pe_tail_col, s.scale, s.xscale = _lib.CH[epi], K, N, prec, 1, -1, 1.0, 1.0
    s.Bp = 8192 if epi != "SEED" else None
    for k, v in kw.items():
        setattr(s, k, v)


@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: host-only check")
def test_seed_step_is_refused_out_of_place():
    from neuraludf_amd import _lib
    lib = _lib.lib()

    def refused(c):
        return lib.nudf_mlp_chain(C.byref(c), None) != 0

    # SEED without a head in front of it / as the first / as the last step
    c = _chain()
    _step(c.step[0], "SOFTPLUS")
    _step(c.step[1], "SEED", r1_col=4096, C1=16384, ldc1=256)
    _step(c.step[2], "NONE", act_write=0, C1=16384, ldc1=256)
    c.n_steps = 3
    assert refused(c) and b"SEED" in lib.nudf_last_error()
    c = _chain()
    _step(c.step[0], "SEED", r1_col=4096)
    _step(c.step[1], "NONE", act_write=0, C1=16384, ldc1=256)
    c.n_steps = 2
    assert refused(c)
    c = _chain()
    _step(c.step[0], "SOFTPLUS")
    _step(c.step[1], "UDFHEAD", N=1, prec=0, act_write=0, C1=16384, C2=32768, ldc1=1, ldc2=1)
    _step(c.step[2], "SEED", r1_col=4096)
    c.n_steps = 3
    assert refused(c)
    # ... in a chain that is not in a split mode (fp32 steps), and on the transposed-product tile
    c = _chain()
    _step(c.step[0], "SOFTPLUS", prec=0)
    _step(c.step[1], "UDFHEAD", N=1, prec=0, act_write=0, C1=16384, C2=32768, ldc1=1, ldc2=1)
    _step(c.step[2], "SEED", r1_col=4096)
    _step(c.step[3], "NONE", prec=0, act_write=0, C1=16384, ldc1=256)
    c.n_steps = 4
    assert refused(c) and b"split-mode" in lib.nudf_last_error()
    for s in (c.step[0], c.step[3]):
        s.prec = 4
    c.tile_rows = 66
    assert refused(c) and b"split-mode" in lib.nudf_last_error()
    # more steps than the descriptor holds
    c = _chain()
    c.n_steps = _lib.CH_MAX_STEPS + 1
    assert refused(c)
