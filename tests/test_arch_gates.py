"""CPU: what the engines' dispatch decides for the network shapes of tests/arch_cases.py, and the limits mlp.py repeats from
the kernels' sources (the GPU side is tests/test_gpu_arch_sweep.py)."""
import os
import re

import pytest

import arch_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encoding_limit_matches_the_kernel_source():
    """UDFEngine._gradient_guard refuses before the first launch what nudf_posenc_vjp would refuse behind the sweeps: the two
    bounds are one number."""
    from neuraludf_amd import mlp
    src = open(os.path.join(ROOT, "neuraludf_amd", "csrc", "rays_embed.hip")).read()
    assert int(re.search(r"#define PV_MAXE (\d+)", src).group(1)) == mlp.PV_MAXE
    assert "D * (2 * L + 1) > PV_MAXE" in src          # (the refusal of nudf_posenc_vjp the guard anticipates)


@pytest.mark.parametrize("name", list(A.ALL) + list(A.REFUSED))
def test_gate_sends_the_entry_where_the_table_says(name):
    entry = A.ALL[name] if name in A.ALL else A.REFUSED[name][0]
    assert A.module(name)[0].engine()._chain_ok() == entry["chain"]


@pytest.mark.parametrize("name,blocked", [("u100", False), ("u250", False), ("u_f100", True), ("u96", True)])
def test_blocked_state_only_where_the_seed_width_is_a_multiple_of_16(name, blocked):
    """fp32 mode above 16 384 points: the transposed-product kernels' seed reads k8(width) columns of X[L] and their stores leave
    the columns behind the width unwritten -- 100- and 250-wide networks keep row-major state (whose pads are cleared)."""
    from neuraludf_amd import mlp
    eng = A.module(name)[0].engine()
    old = mlp.PRECISION
    try:
        mlp.set_precision("fp32")
        assert mlp._state_blocked(20000) and not mlp._state_blocked(349)
        assert eng._blocked(20000) == blocked
        assert not eng._blocked(349)
    finally:
        mlp.set_precision(old)
