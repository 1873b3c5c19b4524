"""CPU: which kernel nudf_mlp_chain and nudf_gemm_tn_grouped give a descriptor, read from the launchers' own host-only reports
(nudf_mlp_chain_plan, nudf_gemm_tn_grouped_kernel: the check and the selection of the launcher, nothing launched) -- one case
per row of the two kernel tables and one per fallback.  The descriptors carry made-up 16-byte aligned addresses: the reports
dereference nothing a descriptor points to."""
import ctypes as C
import os

import pytest

SETTINGS = ("NUDF_CHAIN_ROWS", "NUDF_CHAIN_QUAD", "NUDF_CHAIN_T16", "NUDF_CHAIN_WIN2")
SETTINGS_SET = any(v in os.environ for v in SETTINGS)       # the chain selection depends on them: read once per process
A = 1 << 20


def _report(name, desc):
    from neuraludf_amd import _lib
    buf, out = C.create_string_buffer(64), (C.c_int32 * 4)()
    rc = getattr(_lib.lib(), name)(C.byref(desc), buf, len(buf), out)
    return rc, buf.value.decode(), list(out), (_lib.lib().nudf_last_error() or b"").decode()


# ---- chains ------------------------------------------------------------------------------------------------------------
def _chain(P, tile_rows=0):
    from neuraludf_amd import _lib
    c = _lib.Chain()
    c.P, c.init, c.k0, c.x_div, c.tile_rows = P, _lib.CH_INIT["LOAD"], 256, 1, tile_rows
    c.A0, c.lda0 = 4096, 256
    return c


def _step(c, epi, prec, K=256, N=256, **kw):
    from neuraludf_amd import _lib
    s = c.step[c.n_steps]
    c.n_steps += 1
    s.epi, s.K, s.N, s.prec, s.act_write, s.pe_tail_col, s.scale, s.xscale = _lib.CH[epi], K, N, prec, 1, -1, 1.0, 1.0
    s.Bp = 8192 if epi != "SEED" else None
    for k, v in kw.items():
        setattr(s, k, v)


X1 = dict(X1=A, ldx1=256)
X12 = dict(X1=A, ldx1=256, X2=2 * A, ldx2=256)


def _sweep(P, tile_rows, prec, *more):
    """two SOFTPLUS steps of `prec`, then the steps of `more` = (epi, prec, operands)"""
    c = _chain(P, tile_rows)
    _step(c, "SOFTPLUS", prec)
    _step(c, "SOFTPLUS", prec)
    for epi, pr, kw in more:
        _step(c, epi, pr, **kw)
    return c


def _colour_head(P, tile_rows, prec):
    """SIGMOIDN that composites inside its epilogue (row_w / row_sums)"""
    c = _chain(P, tile_rows)
    _step(c, "RELU", prec)
    _step(c, "SIGMOIDN", prec, N=4, iparam=3, act_write=0, row_w=8 * A, row_sums=9 * A)
    return c


def _seed_chain(tile_rows):
    """the valid forward + input-gradient chain of test_fused_sweeps_abi"""
    c = _chain(128, tile_rows)
    _step(c, "SOFTPLUS", 4)
    _step(c, "UDFHEAD", 0, N=1, act_write=0, C1=16384, C2=32768, ldc1=1, ldc2=1)
    _step(c, "SEED", 4, r1_col=4096)
    _step(c, "NONE", 4, act_write=0, C1=16384, ldc1=256)
    return c


BLK_C1 = dict(C1=4 * A, ldc1=256, layout=4)           # NUDF_CH_BLK_C1
# (id, descriptor, kernel, grid.x, block.x)
CHAIN_CASES = [
    ("split-8192", lambda: _sweep(8192, 0, 4), "mlp_chain_kernel<32, 2>", 256, 256),
    ("split-16384", lambda: _sweep(16384, 0, 4), "mlp_chain_kernel<32, 2>", 512, 256),
    ("split-16385", lambda: _sweep(16385, 0, 4), "mlp_chain_kernel<64, 2>", 257, 256),
    ("split-65536", lambda: _sweep(65536, 0, 4), "mlp_chain_kernel<64, 2>", 1024, 256),
    ("split-tile64-8192", lambda: _sweep(8192, 64, 4), "mlp_chain_kernel<64, 2>", 128, 256),
    ("split-tile32-65536", lambda: _sweep(65536, 32, 4), "mlp_chain_kernel<32, 2>", 2048, 256),
    ("fp32-65536", lambda: _sweep(65536, 0, 0), "mlp_chain_kernel<64, 0>", 1024, 256),
    ("fp32-8192", lambda: _sweep(8192, 0, 0), "mlp_chain_kernel<32, 0>", 256, 256),
    ("rows-class0", lambda: _sweep(65536, 128, 0), "mlp_chain_rows_kernel<0, 4>", 512, 256),
    ("rows-class1", lambda: _sweep(65536, 128, 0, ("MULSP", 0, X1)), "mlp_chain_rows_kernel<1, 4>", 512, 256),
    ("rows-class2", lambda: _sweep(65536, 128, 0, ("BWD", 0, X12)), "mlp_chain_rows_kernel<2, 2>", 512, 256),
    ("rows-split-falls-back", lambda: _sweep(65536, 128, 4), "mlp_chain_kernel<64, 2>", 1024, 256),
    ("rows-unaligned-falls-back", lambda: _sweep(65536, 128, 0, ("MULSP", 0, dict(X1=A + 4, ldx1=256))),
     "mlp_chain_kernel<64, 0>", 1024, 256),
    ("tq-class0", lambda: _sweep(1000, 66, 0), "mlp_chain_tq_kernel<0, 3>", 16, 256),
    ("tq-class1", lambda: _sweep(1000, 66, 0, ("MULSP", 0, X1)), "mlp_chain_tq_kernel<1, 3, true>", 16, 256),
    ("tq-class2", lambda: _sweep(1000, 66, 0, ("BWD", 0, X12)), "mlp_chain_tq_kernel<2>", 16, 256),
    ("tq-split-falls-back", lambda: _sweep(1000, 66, 4), "mlp_chain_kernel<32, 2>", 32, 256),
    ("blocked-class0", lambda: _sweep(1000, 0, 0, ("SOFTPLUS", 0, BLK_C1)), "mlp_chain_tq_kernel<0, 3>", 16, 256),
    ("blocked-class1", lambda: _sweep(1000, 0, 0, ("MULSP", 0, dict(X1, **BLK_C1))), "mlp_chain_tq_kernel<1, 3, true>", 16, 256),
    ("half-65536", lambda: _sweep(65536, 0, 1), "mlp_chain_kernel<64, 3>", 1024, 256),
    ("half-tangent", lambda: _sweep(65536, 0, 1, ("TANGENT", 1, X12)), "mlp_chain_kernel<64, 4>", 1024, 256),
    ("half-one-fp32-step", lambda: _sweep(65536, 0, 1, ("SOFTPLUS", 0, {})), "mlp_chain_kernel<64, 1>", 1024, 256),
    ("half-8192", lambda: _sweep(8192, 0, 1), "mlp_chain_kernel<32, 1>", 256, 256),
    ("roww-split", lambda: _colour_head(65536, 0, 4), "mlp_chain_kernel<64, 2>", 1024, 256),
    ("roww-half", lambda: _colour_head(65536, 0, 1), "mlp_chain_kernel<64, 1>", 1024, 256),
    ("seed", lambda: _seed_chain(0), "mlp_chain_kernel<32, 2>", 4, 256),
]


@pytest.mark.parametrize("make,kernel,grid,block", [c[1:] for c in CHAIN_CASES], ids=[c[0] for c in CHAIN_CASES])
def test_chain_kernel_selection(make, kernel, grid, block):
    if SETTINGS_SET:
        pytest.skip("a NUDF_CHAIN_* setting is in force: the selection below is the default one")
    rc, name, out, err = _report("nudf_mlp_chain_plan", make())
    assert rc == 0, err
    assert name == kernel
    assert out == [grid, block, 0, 0]


def test_chain_t16_switch_is_part_of_the_selection():
    if SETTINGS_SET:
        pytest.skip("a NUDF_CHAIN_* setting is in force")
    from neuraludf_amd import _lib
    lib = _lib.lib()
    old = lib.nudf_set_chain_t16(0)
    try:
        assert _report("nudf_mlp_chain_plan", _sweep(65536, 0, 1))[1] == "mlp_chain_kernel<64, 1>"
    finally:
        lib.nudf_set_chain_t16(old)
    assert _report("nudf_mlp_chain_plan", _sweep(65536, 0, 1))[1] == "mlp_chain_kernel<64, 3>"


@pytest.mark.parametrize("make,word", [
    (lambda: _sweep(1000, 64, 0, ("SOFTPLUS", 0, BLK_C1)), "blocked-layout"),
    (lambda: _colour_head(65536, 66, 4), "row_w"),
    (lambda: _seed_chain(66), "split-mode"),
    (lambda: _sweep(1000, 130, 0), "tile_rows"),           # the retired paired-tile kernel: refused, not given another kernel
], ids=["blocked-on-tile64", "roww-on-tq", "seed-on-tq", "retired-tile130"])
def test_chain_refusals_are_reported_without_a_launch(make, word):
    rc, name, out, err = _report("nudf_mlp_chain_plan", make())
    assert rc != 0 and word in err
    assert name == "" and out == [0, 0, 0, 0]


def test_empty_chain_reports_nothing():
    assert _report("nudf_mlp_chain_plan", _chain(0))[:3] == (0, "", [0, 0, 0, 0])
    c = _sweep(0, 0, 4)
    assert _report("nudf_mlp_chain_plan", c)[:3] == (0, "", [0, 0, 0, 0])


# ---- weight-gradient groups --------------------------------------------------------------------------------------------
UDF = [(256, 40)] + [(256, 256)] * 3 + [(217, 256)] + [(256, 256)] * 3 + [(256, 256), (1, 256)]      # 36 tiles of 128 x 128


def _group(shapes, prec, M=65536, flags=0, ld=None):
    from neuraludf_amd import _lib
    g = _lib.GemmTNGroup()
    g.n_problems, g.M, g.rows_per_block, g.prec = len(shapes), M, 0, prec
    for i, (NA, NB) in enumerate(shapes):
        q = g.prob[i]
        q.A1, q.B1, q.C = 4096, 8192, 16384 + i * (1 << 22)
        q.lda1, q.ldb1, q.ldc = ld or (NA + 3) // 4 * 4, ld or (NB + 3) // 4 * 4, NB
        q.NA, q.NB, q.flags = NA, NB, flags
    return g


def _with_workspace(g):
    from neuraludf_amd import _lib
    g.workspace, g.workspace_floats = 1 << 26, _lib.lib().nudf_gemm_tn_grouped_workspace(C.byref(g))
    return g


def _one_blocked(g):
    g.prob[0].flags = 4          # NUDF_TN_A_BLK
    return g


GROUP_CASES = [
    ("fp32", 0, lambda: _group(UDF, 0), "gemm_tn_group_kernel", 256),
    ("bf16x3", 0, lambda: _group(UDF, 3), "gemm_tn3_group_kernel", 256),
    ("bf16x3-no-split-image", 512, lambda: _group(UDF, 3), "gemm_tn_group_kernel", 256),
    ("bf16x3-retired-wide-flag", 1024, lambda: _group([(256, 256)], 3), "gemm_tn3_group_kernel", 256),
    ("bf16x3-one-blocked", 0, lambda: _one_blocked(_group(UDF, 3)), "gemm_tn_group_kernel", 256),
    ("f16x2", 0, lambda: _group(UDF, 4), "gemm_tn2_group_kernel", 256),
    ("bf16-packed", 0, lambda: _group(UDF, 2, flags=3, ld=256), "gemm_tn16_group_kernel", 256),
    ("bf16-no-pack16", 256, lambda: _group(UDF, 2, flags=3, ld=256), "gemm_tn_group_kernel", 256),
    ("bf16-fp32-operands", 0, lambda: _group(UDF, 2), "gemm_tn_group_kernel", 256),
]


@pytest.mark.parametrize("tn_flags,make,kernel,block", [c[1:] for c in GROUP_CASES], ids=[c[0] for c in GROUP_CASES])
def test_weight_gradient_kernel_selection(tn_flags, make, kernel, block):
    from neuraludf_amd import _lib
    lib = _lib.lib()
    prev = lib.nudf_set_tn_flags(tn_flags)
    try:
        g = make()
        rc, name, out, err = _report("nudf_gemm_tn_grouped_kernel", g)
        assert rc == 0, err
        assert name == kernel and out[1] == block and out[2:] == [0, 0]         # no workspace: no reduce launch
        assert out[0] == lib.nudf_gemm_tn_grouped_plan(C.byref(g), (C.c_int32 * 4)(), 1)
        rc, name, out2, err = _report("nudf_gemm_tn_grouped_kernel", _with_workspace(make()))
        assert rc == 0, err
        assert name == kernel and out2[:2] == out[:2]
        assert out2[2] == (36 if g.n_problems == len(UDF) else 4) * 17            # tn_reduce_kernel: 17 workgroups per tile
    finally:
        lib.nudf_set_tn_flags(prev)


def test_retired_wide_flag_changes_neither_kernel_nor_grid():
    """NUDF_TN_FLAGS bit 1024 once selected the wide bf16x3 kernel (deleted: profiles/r05_tn_wide.txt); it is masked off"""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    reports = []
    for flags in (0, 1024):
        prev = lib.nudf_set_tn_flags(flags)
        try:
            reports.append(_report("nudf_gemm_tn_grouped_kernel", _group([(256, 256)], 3))[:3])
        finally:
            lib.nudf_set_tn_flags(prev)
    assert reports[0][0] == 0 and reports[0][1] == "gemm_tn3_group_kernel" and reports[0][2][1] == 256
    assert reports[1] == reports[0]


def test_weight_gradient_refusals_are_reported_without_a_launch():
    rc, name, out, err = _report("nudf_gemm_tn_grouped_kernel", _group(UDF, 4, flags=1, ld=256))
    assert rc != 0 and "prec 4" in err and name == "" and out == [0, 0, 0, 0]
    g = _group(UDF, 0)
    g.assign = 1
    rc, name, out, err = _report("nudf_gemm_tn_grouped_kernel", g)
    assert rc != 0 and "assign" in err and name == "" and out == [0, 0, 0, 0]
    assert _report("nudf_gemm_tn_grouped_kernel", _group([], 0))[:3] == (0, "", [0, 0, 0, 0])
