"""CPU: the block selection of the sparse UDF extraction (neuraludf_amd/meshing.py udf_sparse_grid, which is host-side
torch and runs on the CPU too) against the numpy restatement (tests/meshudf_sparse_ref.py): geometry for exact and ragged
N, the threshold, coverage of every active cell of the dense grid for true distance fields, and sharpness."""
import numpy as np
import pytest
import torch

import meshudf_sparse_ref as S

CASES = [(fn, n, S.BOX) for fn in (S.sphere_udf, S.disc_udf) for n in (65, 96, 97)] + [(S.disc_udf, 96, S.NONCUBIC)]
LIP = 1.05       # true distance fields: |grad U| = 1; the 5 % margin covers fp32 rounding at the threshold


def test_block_geometry_exact_and_ragged():
    nb, lo, hi = S.block_geometry(65, 8)                       # 64 cells: 8 exact blocks
    assert nb == 8 and lo.tolist() == list(range(0, 64, 8)) and hi.tolist() == list(range(8, 65, 8))
    nb, lo, hi = S.block_geometry(96, 8)                       # 95 cells: the last block has 7
    assert nb == 12 and lo[-1] == 88 and hi[-1] == 95 and hi[-2] == 88
    nb, lo, hi = S.block_geometry(5, 8)                        # one ragged block
    assert nb == 1 and lo.tolist() == [0] and hi.tolist() == [4]
    assert S.coarse_indices(5, 8).tolist() == [0, 4] and S.coarse_indices(96, 4)[-2:].tolist() == [92, 95]
    for n, b in [(65, 4), (96, 4), (97, 8), (3, 4), (4096, 8)]:
        nb, lo, hi = S.block_geometry(n, b)
        assert lo[0] == 0 and hi[-1] == n - 1 and (hi[:-1] == lo[1:]).all() and ((hi - lo) <= b).all() and (hi > lo).all()


def test_threshold_is_rounded_up():
    from neuraludf_amd import meshing
    for (bmin, bmax), n, b, lip in [(S.BOX, 65, 8, 2.0), (S.BOX, 96, 4, 1.05), (S.NONCUBIC, 96, 8, 1.05),
                                    (S.BOX, 2049, 8, 1.05), (S.BOX, 4096, 4, 2.0), (S.NONCUBIC, 97, 4, 3.7)]:
        t = S.threshold(bmin, bmax, n, b, lip)
        got = meshing.sparse_threshold(bmin, bmax, n, b, lip)
        assert isinstance(got, np.float32) and got == t
        ha = [(bmax[a] - bmin[a]) / (n - 1) for a in range(3)]
        exact = 1.74 * max(ha) + lip * 0.5 * np.sqrt(sum((b * x) ** 2 for x in ha))
        assert float(got) >= exact and float(got) - exact <= np.spacing(np.float32(exact))


def test_ordering_keys():
    n = 4096
    assert int(S.edge_key(n - 1, n - 1, n - 1, 2, n)) == 3 * n ** 3 - 1 < 2 ** 63
    assert int(S.cell_key(n - 2, n - 2, n - 2, n)) == (n - 1) ** 3 - 1
    i, j, k = np.meshgrid(*[np.arange(4)] * 3, indexing="ij")
    assert (np.diff(S.cell_key(i, j, k, 5).reshape(-1)) == 1).all()           # x-major, k fastest
    assert (np.diff(S.edge_key(i, j, k, 0, 4).reshape(-1)) == 3).all()
    assert S.block_of_cell(94, 7, 8, 96, 8).item() == (11 * 12 + 0) * 12 + 1


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_selection_covers_every_active_cell_and_is_sharp(case, b):
    from neuraludf_amd import meshing
    fn, n, (bmin, bmax) = CASES[case]
    nb = S.block_geometry(n, b)[0]
    thr = S.threshold(bmin, bmax, n, b, LIP)
    blocks = S.select(S.coarse_values(fn, n, b, bmin, bmax), n, b, thr)
    U = S.grid_values(fn, n, bmin, bmax).numpy()
    assert S.uncovered_active_cells(U, blocks, b, bmin, bmax) == 0
    assert 0 < len(blocks) < nb ** 3                                           # not "everything"
    g = meshing.udf_sparse_grid(S.Field(fn), n, bmin, bmax, block=b, lipschitz=LIP, device="cpu")
    np.testing.assert_array_equal(g.blocks.numpy(), blocks)
    nodes = S.unique_nodes(blocks, n, b)
    assert (g.n_coarse, g.n_blocks, g.n_queried) == ((nb + 1) ** 3, len(blocks), len(nodes))
    slot = g.block_slot.numpy()
    assert slot.shape == (nb ** 3,) and (slot[blocks] == np.arange(len(blocks))).all() and (slot >= 0).sum() == len(blocks)
    ids = g.node_ids().numpy()
    assert ids.shape == (len(blocks), (b + 1) ** 3)
    np.testing.assert_array_equal(np.unique(ids[ids >= 0]), nodes)
    # the bricks hold the field at their nodes (+inf at the padding); copies of a shared node are the same bits
    np.testing.assert_array_equal(g.U.numpy()[ids >= 0], U.reshape(-1)[ids[ids >= 0]])
    assert np.isinf(g.U.numpy()[ids < 0]).all()


def test_nan_corner_never_selects():
    from neuraludf_amd import meshing

    def fn(p):
        u, g = S.sphere_udf(p)
        return torch.where(p[..., :1] > 0.4, torch.full_like(u, float("nan")), u), g
    n, b = 33, 4
    coarse = S.coarse_values(fn, n, b, *S.BOX)
    blocks = S.select(coarse, n, b, S.threshold(*S.BOX, n, b, LIP))
    g = meshing.udf_sparse_grid(S.Field(fn), n, *S.BOX, block=b, lipschitz=LIP, device="cpu")
    np.testing.assert_array_equal(g.blocks.numpy(), blocks)
    nb = S.block_geometry(n, b)[0]
    assert len(blocks) and ((blocks // (nb * nb)) * b <= 0.7 * (n - 1)).all()   # no block right of x = 0.4
