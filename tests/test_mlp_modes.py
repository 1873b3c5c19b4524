"""The decisions of neuraludf_amd/mlp.py that depend on the operand mode, pinned as literals (no GPU): operand dtype per sweep,
precision of the weight-gradient GEMMs, the head fragment, and the fragment copies every layer of the three engines packs.
The expected values were recorded by running this sweep on the commit before the engines got their common base class."""
import itertools

import pytest
import torch

from neuraludf_amd import mlp
from neuraludf_amd.models import fields

# per record: (_sweep_dtype of fwd / grad / bwd, _tn_prec(), _head_kind(), fragment kinds per layer of the UDF engine (one skip
# layer), of the colour engine (base + view, its pack order) and of the NeRF engine (pts with one skip, views, feature, alpha, rgb))
FP32 = (('f32', 'f32', 'f32'), 0, 'fwd_head0',
 (('fwd', 'bwd'), ('fwd', 'bwd'), ('fwd', 'bwd', 'bwd_hid:25'), ('fwd', 'bwd'), ('fwd_head0', 'fwd_feat', 'bwd_feat')),
 (('fwd', 'bwd_hid:64'), ('fwd', 'bwd'), ('fwd', 'bwd'), ('fwd', 'bwd'), ('fwd', 'bwd'), ('fwd', 'bwd')),
 (('fwd',), ('fwd', 'bwd'), ('fwd_in:0:64', 'fwd_in:64:84', 'bwd_hid:64'), ('fwd', 'bwd'), ('fwd', 'bwd_hid:64'), ('fwd', 'bwd'), ('fwd',),
  ('fwd', 'bwd')))
BF16X3 = (('bf16x3', 'bf16x3', 'bf16x3'), 3, 'fwd_head0',
 (('fwd@bf16x3', 'bwd@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3', 'bwd_hid:25@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'),
  ('fwd_head0', 'fwd_feat@bf16x3', 'bwd_feat@bf16x3')),
 (('fwd@bf16x3', 'bwd_hid:64@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'),
  ('fwd@bf16x3', 'bwd@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3')),
 (('fwd@bf16x3',), ('fwd@bf16x3', 'bwd@bf16x3'), ('fwd_in:0:64@bf16x3', 'fwd_in:64:84@bf16x3', 'bwd_hid:64@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'),
  ('fwd@bf16x3', 'bwd_hid:64@bf16x3'), ('fwd@bf16x3', 'bwd@bf16x3'), ('fwd@bf16x3',), ('fwd@bf16x3', 'bwd@bf16x3')))
F16X2 = (('f16x2', 'f16x2', 'f16x2'), 3, 'fwd_head0',
 (('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2', 'bwd_hid:25@f16x2'), ('fwd@f16x2', 'bwd@f16x2'),
  ('fwd_head0', 'fwd_feat@f16x2', 'bwd_feat@f16x2')),
 (('fwd@f16x2', 'bwd_hid:64@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'),
  ('fwd@f16x2', 'bwd@f16x2')),
 (('fwd@f16x2',), ('fwd@f16x2', 'bwd@f16x2'), ('fwd_in:0:64@f16x2', 'fwd_in:64:84@f16x2', 'bwd_hid:64@f16x2'), ('fwd@f16x2', 'bwd@f16x2'),
  ('fwd@f16x2', 'bwd_hid:64@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2',), ('fwd@f16x2', 'bwd@f16x2')))
F16X2_BWD_BF16X3 = (('f16x2', 'f16x2', 'bf16x3'), 3, 'fwd_head0',
 (('fwd@f16x2', 'bwd@f16x2', 'fwd@bf16x3', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@f16x2', 'fwd@bf16x3', 'bwd@bf16x3'),
  ('fwd@f16x2', 'bwd@f16x2', 'bwd_hid:25@bf16x3', 'fwd@bf16x3'), ('fwd@f16x2', 'bwd@f16x2', 'fwd@bf16x3', 'bwd@bf16x3'),
  ('fwd_head0', 'fwd_feat@f16x2', 'bwd_feat@bf16x3')),
 (('fwd@f16x2', 'bwd_hid:64@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'),
  ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3')),
 (('fwd@f16x2',), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd_in:0:64@f16x2', 'fwd_in:64:84@f16x2', 'bwd_hid:64@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'),
  ('fwd@f16x2', 'bwd_hid:64@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2',), ('fwd@f16x2', 'bwd@bf16x3')))
F16X2_GRAD_BF16X3 = (('f16x2', 'bf16x3', 'f16x2'), 3, 'fwd_head0',
 (('fwd@f16x2', 'bwd@bf16x3', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@bf16x3', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@bf16x3', 'bwd_hid:25@f16x2'),
  ('fwd@f16x2', 'bwd@bf16x3', 'bwd@f16x2'), ('fwd_head0', 'fwd_feat@f16x2', 'bwd_feat@f16x2')),
 (('fwd@f16x2', 'bwd_hid:64@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2', 'bwd@f16x2'),
  ('fwd@f16x2', 'bwd@f16x2')),
 (('fwd@f16x2',), ('fwd@f16x2', 'bwd@f16x2'), ('fwd_in:0:64@f16x2', 'fwd_in:64:84@f16x2', 'bwd_hid:64@f16x2'), ('fwd@f16x2', 'bwd@f16x2'),
  ('fwd@f16x2', 'bwd_hid:64@f16x2'), ('fwd@f16x2', 'bwd@f16x2'), ('fwd@f16x2',), ('fwd@f16x2', 'bwd@f16x2')))
F16X2_FWD_ONLY = (('f16x2', 'bf16x3', 'bf16x3'), 3, 'fwd_head0',
 (('fwd@f16x2', 'bwd@bf16x3', 'fwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3', 'fwd@bf16x3'),
  ('fwd@f16x2', 'bwd@bf16x3', 'bwd_hid:25@bf16x3', 'fwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3', 'fwd@bf16x3'),
  ('fwd_head0', 'fwd_feat@f16x2', 'bwd_feat@bf16x3')),
 (('fwd@f16x2', 'bwd_hid:64@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'),
  ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3')),
 (('fwd@f16x2',), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd_in:0:64@f16x2', 'fwd_in:64:84@f16x2', 'bwd_hid:64@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'),
  ('fwd@f16x2', 'bwd_hid:64@bf16x3'), ('fwd@f16x2', 'bwd@bf16x3'), ('fwd@f16x2',), ('fwd@f16x2', 'bwd@bf16x3')))
MIXED16 = (('f16', 'f16', 'bf16'), 2, 'fwd_head0@f16',
 (('fwd@f16', 'bwd@f16', 'fwd@bf16', 'bwd@bf16'), ('fwd@f16', 'bwd@f16', 'fwd@bf16', 'bwd@bf16'),
  ('fwd@f16', 'bwd@f16', 'bwd_hid:25@bf16', 'fwd@bf16'), ('fwd@f16', 'bwd@f16', 'fwd@bf16', 'bwd@bf16'),
  ('fwd_head0@f16', 'fwd_feat@f16', 'bwd_feat@bf16')),
 (('fwd@f16', 'bwd_hid:64@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16', 'bwd@bf16'),
  ('fwd@f16', 'bwd@bf16')),
 (('fwd@f16',), ('fwd@f16', 'bwd@bf16'), ('fwd_in:0:64@f16', 'fwd_in:64:84@f16', 'bwd_hid:64@bf16'), ('fwd@f16', 'bwd@bf16'),
  ('fwd@f16', 'bwd_hid:64@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16',), ('fwd@f16', 'bwd@bf16')))
MIXED16_HEAD32 = (('f16', 'f16', 'bf16'), 2, 'fwd_head0',
 (('fwd@f16', 'bwd@f16', 'fwd@bf16', 'bwd@bf16'), ('fwd@f16', 'bwd@f16', 'fwd@bf16', 'bwd@bf16'),
  ('fwd@f16', 'bwd@f16', 'bwd_hid:25@bf16', 'fwd@bf16'), ('fwd@f16', 'bwd@f16', 'fwd@bf16', 'bwd@bf16'),
  ('fwd_head0', 'fwd_feat@f16', 'bwd_feat@bf16')),
 (('fwd@f16', 'bwd_hid:64@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16', 'bwd@bf16'),
  ('fwd@f16', 'bwd@bf16')),
 (('fwd@f16',), ('fwd@f16', 'bwd@bf16'), ('fwd_in:0:64@f16', 'fwd_in:64:84@f16', 'bwd_hid:64@bf16'), ('fwd@f16', 'bwd@bf16'),
  ('fwd@f16', 'bwd_hid:64@bf16'), ('fwd@f16', 'bwd@bf16'), ('fwd@f16',), ('fwd@f16', 'bwd@bf16')))

# (PRECISION, FWD_F16X2, BWD_F16X2, HEAD16) -> record
EXPECTED = {
    ('fp32', '0', True, True): FP32,
    ('fp32', '0', True, False): FP32,
    ('fp32', '0', False, True): FP32,
    ('fp32', '0', False, False): FP32,
    ('fp32', '1', True, True): FP32,
    ('fp32', '1', True, False): FP32,
    ('fp32', '1', False, True): FP32,
    ('fp32', '1', False, False): FP32,
    ('fp32', 'grad', True, True): FP32,
    ('fp32', 'grad', True, False): FP32,
    ('fp32', 'grad', False, True): FP32,
    ('fp32', 'grad', False, False): FP32,
    ('bf16x3', '0', True, True): BF16X3,
    ('bf16x3', '0', True, False): BF16X3,
    ('bf16x3', '0', False, True): BF16X3,
    ('bf16x3', '0', False, False): BF16X3,
    ('bf16x3', '1', True, True): F16X2,
    ('bf16x3', '1', True, False): F16X2,
    ('bf16x3', '1', False, True): F16X2_BWD_BF16X3,
    ('bf16x3', '1', False, False): F16X2_BWD_BF16X3,
    ('bf16x3', 'grad', True, True): F16X2_GRAD_BF16X3,
    ('bf16x3', 'grad', True, False): F16X2_GRAD_BF16X3,
    ('bf16x3', 'grad', False, True): F16X2_FWD_ONLY,
    ('bf16x3', 'grad', False, False): F16X2_FWD_ONLY,
    ('mixed16', '0', True, True): MIXED16,
    ('mixed16', '0', True, False): MIXED16_HEAD32,
    ('mixed16', '0', False, True): MIXED16,
    ('mixed16', '0', False, False): MIXED16_HEAD32,
    ('mixed16', '1', True, True): MIXED16,
    ('mixed16', '1', True, False): MIXED16_HEAD32,
    ('mixed16', '1', False, True): MIXED16,
    ('mixed16', '1', False, False): MIXED16_HEAD32,
    ('mixed16', 'grad', True, True): MIXED16,
    ('mixed16', 'grad', True, False): MIXED16_HEAD32,
    ('mixed16', 'grad', False, True): MIXED16,
    ('mixed16', 'grad', False, False): MIXED16_HEAD32,
}


@pytest.fixture(scope="module")
def engines():
    torch.manual_seed(0)
    udf = fields.UDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=4, skip_in=(2,), multires=6, scale=1.0)
    col = fields.ResidualRenderingNetwork(d_feature=64, mode="no_normal", d_in=6, d_out=3, d_hidden=64, n_layers=2,
                                          multires_view=4, blending_cand_views=4)
    nerf = fields.NeRF(D=4, W=64, d_in=4, d_in_view=3, multires=10, multires_view=4, skips=[1], use_viewdirs=True)
    return mlp.UDFEngine(udf), mlp.ColorEngine(col), mlp.NerfEngine(nerf)


def test_every_setting_is_listed():
    assert set(EXPECTED) == set(itertools.product(("fp32", "bf16x3", "mixed16"), ("0", "1", "grad"), (True, False), (True, False)))


@pytest.mark.parametrize("setting", sorted(EXPECTED, key=repr), ids=lambda s: "-".join(map(str, s)))
def test_mode_decisions(engines, setting):
    old_head = mlp.HEAD16          # (tests/conftest.py restores the other three)
    mlp.PRECISION, mlp.FWD_F16X2, mlp.BWD_F16X2, mlp.HEAD16 = setting
    try:
        got = (tuple(mlp._sweep_dtype(s) for s in ("fwd", "grad", "bwd")), mlp._tn_prec(), mlp._head_kind()) + \
            tuple(e._frag_kinds() for e in engines)
    finally:
        mlp.HEAD16 = old_head
    assert got == EXPECTED[setting]

