"""ctypes binding of libnudf.so (declared in include/nudf.h).

The product path has NO fallback: if the library is missing or a call fails this raises.
torch is imported first so that the library's HIP runtime dependency (libamdhip64.so.7)
resolves to the copy already loaded by PyTorch-ROCm (one HIP runtime per process)."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must be loaded before libnudf, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NUDF_LIB") or os.path.join(_HERE, "libnudf.so")      # NUDF_LIB: A/B builds of the library
ABI_VERSION = 111         # NUDF_ABI_VERSION of the include/nudf.h these ctypes structures mirror

c_fp = C.c_void_p
i32 = C.c_int32
f32 = C.c_float


class NudfError(RuntimeError):
    pass


class GemmNN(C.Structure):
    _fields_ = [("A", c_fp), ("lda", i32), ("B", c_fp), ("ldb", i32), ("bias", c_fp),
                ("C1", c_fp), ("ldc1", i32), ("C2", c_fp), ("ldc2", i32), ("C3", c_fp), ("ldc3", i32),
                ("X1", c_fp), ("ldx1", i32), ("X2", c_fp), ("ldx2", i32),
                ("M", i32), ("N", i32), ("K", i32), ("epi", i32), ("iparam", i32), ("scale", f32), ("xscale", f32)]


class GemmTN(C.Structure):
    _fields_ = [("A1", c_fp), ("lda1", i32), ("na1", i32), ("B1", c_fp), ("ldb1", i32),
                ("A2", c_fp), ("lda2", i32), ("na2", i32), ("B2", c_fp), ("ldb2", i32),
                ("C", c_fp), ("ldc", i32), ("dbias", c_fp), ("M", i32), ("NA", i32), ("NB", i32),
                ("rows_per_block", i32), ("prec", i32)]


TN_MAX_PROBLEMS = 12


class GemmTNProblem(C.Structure):
    _fields_ = [("A1", c_fp), ("B1", c_fp), ("C", c_fp), ("dbias", c_fp), ("lda1", i32), ("ldb1", i32), ("ldc", i32),
                ("NA", i32), ("NB", i32), ("tile_start", i32), ("flags", i32)]


class GemmTNGroup(C.Structure):
    _fields_ = [("n_problems", i32), ("M", i32), ("rows_per_block", i32), ("total_tiles", i32), ("prec", i32),
                ("prob", GemmTNProblem * TN_MAX_PROBLEMS), ("workspace", c_fp), ("workspace_floats", C.c_int64),
                ("assign", i32), ("amax_a", c_fp), ("amax_b", c_fp)]


class BlendLoss(C.Structure):
    _fields_ = [("cb", c_fp), ("c", c_fp), ("pix", c_fp), ("gt", c_fp), ("err", c_fp), ("patch_mask", c_fp),
                ("weight_sum", c_fp), ("err_sorted", c_fp), ("order", c_fp), ("m", c_fp), ("err_masked", c_fp), ("sums", c_fp),
                ("sums_ws", c_fp), ("w_dev", c_fp), ("out", c_fp), ("d_total", c_fp), ("d_cb", c_fp), ("d_c", c_fp),
                ("d_pix", c_fp), ("d_err", c_fp), ("d_sums", c_fp), ("N", i32), ("sums_nblk", i32), ("n_rays", f32),
                ("trim_ratio", f32)]


class RayBatch(C.Structure):
    _fields_ = [("image", c_fp), ("mask", c_fp), ("intrinsics_inv", c_fp), ("pose", c_fp), ("pixels_x", c_fp),
                ("pixels_y", c_fp), ("N", i32), ("H", i32), ("W", i32), ("h_patch_size", i32), ("rays", c_fp),
                ("ndc_uv", c_fp), ("xyz_cam", c_fp), ("near", c_fp), ("far", c_fp), ("patch_color", c_fp),
                ("patch_mask", c_fp)]


class Composite(C.Structure):
    _fields_ = [("rays_o", c_fp), ("rays_d", c_fp), ("z", c_fp), ("udf", c_fp), ("grad", c_fp),
                ("color", c_fp), ("color_base", c_fp), ("bg_z", c_fp), ("bg_sigma", c_fp), ("bg_color", c_fp),
                ("scal", c_fp), ("sample_dist", c_fp), ("background_rgb", c_fp),
                ("N", i32), ("S", i32), ("n_out", i32), ("s_nominal", i32),
                ("has_anneal", i32), ("cos_anneal", f32), ("flip_saturation", f32),
                ("use_norm_grad", i32), ("sparse_scale", f32), ("alpha_type", i32),
                ("weights", c_fp), ("out_color", c_fp), ("out_color_base", c_fp), ("out_depth", c_fp),
                ("out_normals", c_fp), ("out_wsum", c_fp), ("out_wsum_all", c_fp), ("sums", c_fp), ("ws", c_fp),
                ("o_alpha", c_fp), ("o_alpha_plus", c_fp), ("o_alpha_minus", c_fp), ("o_vis_prob", c_fp),
                ("o_alpha_occ", c_fp), ("o_raw_occ", c_fp), ("o_true_cos", c_fp), ("o_grad_mag", c_fp),
                ("o_mid_z", c_fp), ("o_dists", c_fp), ("o_inside", c_fp), ("o_flip", c_fp), ("sched", c_fp),
                ("p_variance", c_fp), ("p_beta", c_fp), ("p_gamma", c_fp), ("beta_hi", f32), ("defer_sums", i32),
                ("scal_out", c_fp), ("recip_out", c_fp)]


class CompositeGrad(C.Structure):
    _fields_ = [("d_color", c_fp), ("d_color_base", c_fp), ("d_weights", c_fp), ("d_depth", c_fp),
                ("d_normals", c_fp), ("d_wsum", c_fp), ("d_wsum_all", c_fp), ("d_sums", c_fp),
                ("o_d_udf", c_fp), ("o_d_grad", c_fp), ("o_d_color", c_fp), ("o_d_color_base", c_fp),
                ("o_d_bg_sigma", c_fp), ("o_d_bg_color", c_fp), ("o_d_scal", c_fp), ("ws", c_fp), ("o_d_param", c_fp)]


class Upsample(C.Structure):
    _fields_ = [("rays_o", c_fp), ("rays_d", c_fp), ("z", c_fp), ("udf", c_fp), ("u", c_fp),
                ("sample_dist", c_fp), ("gamma_dev", c_fp),
                ("N", i32), ("M", i32), ("K", i32), ("mode", i32),
                ("inv_s", f32), ("beta", f32), ("gamma", f32),
                ("z_new", c_fp), ("pts_new", c_fp), ("dbg", c_fp),
                ("prev_z", c_fp), ("prev_udf", c_fp), ("add_z", c_fp), ("add_udf", c_fp),
                ("z_merged", c_fp), ("udf_merged", c_fp), ("merge_K", i32)]


class PixelBlend(C.Structure):
    _fields_ = [("pts", c_fp), ("logits", c_fp), ("nl", i32), ("proj", c_fp), ("imgs", c_fp),
                ("P", i32), ("V", i32), ("H", i32), ("W", i32), ("pix", c_fp), ("img_layout", i32)]


class PixelComposite(C.Structure):
    _fields_ = [("w", c_fp), ("pix", c_fp), ("pts", c_fp), ("bg_in", c_fp), ("bg_tail", c_fp),
                ("N", i32), ("S", i32), ("n_out", i32), ("out", c_fp)]


class PatchBlend(C.Structure):
    _fields_ = [("pts", c_fp), ("grad", c_fp), ("rays_d", c_fp), ("uv", c_fp), ("logits", c_fp), ("nl", i32),
                ("w", c_fp), ("ldw", i32), ("ref_cam", c_fp), ("src_cam", c_fp), ("imgs", c_fp),
                ("N", i32), ("S", i32), ("V", i32), ("H", i32), ("W", i32), ("hps", i32),
                ("patch_colors", c_fp), ("patch_mask", c_fp), ("img_layout", i32)]


class PatchWarp(C.Structure):
    _fields_ = [("pts", c_fp), ("normals", c_fp), ("uv", c_fp), ("ref_cam", c_fp), ("src_cam", c_fp), ("imgs", c_fp),
                ("N", i32), ("S", i32), ("V", i32), ("H", i32), ("W", i32), ("hps", i32), ("img_layout", i32),
                ("colors", c_fp), ("mask", c_fp)]


ADAM_MAX_TENSORS = 64
ADAM_MAX_GROUPS = 4


class AdamTensor(C.Structure):
    _fields_ = [("p", c_fp), ("g", c_fp), ("m", c_fp), ("v", c_fp), ("n", i32), ("group", i32), ("neg_step_size", f32), ("bc2_sqrt", f32)]


class AdamGroup(C.Structure):
    _fields_ = [("one_minus_beta1", f32), ("beta2", f32), ("one_minus_beta2", f32), ("eps", f32)]


class Adam(C.Structure):
    _fields_ = [("n_tensors", i32), ("pad_", i32), ("t", AdamTensor * ADAM_MAX_TENSORS),
                ("block_start", i32 * (ADAM_MAX_TENSORS + 1)), ("pad2_", i32), ("group", AdamGroup * ADAM_MAX_GROUPS),
                ("dyn", c_fp)]


CH_MAX_STEPS = 20
CH_STATE16 = 32     # NudfChainStep.layout: the step's stored-state arrays hold bf16
CH_P4_X1, CH_P4_C1 = 64, 128   # ReLU-family steps of the 16-bit mode: that array is bf16, 4-point packed
CH = dict(NONE=0, SOFTPLUS=1, MULSP=2, TANGENT=3, BWD=4, UDFHEAD=5, RELU=6, SIGMOIDN=7, MULMASK=8, ADDMASK=9, RELUADD=10,
          SEED=11)     # contracts nothing: forward + input-gradient sweep in one launch (include/nudf.h)
CH_INIT = dict(LOAD=0, POSENC=1, SEED=2)


class ChainStep(C.Structure):
    _fields_ = [("Bp", c_fp), ("bias", c_fp), ("X1", c_fp), ("X2", c_fp), ("C1", c_fp), ("C2", c_fp),
                ("r1_row", c_fp), ("r1_col", c_fp), ("K", i32), ("N", i32), ("epi", i32), ("iparam", i32),
                ("ldx1", i32), ("ldx2", i32), ("ldc1", i32), ("ldc2", i32), ("ldr1", i32), ("prec", i32), ("act_write", i32),
                ("act_col0", i32), ("pe_tail_col", i32), ("ld_pe", i32), ("pe_dst", c_fp), ("pe_tail_scale", f32),
                ("scale", f32), ("xscale", f32), ("layout", i32), ("row_w", c_fp), ("row_sums", c_fp), ("X3", c_fp),
                ("ldx3", i32)]


class Chain(C.Structure):
    _fields_ = [("P", i32), ("n_steps", i32), ("init", i32), ("k0", i32), ("x_div", i32), ("tile_rows", i32), ("lda0", i32),
                ("ldg0", i32), ("pe_L", i32), ("pe_jvp", i32), ("init_state16", i32), ("pe_in_scale", f32), ("seed_scale", f32),
                ("seed_xscale", f32), ("A0", c_fp), ("G0", c_fp), ("x", c_fp), ("v", c_fp), ("seed_sign", c_fp),
                ("seed_wrow", c_fp), ("dbg", c_fp), ("absmax_out", c_fp), ("tile_amax_in", c_fp),
                ("tile_amax_out", c_fp), ("tile_scale", C.c_int32), ("reserved0", C.c_int32), ("step", ChainStep * CH_MAX_STEPS)]


PACK_MAX_LAYERS = 16
PACK_MAX_FRAGS = 4


class PackFrag(C.Structure):
    _fields_ = [("dst", c_fp), ("transpose", i32), ("o0", i32), ("i0", i32), ("K", i32), ("N", i32), ("dtype", i32)]


class PackLayer(C.Structure):
    _fields_ = [("v", c_fp), ("g", c_fp), ("perm", c_fp), ("W", c_fp), ("Wt", c_fp), ("inv_norm", c_fp),
                ("out", i32), ("in_", i32), ("ldw", i32), ("ldwt", i32), ("nfrag", i32), ("row_start", i32),
                ("frag", PackFrag * PACK_MAX_FRAGS)]


class PackMulti(C.Structure):
    _fields_ = [("n_layers", i32), ("total_rows", i32), ("layer", PackLayer * PACK_MAX_LAYERS)]


class UnpackLayer(C.Structure):
    _fields_ = [("dW", c_fp), ("v", c_fp), ("g", c_fp), ("inv_norm", c_fp), ("perm", c_fp), ("dv", c_fp),
                ("dg", c_fp), ("db_in", c_fp), ("db_out", c_fp), ("out", i32), ("in_", i32), ("ldw", i32), ("row_start", i32)]


class UnpackMulti(C.Structure):
    _fields_ = [("n_layers", i32), ("total_rows", i32), ("layer", UnpackLayer * PACK_MAX_LAYERS)]


class MeshUDF(C.Structure):
    _fields_ = [("U", c_fp), ("G", c_fp), ("axes", c_fp), ("cell_case", c_fp), ("cell_ntri", c_fp), ("edge_flag", c_fp),
                ("cells", c_fp), ("face_off", c_fp), ("edge_scan", c_fp), ("faces", c_fp), ("edges", c_fp), ("verts", c_fp),
                ("n_cells", C.c_int64), ("n_edges", C.c_int64), ("n_faces", C.c_int64), ("N", i32), ("mean_thr", f32),
                ("max_thr", f32), ("pad_", i32)]


class MeshUDFSparse(C.Structure):
    _fields_ = [("U", c_fp), ("G", c_fp), ("axes", c_fp), ("blocks", c_fp), ("block_slot", c_fp), ("cell_case", c_fp),
                ("cell_ntri", c_fp), ("cells", c_fp), ("face_off", c_fp), ("edge_keys", c_fp), ("edges", c_fp),
                ("faces", c_fp), ("verts", c_fp), ("n_blocks", C.c_int64), ("n_cells", C.c_int64), ("n_edges", C.c_int64),
                ("n_faces", C.c_int64), ("N", i32), ("B", i32), ("nb", i32), ("mean_thr", f32), ("max_thr", f32),
                ("pad_", i32)]


class IsoSurface(C.Structure):
    _fields_ = [("F", c_fp), ("axes", c_fp), ("cell_case", c_fp), ("cell_ntri", c_fp), ("edge_flag", c_fp), ("cells", c_fp),
                ("face_off", c_fp), ("edge_scan", c_fp), ("faces", c_fp), ("edges", c_fp), ("verts", c_fp),
                ("n_cells", C.c_int64), ("n_edges", C.c_int64), ("n_faces", C.c_int64), ("N", i32), ("level", f32)]


class IsoSurfaceSparse(C.Structure):
    _fields_ = [("F", c_fp), ("axes", c_fp), ("blocks", c_fp), ("block_slot", c_fp), ("cell_case", c_fp), ("cell_ntri", c_fp),
                ("cells", c_fp), ("face_off", c_fp), ("edge_keys", c_fp), ("edges", c_fp), ("faces", c_fp), ("verts", c_fp),
                ("n_blocks", C.c_int64), ("n_cells", C.c_int64), ("n_edges", C.c_int64), ("n_faces", C.c_int64), ("N", i32),
                ("B", i32), ("nb", i32), ("level", f32)]


class PointCloud(C.Structure):
    _fields_ = [("verts", c_fp), ("faces", c_fp), ("tri_n", c_fp), ("tri_off", c_fp), ("out", c_fp),
                ("n_verts", C.c_int64), ("n_faces", C.c_int64), ("n_out", C.c_int64), ("out_base", C.c_int64),
                ("cap", C.c_int64), ("density", C.c_double),
                ("pts", c_fp), ("n", C.c_int64), ("origin", C.c_double * 3), ("cell", C.c_double), ("grid", i32 * 3),
                ("pad_", i32), ("keys", c_fp), ("cell_key", c_fp), ("cell_start", c_fp), ("cell_count", c_fp),
                ("n_cells", C.c_int64), ("hash_key", c_fp), ("hash_row", c_fp), ("hash_cap", C.c_int64),
                ("rank", c_fp), ("state", c_fp), ("undecided", c_fp), ("r2", C.c_double),
                ("query", c_fp), ("query_idx", c_fp), ("n_query", C.c_int64), ("bound", C.c_double),
                ("box_bound2", C.c_double), ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3),
                ("dist", c_fp), ("idx", c_fp),
                ("md_ref_n", c_fp), ("md_ref_off", c_fp), ("md_ref_key", c_fp), ("md_ref_face", c_fp),
                ("md_n_refs", C.c_int64), ("md_cell_face", c_fp), ("md_point", c_fp), ("md_bary", c_fp),
                ("md_ray_o", c_fp), ("md_ray_d", c_fp), ("md_t_min", C.c_double), ("md_t_max", C.c_double),
                ("md_ray_window", c_fp), ("md_mode", i32), ("md_pad_", i32), ("md_count", c_fp)]


class MeshTopo(C.Structure):
    _fields_ = [("faces", c_fp), ("he_key", c_fp), ("he_id", c_fp), ("edge_start", c_fp), ("edges", c_fp), ("he_edge", c_fp),
                ("edge_key", c_fp), ("nbr_off", c_fp), ("nbr", c_fp), ("bverts", c_fp), ("new_count", c_fp), ("new_off", c_fp),
                ("new_faces", c_fp), ("pos", c_fp), ("pos_out", c_fp), ("labels", c_fp), ("changed", c_fp), ("proj", c_fp),
                ("masks", c_fp), ("vis_count", c_fp), ("n_faces", C.c_int64), ("n_verts", C.c_int64), ("n_edges", C.c_int64),
                ("n_bverts", C.c_int64), ("n_new", C.c_int64), ("lam", C.c_double), ("max_loop", i32), ("n_views", i32),
                ("H", i32), ("W", i32), ("border", i32), ("pad_", i32),
                ("sp_key", c_fp), ("sp_cluster_key", c_fp), ("sp_vcluster", c_fp), ("sp_member_off", c_fp),
                ("sp_member", c_fp), ("sp_corner_off", c_fp), ("sp_corner", c_fp), ("sp_attr", c_fp), ("sp_rep", c_fp),
                ("sp_accepted", c_fp), ("sp_quadric", c_fp), ("sp_attr_out", c_fp), ("sp_faces", c_fp),
                ("sp_triple", c_fp), ("sp_degenerate", c_fp), ("n_clusters", C.c_int64), ("sp_grid", C.c_int64 * 3),
                ("sp_origin", C.c_double * 3), ("sp_cell", C.c_double), ("sp_lambda", C.c_double),
                ("sp_boundary_weight", C.c_double), ("sp_attr_width", i32), ("sp_placement", i32),
                ("sp_sd_mark", c_fp), ("sp_sd_edge_vertex", c_fp), ("sp_sd_marked", c_fp), ("sp_sd_ring_off", c_fp),
                ("sp_sd_ring", c_fp), ("sp_sd_vclass", c_fp), ("sp_sd_pos_out", c_fp), ("sp_sd_attr_out", c_fp),
                ("sp_sd_fcount", c_fp), ("sp_sd_foff", c_fp), ("sp_sd_faces_out", c_fp), ("sp_sd_parent", c_fp),
                ("sp_sd_n_ring", C.c_int64), ("sp_sd_n_border", C.c_int64), ("sp_sd_n_marked", C.c_int64),
                ("sp_sd_n_out", C.c_int64), ("sp_sd_max_edge", C.c_double), ("sp_sd_scheme", i32),
                ("sp_sd_mark_all", i32),
                ("sp_sd_hf_bedge", c_fp), ("sp_sd_hf_brank", c_fp), ("sp_sd_hf_link", c_fp), ("sp_sd_hf_rank_in", c_fp),
                ("sp_sd_hf_rank_out", c_fp), ("sp_sd_hf_loop_off", c_fp), ("sp_sd_hf_loop_vertex", c_fp),
                ("sp_sd_hf_loop_edge", c_fp), ("sp_sd_hf_closed", c_fp), ("sp_sd_hf_perimeter", c_fp),
                ("sp_sd_hf_status", c_fp), ("sp_sd_hf_n_border", C.c_int64), ("sp_sd_hf_n_loops", C.c_int64),
                ("sp_sd_hf_n_items", C.c_int64), ("sp_sd_hf_max_perimeter", C.c_double), ("sp_sd_hf_round", i32),
                ("sp_sd_hf_pad_", i32),
                ("sp_sd_hf_rm_corner_off", c_fp), ("sp_sd_hf_rm_corner", c_fp), ("sp_sd_hf_rm_vedge_off", c_fp),
                ("sp_sd_hf_rm_vedge", c_fp), ("sp_sd_hf_rm_status", c_fp), ("sp_sd_hf_rm_keep", c_fp),
                ("sp_sd_hf_rm_gone", c_fp), ("sp_sd_hf_rm_gain", c_fp), ("sp_sd_hf_rm_ab", c_fp),
                ("sp_sd_hf_rm_rank", c_fp), ("sp_sd_hf_rm_best_in", c_fp), ("sp_sd_hf_rm_best_out", c_fp),
                ("sp_sd_hf_rm_remap", c_fp), ("sp_sd_hf_rm_pos_out", c_fp), ("sp_sd_hf_rm_faces_out", c_fp),
                ("sp_sd_hf_rm_win", c_fp), ("sp_sd_hf_rm_n_vedge", C.c_int64), ("sp_sd_hf_rm_low", C.c_double),
                ("sp_sd_hf_rm_high", C.c_double), ("sp_sd_hf_rm_cos_border", C.c_double), ("sp_sd_hf_rm_mode", i32),
                ("sp_sd_hf_rm_pad_", i32)]


class MeshOrient(C.Structure):
    _fields_ = [("faces", c_fp), ("me_a", c_fp), ("me_b", c_fp), ("word", c_fp), ("changed", c_fp), ("nonorient", c_fp),
                ("comp_off", c_fp), ("comp_face", c_fp), ("comp_sum", c_fp), ("pos", c_fp), ("corner_off", c_fp),
                ("corner", c_fp), ("normals", c_fp), ("origin", C.c_double * 3), ("n_faces", C.c_int64),
                ("n_verts", C.c_int64), ("n_medges", C.c_int64), ("n_comps", C.c_int64),
                ("sm_nbr_off", c_fp), ("sm_nbr", c_fp), ("sm_fixed", c_fp), ("sm_pos_out", c_fp), ("sm_fnormal", c_fp),
                ("sm_fnormal_out", c_fp), ("sm_farea", c_fp), ("sm_fcentre", c_fp), ("sm_n_nbr", C.c_int64),
                ("sm_step", C.c_double), ("sm_inv2sc", C.c_double), ("sm_inv2ss", C.c_double), ("sm_weights", i32),
                ("sm_pad_", i32)]


class MeshRaster(C.Structure):
    _fields_ = [("pos", c_fp), ("faces", c_fp), ("proj", c_fp), ("scr", c_fp), ("npix", c_fp), ("entries", c_fp),
                ("zbuf", c_fp), ("depth", c_fp), ("face", c_fp), ("bary", c_fp), ("vis", c_fp), ("images", c_fp),
                ("normals", c_fp), ("cam_pos", c_fp), ("colors", c_fp), ("n_seen", c_fp), ("n_faces", C.c_int64),
                ("n_verts", C.c_int64), ("n_entries", C.c_int64), ("power", C.c_double), ("fill", f32 * 3),
                ("min_gap", f32), ("n_views", i32), ("H", i32), ("W", i32), ("image_f32", i32),
                ("tx_uv", c_fp), ("tx_cell_face", c_fp), ("tx_fallback", c_fp), ("tx_colors", c_fp), ("tx_n_seen", c_fp),
                ("tx_out", c_fp), ("tx_n_cells", C.c_int64), ("tx_class_off", C.c_int64 * 11),
                ("tx_class_cell", C.c_int64 * 11), ("tx_class_k", i32 * 10), ("tx_n_classes", i32), ("tx_W", i32),
                ("tx_H", i32), ("tx_background", f32 * 3)]


# float offsets of the device loss-weight vector (include/nudf.h NUDF_LW_*)
LW = dict(color_base=0, color=1, color_pixel=2, color_patch=3, igr=4, igr_ns=5, sparse=6, mask=7, color_sum=8)
LW_COUNT = 16

EPI = dict(NONE=0, SOFTPLUS=1, RELU=2, MUL=3, MULMASK=4, TANGENT=5, BWD=6, SIGMOID=7, UDFHEAD=8,
           SKIPSPLIT=9, RELU_DUAL=10, ADDMASK=11, MULSP=12)

# the status of a border loop after close_holes (include/nudf.h NUDF_HOLE_*)
HOLE = dict(FILLED=0, OPEN_CHAIN=1, TOO_MANY_EDGES=2, PERIMETER=3, NONFINITE=4, DUPLICATE=5, REPEATED_VERTEX=6)
HOLE_MAX_EDGES = 64
HOLE_FAN_CAP = 4096
# why an edge is not collapsed / flipped (include/nudf.h NUDF_REMESH_*, csrc/meshremesh.hip); 0: it is a candidate
REMESH = dict(CANDIDATE=0, COUNT=1, LONG=2, CLASS=3, BORDER=4, LINK=5, REACH=6, FOLD=7, DUPLICATE=8, SAME=9, EXISTS=10,
              GAIN=11)
# the kind of a reported pair of faces (include/nudf.h NUDF_ISECT_*, csrc/meshintersect.hip)
ISECT = dict(CROSSING=1, COPLANAR=2, UNCERTAIN=3)

# the ctypes mirror of every argument struct, under the header's name: NudfX is the class X above, without exception
MIRRORS = {"Nudf" + c.__name__: c for c in C.Structure.__subclasses__() if c.__module__ == __name__}

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
# every symbol include/nudf.h declares: name -> (restype, argtypes)   (checked by tests/test_abi.py)
SIGNATURES = {
    "nudf_version": (_I, []),
    "nudf_abi_struct": (_I, [_I, C.POINTER(C.c_char_p)]),
    "nudf_last_error": (C.c_char_p, []),
    "nudf_set_status_flag": (_I, [_P]),
    "nudf_status_flag": (_P, []),
    "nudf_gemm_nn": (_I, [C.POINTER(GemmNN), _P]),
    "nudf_gemm_tn": (_I, [C.POINTER(GemmTN), _P]),
    "nudf_gemm_tn_grouped": (_I, [C.POINTER(GemmTNGroup), _P]),
    "nudf_gemm_tn_grouped_workspace": (C.c_int64, [C.POINTER(GemmTNGroup)]),
    "nudf_gemm_tn_grouped_plan": (_I, [C.POINTER(GemmTNGroup), C.POINTER(C.c_int32), i32]),
    "nudf_gemm_tn_grouped_kernel": (_I, [C.POINTER(GemmTNGroup), C.c_char_p, i32, C.POINTER(C.c_int32)]),
    "nudf_set_tn_flags": (_I, [i32]),
    "nudf_set_tn_debug": (_I, [_P]),
    "nudf_composite_fwd": (_I, [C.POINTER(Composite), _P]),
    "nudf_composite_bwd": (_I, [C.POINTER(Composite), C.POINTER(CompositeGrad), _P]),
    "nudf_partial_sums": (_I, [_P, _I, _I, _P, _P]),
    "nudf_composite_colour_finish": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "nudf_upsample": (_I, [C.POINTER(Upsample), _P]),
    "nudf_merge": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "nudf_coarse_z": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "nudf_coarse_start": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "nudf_merge_points": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "nudf_outside_z": (_I, [_P, _I, _P, _I, _I, _I, _P, _P]),
    "nudf_ray_points": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "nudf_posenc": (_I, [_P, _I, _I, _P, _I, _I, _F, _I, _P, _I, _F, _P, _I, _F, _P]),
    "nudf_posenc_vjp": (_I, [_P, _I, _I, _I, _F, _I, _P, _I, _F, _P, _I, _F, _P, _P]),
    "nudf_copy_cols": (_I, [_P, _I, _I, _P, _I, _I, _I, _F, _P]),
    "nudf_udf_grad_seed": (_I, [_P, _P, _P, _I, _F, _I, _I, _F, _P, _I, _P]),
    "nudf_udf_head_bwd": (_I, [_P, _P, _P, _I, _I, _I, _F, _P, _I, _P]),
    "nudf_signed_colsum": (_I, [_P, _P, _I, _I, _I, _F, _P, _P]),
    "nudf_sigmoid_head_bwd": (_I, [_P, _P, _P, _I, _I, _P, _I, _I, _I, _P, _I, _P]),
    "nudf_weightnorm_pack": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _I, _P, _P]),
    "nudf_weightnorm_unpack_grad": (_I, [_P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "nudf_pixel_blend_fwd": (_I, [C.POINTER(PixelBlend), _P]),
    "nudf_pixel_blend_bwd": (_I, [C.POINTER(PixelBlend), _P, _P, _P]),
    "nudf_pixel_composite_fwd": (_I, [C.POINTER(PixelComposite), _P]),
    "nudf_pixel_composite_bwd": (_I, [C.POINTER(PixelComposite), _P, _P, _P, _P, _P, _P]),
    "nudf_patch_blend_fwd": (_I, [C.POINTER(PatchBlend), _P]),
    "nudf_patch_blend_bwd": (_I, [C.POINTER(PatchBlend), _P, _P, _P, _P]),
    "nudf_pixel_warp": (_I, [C.POINTER(PixelBlend), _P, _P, _P]),
    "nudf_patch_warp": (_I, [C.POINTER(PatchWarp), _P]),
    "nudf_ssim_patch": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "nudf_patch_metric": (_I, [_I] + [_P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "nudf_adam_step": (_I, [C.POINTER(Adam), _P]),
    "nudf_adam_chunk": (_I, []),
    "nudf_mlp_chain": (_I, [C.POINTER(Chain), _P]),
    "nudf_mlp_chain_plan": (_I, [C.POINTER(Chain), C.c_char_p, i32, C.POINTER(C.c_int32)]),
    "nudf_set_chain_t16": (_I, [_I]),
    "nudf_pack_frag": (_I, [_P, _I, _I, _I, _P, _P]),
    "nudf_weightnorm_pack_multi": (_I, [C.POINTER(PackMulti), _P]),
    "nudf_weightnorm_unpack_grad_multi": (_I, [C.POINTER(UnpackMulti), _P]),
    "nudf_scalars_fwd": (_I, [_P, _P, _P, _F, _P, _P, _P]),
    "nudf_scalars_bwd": (_I, [_P, _P, _P, _F, _P, _P, _P]),
    "nudf_l1_sum_fwd": (_I, [_P, _P, _I, _P, _P]),
    "nudf_l1_sum_bwd": (_I, [_P, _P, _I, _P, _P, _P]),
    "nudf_sums_errors_fwd": (_I, [_P, _F, _P, _P]),
    "nudf_sums_errors_bwd": (_I, [_P, _F, _P, _P, _P]),
    "nudf_color_loss_fwd": (_I, [_P, _P, _P, _I, _P, _I, _F, _F, _F, _P, _P, _P, _P]),
    "nudf_color_loss_bwd": (_I, [_P, _P, _P, _I, _P, _F, _F, _F, _P, _P, _P, _P, _P]),
    "nudf_gen_ray_batch": (_I, [C.POINTER(RayBatch), _P]),
    "nudf_color_loss_sums": (_I, [_P, _P, _P, _I, _P, _I, _P, _P]),
    "nudf_color_loss_finish": (_I, [_P, _I, _F, _F, _F, _P, _P, _P, _P]),
    "nudf_step_loss_fwd": (_I, [_P, _P, _P, _I, _P, _I, _P, _F, _F, _F, _F, _F, _F, _F, _P, _P, _P, _P, _I, _P]),
    "nudf_step_loss_bwd": (_I, [_P, _P, _P, _I, _P, _P, _F, _F, _F, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P]),
    "nudf_col0_seed4": (_I, [_P, _P, _F, _I, _I, _P, _P, _P]),
    # one struct and the stream: every entry point of these families
    **{"nudf_" + n: (_I, [C.POINTER(st), _P]) for st, names in (
        (BlendLoss, ("blend_loss_prepare", "blend_loss_fwd", "blend_loss_bwd")),
        (MeshUDF, ("meshudf_classify", "meshudf_emit", "meshudf_vertices")),
        (MeshUDFSparse, ("meshudf_sparse_classify", "meshudf_sparse_edges", "meshudf_sparse_emit",
                         "meshudf_sparse_vertices")),
        (IsoSurface, ("isosurface_classify", "isosurface_emit", "isosurface_vertices")),
        (IsoSurfaceSparse, ("isosurface_sparse_classify", "isosurface_sparse_edges", "isosurface_sparse_emit",
                            "isosurface_sparse_vertices")),
        (PointCloud, ("pc_tri_count", "pc_tri_emit", "pc_keys", "pc_cells", "pc_thin_round", "pc_nearest",
                      "pc_tribin_count", "pc_tribin_emit", "pc_closest", "pc_raycast", "pc_isect_count",
                      "pc_isect_emit", "pc_wn_faces", "pc_wn_nodes", "pc_winding")),
        (MeshTopo, ("meshtopo_edges", "meshtopo_fill_count", "meshtopo_fill_emit", "meshtopo_smooth", "meshtopo_cc_hook",
                    "meshtopo_cc_jump", "meshtopo_views", "meshsimplify_keys", "meshsimplify_place",
                    "meshsimplify_faces", "meshsubdiv_mark", "meshsubdiv_odd", "meshsubdiv_even", "meshsubdiv_count",
                    "meshsubdiv_emit", "meshhole_link", "meshhole_rank", "meshhole_count", "meshhole_triangulate",
                    "meshremesh_collapse_check", "meshremesh_vertex_min", "meshremesh_collapse_apply",
                    "meshremesh_flip_check", "meshremesh_flip_apply", "meshremesh_relax")),
        (MeshOrient, ("meshorient_hook", "meshorient_jump", "meshorient_check", "meshorient_outward", "meshorient_normals",
                      "meshsmooth_laplace", "meshsmooth_frames", "meshsmooth_normals", "meshsmooth_update")),
        (MeshRaster, ("meshraster_project", "meshraster_bounds", "meshraster_draw_small", "meshraster_draw_large",
                      "meshraster_resolve", "meshraster_visible", "meshraster_colour", "meshtexture_bake",
                      "meshtexture_shade")),
    ) for n in names},
}
SYMBOLS = list(SIGNATURES)

_lib = None


def _abi_mismatch(version, table):
    """why a library that reports this nudf_version() and this {struct name: sizeof} table cannot be driven through the
    mirrors above, or None when it can.  Pure: no library, no GPU."""
    if version != ABI_VERSION:
        return f"is ABI version {version}, this package binds {ABI_VERSION}"
    for name, size in table.items():
        if name not in MIRRORS:
            return f"has an argument struct {name} that this package does not bind"
        if size != C.sizeof(MIRRORS[name]):
            return f"has a {name} of {size} bytes, this package binds {C.sizeof(MIRRORS[name])}"
    missing = [name for name in MIRRORS if name not in table]
    if missing:
        return f"does not report {', '.join(missing)}, which this package binds"
    return None


def _abi_report(l):
    """(nudf_version(), {struct name: sizeof}) of a loaded library.  The version is read first: a library of another version
    is refused by that number, whether or not it has the table."""
    version, table, name, i = int(l.nudf_version()), {}, C.c_char_p(), 0
    if version == ABI_VERSION:
        while (size := l.nudf_abi_struct(i, C.byref(name))) >= 0:
            table[name.value.decode()], i = size, i + 1
    return version, table


def lib():
    """The loaded library; raises NudfError when it has not been built (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NudfError(
                f"{LIB_PATH} not found: build it with `python -m neuraludf_amd.build` "
                "(the NeuralUDF hot path has no CPU/PyTorch fallback)")
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise NudfError(f"cannot load {LIB_PATH}: {e}") from e
        try:
            why = _abi_mismatch(*_abi_report(l))
            if why is None:
                for name, (restype, argtypes) in SIGNATURES.items():
                    fn = getattr(l, name)
                    fn.restype, fn.argtypes = restype, argtypes
        except AttributeError as e:
            why = f"does not export every symbol of include/nudf.h ({e})"
        if why is not None:
            raise NudfError(f"{LIB_PATH} {why}: rebuild with `python -m neuraludf_amd.build --force`")
        _lib = l
    return _lib


# ---- the non-finite status word (include/nudf.h: nudf_set_status_flag) -----------------------------------------------
STATUS_NONFINITE_RENDER, STATUS_NONFINITE_SAMPLES, STATUS_NONFINITE_LOSS = 1, 2, 4
_STATUS_WORDS = {}        # device index -> the int32 tensor the kernels OR their bits into
_STATUS_BOUND = None      # device index the library currently points at


def bind_status(dev):
    """make the kernels' status word the one of `dev` (allocated and zeroed on first use).  One python compare per call
    once bound; the library keeps one pointer per process (one process per GPU)."""
    global _STATUS_BOUND
    if dev.type != "cuda":
        raise NudfError("libnudf kernels need device tensors (got a CPU tensor): run on an MI355X")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if _STATUS_BOUND == idx:
        return _STATUS_WORDS[idx]
    w = _STATUS_WORDS.get(idx)
    if w is None:
        w = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
        _STATUS_WORDS[idx] = w
    check(lib().nudf_set_status_flag(C.c_void_p(w.data_ptr())), "nudf_set_status_flag")
    _STATUS_BOUND = idx
    return w


def read_status(dev, clear=False):
    """the status bits seen so far on `dev` (synchronises: one 4-byte D2H copy)."""
    w = bind_status(dev)
    v = int(w.item())
    if clear and v:
        w.zero_()
    return v


def status_text(bits):
    names = [(STATUS_NONFINITE_SAMPLES, "non-finite new samples in the hierarchical re-sampling (nudf_upsample)"),
             (STATUS_NONFINITE_RENDER, "non-finite composited ray outputs or renderer scalars (nudf_composite_fwd)"),
             (STATUS_NONFINITE_LOSS, "non-finite loss (nudf_step_loss_fwd)")]
    return "; ".join(t for b, t in names if bits & b) or "finite"


def ptr(t):
    """raw device pointer of a contiguous fp32 / int32 / bf16 CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NudfError("libnudf kernels need device tensors (got a CPU tensor): run on an MI355X")
    if not t.is_contiguous():
        raise NudfError("libnudf kernels need contiguous tensors")
    return t.data_ptr()


HOST_FAST = os.environ.get("NUDF_HOST_FAST", "1") != "0"      # 0: the round-5 host path (A/B of the eager host cost)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """torch's current stream of the current device as a raw hipStream_t.  (torch.cuda.current_stream() builds a Stream object
    through three layers of Python argument checking: 12 us per call, 19 launches per forward pass -- the raw accessors of
    the same state cost 0.3 us.)"""
    if HOST_FAST and _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what=""):
    if rc != 0:
        msg = lib().nudf_last_error()
        raise NudfError(f"{what} failed (hipError {rc}): {msg.decode() if msg else ''}")


_FN = {}


def call(name, *args):
    """call an entry point on torch's current stream; struct arguments are passed by reference."""
    fn = _FN.get(name)
    if fn is None:
        fn = _FN[name] = getattr(lib(), name)
    rc = fn(*[C.byref(a) if isinstance(a, C.Structure) else a for a in args], stream())
    if rc != 0:
        check(rc, name)


def kernel_of(name, desc):
    """what the launcher would give `desc`, from its host-only report `name` (nudf_mlp_chain_plan / nudf_gemm_tn_grouped_kernel):
    (kernel instantiation, [grid.x, block.x, grid.x of the reduce launch or 0, 0]); ("", zeros) for an empty or a refused
    descriptor -- the launch itself raises the refusal."""
    buf, out = C.create_string_buffer(64), (C.c_int32 * 4)()
    getattr(lib(), name)(C.byref(desc), buf, len(buf), out)
    return buf.value.decode(), list(out)
