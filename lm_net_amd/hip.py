"""ctypes binding of ``liblmnet_hip.so`` (the C-ABI declared in ``include/lmnet_hip.h``).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic op of the
LM-Net path is a hand-written gfx950 kernel behind this boundary.  There is NO fallback: if the
shared library is missing the import raises, and calling any op with a non-device tensor raises.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.abspath(os.environ["LMNET_HIP_LIB"]) if os.environ.get("LMNET_HIP_LIB") else os.path.join(_HERE, "liblmnet_hip.so")   # (override: A/B runs against another build)

# ---- constants mirrored from include/lmnet_hip.h
SRC_GELU, SRC_DROP, SRC_LN, SRC_UP2 = 1, 2, 4, 8
EP_LINEAR, EP_AFFINE_ACT, EP_DGELU, EP_BN_BWD1, EP_BN_BWD2, EP_SE_BWD, EP_LN_BWD = 0, 1, 2, 3, 4, 5, 6
ACT_NONE, ACT_HSWISH, ACT_GELU = 0, 1, 2
STATS_NONE, STATS_SUM_SQ, STATS_EP = 0, 1, 2
F32, BF16 = 0, 1            # matrix-core operand type of the dense contractions (LMN_F32 / LMN_BF16)
_MMA = [F32]                # ... of the pass in flight (engine.begin_pass)
ABI_VERSION = 15


class SrcT(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("scale", C.c_void_p), ("C", C.c_int32), ("cstride", C.c_int32),
                ("flags", C.c_int32), ("drop_seed", C.c_uint32), ("drop_p", C.c_float), ("rp_w", C.c_int32),
                ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_stats", C.c_void_p), ("ln_eps", C.c_float), ("_pad0", C.c_int32)]


class BnFin(C.Structure):
    _fields_ = [("mode", C.c_int32), ("nrep", C.c_int32), ("count", C.c_float), ("eps", C.c_float), ("momentum", C.c_float),
                ("batch_stats", C.c_int32), ("sums", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("about", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("A", C.c_void_p), ("shift", C.c_void_p),
                ("rmean", C.c_void_p), ("rvar", C.c_void_p), ("Ain", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p)]


FIN_BN, FIN_BN_BWD = 1, 2


class ConvChain(C.Structure):
    """Mirror of lmn_conv_chain_t: a second 1x1 conv applied to the output tile of a 1x1 conv_fwd call."""
    _fields_ = [("wpack", C.c_void_p), ("bias", C.c_void_p), ("shift", C.c_void_p), ("aux", C.c_void_p), ("out", C.c_void_p),
                ("stats", C.c_void_p), ("Cout", C.c_int32), ("out_cstride", C.c_int32), ("out_rp_w", C.c_int32),
                ("aux_cstride", C.c_int32), ("aux_rp_w", C.c_int32), ("epilogue", C.c_int32), ("stats_mode", C.c_int32),
                ("stats_rep", C.c_int32), ("stats_snap", C.c_int32)]


class ConvArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
                ("ksize", C.c_int32), ("stride", C.c_int32), ("transposed", C.c_int32), ("nsrc", C.c_int32),
                ("Cout", C.c_int32), ("src", SrcT * 3), ("wpack", C.c_void_p), ("bias", C.c_void_p),
                ("p0", C.c_void_p), ("p1", C.c_void_p), ("p2", C.c_void_p), ("p3", C.c_void_p), ("p4", C.c_void_p),
                ("aux", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p), ("stats", C.c_void_p),
                ("aux_cstride", C.c_int32), ("res_cstride", C.c_int32), ("out_cstride", C.c_int32),
                ("epilogue", C.c_int32), ("act", C.c_int32), ("stats_mode", C.c_int32),
                ("drop_p", C.c_float), ("drop_seed", C.c_uint32), ("seed_ctr", C.c_void_p), ("bias2", C.c_void_p),
                ("stats_rep", C.c_int32), ("mma_dtype", C.c_int32), ("act_dtype", C.c_int32), ("out_rp_w", C.c_int32),
                ("p5", C.c_void_p), ("p6", C.c_void_p), ("fin", BnFin), ("stats_snap", C.c_int32), ("aux_rp_w", C.c_int32),
                ("chain", ConvChain)]


class WgradArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
                ("ksize", C.c_int32), ("stride", C.c_int32), ("nsrc", C.c_int32), ("Cout", C.c_int32),
                ("src", SrcT * 3), ("dy", C.c_void_p), ("dy_cstride", C.c_int32), ("dy_flags", C.c_int32),
                ("dy_seed", C.c_uint32), ("dy_p", C.c_float), ("dW", C.c_void_p), ("db", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_floats", C.c_int64), ("seed_ctr", C.c_void_p),
                ("dW_src", C.c_void_p * 3), ("db2", C.c_void_p), ("mma_dtype", C.c_int32), ("act_dtype", C.c_int32),
                ("defer_reduce", C.c_int32), ("dy_rp_w", C.c_int32)]


class DwPre(C.Structure):
    """Mirror of lmn_dw_pre_t (z-path of ReparamConv: the depthwise kernels form x1 = Hardswish(A z + shift) themselves)."""
    _fields_ = [("A", C.c_void_p), ("shift", C.c_void_p), ("fin", BnFin)]


def _fill_fin(f, fin):
    f.mode, f.nrep, f.count = fin["mode"], fin["nrep"], float(fin["count"])
    f.eps, f.momentum, f.batch_stats = float(fin.get("eps", 0.0)), float(fin.get("momentum", 0.0)), int(fin.get("batch_stats", 1))
    for k in ("sums", "gamma", "beta", "about", "mean", "rstd", "A", "shift", "rmean", "rvar", "Ain", "dgamma", "dbeta"):
        t = fin.get(k)
        setattr(f, k, t.data_ptr() if t is not None else None)


def _dw_pre(zpre):
    """zpre: None | dict(A=, shift=) | dict(fin=dict(...)) (lmn_dw_stats only: A / shift are formed from the batch sums)"""
    if zpre is None:
        return None
    p = DwPre()
    if zpre.get("fin") is not None:
        _fill_fin(p.fin, zpre["fin"])
    else:
        p.A, p.shift = _p(zpre["A"]).value, _p(zpre["shift"]).value
    return C.byref(p)


class SeFuse(C.Structure):
    """Mirror of lmn_se_fuse_t."""
    _fields_ = [("ticket", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("s", C.c_void_p), ("hidden", C.c_void_p), ("inv_hw", C.c_float), ("R", C.c_int32)]


class SeBwd(C.Structure):
    """Mirror of lmn_se_bwd_t."""
    _fields_ = [("ds", C.c_void_p), ("w1", C.c_void_p), ("w2", C.c_void_p), ("hidden", C.c_void_p), ("dvec", C.c_void_p),
                ("inv_hw", C.c_float), ("R", C.c_int32)]


def _se_fuse(se):
    """se: None | dict(ticket=[B] zeroed fp32/int32 tensor, fc1w, fc1b, fc2w, fc2b, s, hidden, inv_hw)"""
    if se is None:
        return None
    f = SeFuse()
    f.ticket = se["ticket"].data_ptr()
    f.w1, f.b1, f.w2, f.b2 = (_p(se[k]).value for k in ("fc1w", "fc1b", "fc2w", "fc2b"))
    f.s, f.hidden = _p(se["s"]).value, _p(se["hidden"]).value
    f.inv_hw, f.R = float(se["inv_hw"]), se["fc1w"].shape[0]
    return C.byref(f)


class ReduceJob(C.Structure):
    """Mirror of lmn_reduce_job_t (the deferred second stage of a weight gradient's K-split reduction)."""
    _fields_ = [("partial", C.c_void_p), ("first_block", C.c_int64),
                ("nblk", C.c_int32), ("per", C.c_int32), ("gy", C.c_int32), ("nsets_n", C.c_int32),
                ("taps", C.c_int32), ("NMT", C.c_int32), ("NNT", C.c_int32), ("nsrc", C.c_int32),
                ("Cout", C.c_int32), ("Cin", C.c_int32), ("NMTT", C.c_int32), ("NNTT", C.c_int32),
                ("srcC", C.c_int32 * 3), ("ntile_off", C.c_int32 * 3), ("cbase", C.c_int32 * 3),
                ("ksl", C.c_int32), ("blocks_per_set", C.c_int32), ("_pad", C.c_int32),
                ("dW", C.c_void_p), ("dW_src", C.c_void_p * 3), ("db", C.c_void_p), ("db2", C.c_void_p)]


class PackJob(C.Structure):
    """Mirror of lmn_pack_job_t."""
    _fields_ = [("w", C.c_void_p), ("wpack", C.c_void_p), ("total", C.c_int64), ("first_block", C.c_int64),
                ("ksize", C.c_int32), ("Cout", C.c_int32), ("Cin", C.c_int32), ("nsrc", C.c_int32),
                ("c", C.c_int32 * 3), ("transposed", C.c_int32), ("row_off", C.c_int32), ("rows", C.c_int32),
                ("dtype", C.c_int32), ("_pad", C.c_int32)]


class AugParam(C.Structure):
    """Mirror of lmn_aug_param_t: one sample's parameters of lmn_augment_u8 (lm_net_amd.data.DeviceAugment)."""
    _fields_ = [("M", C.c_double * 6), ("iM", C.c_double * 6), ("cj", C.c_double * 4), ("y0", C.c_int32), ("x0", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("apply_ssr", C.c_int32), ("apply_cj", C.c_int32), ("flips", C.c_int32),
                ("order", C.c_int32 * 4), ("_pad", C.c_int32)]


class OneOfParam(C.Structure):
    """Mirror of lmn_oneof_param_t (include/lmnet_oneof.h): one sample's member of the OneOf block and its drawn values."""
    _fields_ = [("op", C.c_int32), ("k", C.c_int32), ("perm", C.c_int32 * 3), ("unit", C.c_int32), ("hole", C.c_int32),
                ("radius", C.c_int32), ("slot", C.c_int32), ("_pad", C.c_int32), ("tab_off", C.c_int64), ("v", C.c_double * 3)]


# LMN_ONEOF_* of include/lmnet_oneof.h
ONEOF_OPS = {"none": 0, "to_gray": 1, "grid_distortion": 2, "elastic": 3, "clahe": 4, "hsv": 5, "channel_shuffle": 6,
             "grid_dropout": 7, "rgb_shift": 8, "gaussian_blur": 9}
ONEOF_MAX_RADIUS = 4096
# offsets into the int32 array of 8-bit LAB tables (LMN_LAB_* of include/lmnet_oneof.h; built by lm_net_amd.data.lab_tables)
LAB_GAMMA, LAB_CBRT, LAB_FY, LAB_DA, LAB_DB, LAB_FWD, LAB_INV, LAB_INVGAMMA, LAB_TABLE_INTS = 0, 256, 3328, 3584, 3840, 4096, 4105, 4128, 20513


class LossParam(C.Structure):
    """Mirror of lmn_loss_param_t (include/lmnet_loss.h): the scalar parameters of lmn_segloss_ex_fwd / _bwd."""
    _fields_ = [("ignore_index", C.c_int64), ("has_ignore", C.c_int32), ("label_smoothing", C.c_float), ("smooth", C.c_float),
                ("ce_scale", C.c_float), ("dice_scale", C.c_float), ("focal_scale", C.c_float), ("focal_gamma", C.c_float),
                ("focal_alpha", C.c_float), ("_pad", C.c_int32 * 6)]


def loss_sums_floats(n_classes):
    """LMN_LOSS_SUMS_FLOATS of include/lmnet_loss.h: floats of the `sums` workspace of segloss_ex_fwd."""
    return 4 + 3 * int(n_classes)


def loss_coef_floats(n_classes):
    """LMN_LOSS_COEF_FLOATS of include/lmnet_loss.h: floats of the `coef` workspace shared by segloss_ex_fwd / _bwd."""
    return 4 + 2 * int(n_classes)


class SigParam(C.Structure):
    """Mirror of lmn_sig_param_t (include/lmnet_sigmoid.h): the scalar parameters of lmn_sigloss_fwd / _bwd."""
    _fields_ = [("smooth", C.c_float), ("bce_scale", C.c_float), ("dice_scale", C.c_float), ("focal_scale", C.c_float),
                ("focal_gamma", C.c_float), ("focal_alpha", C.c_float), ("target_kind", C.c_int32), ("_pad", C.c_int32 * 9)]


SIG_T_U8, SIG_T_I64 = 0, 1      # LMN_SIG_T_* of include/lmnet_sigmoid.h


def sig_sums_words(n_classes):
    """LMN_SIG_SUMS_WORDS of include/lmnet_sigmoid.h: 4-byte words of the `sums` workspace of sigloss_fwd."""
    return 6 * int(n_classes)


def sig_coef_floats(n_classes):
    """LMN_SIG_COEF_FLOATS of include/lmnet_sigmoid.h: floats of the `coef` workspace shared by sigloss_fwd / _bwd."""
    return 4 * int(n_classes)


class PostParam(C.Structure):
    """Mirror of lmn_post_param_t: the cleaning parameters of lmn_post_clean (lm_net_amd.post.DevicePostprocess)."""
    _fields_ = [("connectivity", C.c_int32), ("hole_limit", C.c_int32), ("class_mask", C.c_uint64), ("keep_largest_mask", C.c_uint64),
                ("min_area", C.c_int32 * 64)]

class OptimParam(C.Structure):
    """Mirror of lmn_optim_param_t (include/optim/lmnet_optim.h): the scalar parameters of lmn_optim_prepare / lmn_adamw_step_ex."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float), ("max_norm", C.c_float), ("ema_decay", C.c_float),
                ("flags", C.c_int32), ("n_groups", C.c_int32), ("_pad", C.c_int32 * 7)]


class TileParam(C.Structure):
    """Mirror of lmn_tile_param_t (include/tiles/lmnet_tiles.h): the geometry shared by lmn_tile_gather / lmn_tile_blend."""
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("tile_h", C.c_int32),
                ("tile_w", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32), ("pad", C.c_int32), ("n_flip", C.c_int32),
                ("flip", C.c_int32 * 4), ("average", C.c_int32), ("_pad", C.c_int32 * 9)]


# LMN_TILE_* of include/tiles/lmnet_tiles.h
TILE_MIN, TILE_MAX, TILE_MAX_LEN, TILE_MAX_CLASSES, TILE_MAX_FLIPS, TILE_PARAM_BYTES = 32, 1024, 8192, 64, 4, 96
TILE_PADS = {"zero": 0, "reflect": 1}
TILE_FLIPS = {"h": 1, "v": 2, "hv": 3}
TILE_AVERAGES = {"logits": 0, "softmax": 1, "sigmoid": 2}


def tile_axis(L, t, s):
    """One axis of the tile geometry (include/tiles/lmnet_tiles.h) -> (virtual length, padding before, tiles)."""
    V = max(int(L), int(t))
    return V, (V - int(L)) // 2, -(-(V - int(t)) // max(int(s), 1)) + 1      # (a stride below 1 is the library's to reject)


# LMN_CURVE_* of include/curves/lmnet_curves.h
CURVE_MAX_EDGES, CURVE_MAX_CLASSES = 1024, 64
CURVE_RAW, CURVE_SOFTMAX = 0, 1
CURVE_PLANES, CURVE_LABELS = 0, 1
CURVE_T_U8, CURVE_T_I64 = 0, 1


# LMN_OPTIM_* of include/optim/lmnet_optim.h
OPTIM_MAX_GROUPS, OPTIM_GRID_CAP, OPTIM_PARAM_BYTES = 16, 1024, 64
OPTIM_SKIP_NONFINITE, OPTIM_NORM = 1, 2
OPTIM_CTRL_WORDS, OPTIM_GROUP_WORDS = 16, 64
(OPTIM_SKIP, OPTIM_STEP, OPTIM_SKIPPED, OPTIM_GRAD_NORM, OPTIM_INV_SCALE, OPTIM_COEF, OPTIM_INV_BC1, OPTIM_INV_SQRT_BC2,
 OPTIM_NONFINITE) = range(9)


def optim_blocks(n):
    """Blocks of the reduction of lmn_optim_prepare over n floats: the control block starts at word 2 * optim_blocks(n)."""
    return max(1, min((int(n) // 4 + 255) // 256, OPTIM_GRID_CAP))


def optim_workspace_words(n):
    """lmn_optim_workspace restated (include/optim/lmnet_optim.h): block partials, block counts, control block, group table."""
    return 2 * optim_blocks(n) + OPTIM_CTRL_WORDS + OPTIM_GROUP_WORDS if n > 0 else 0


# The C ABI, one list per header: every symbol that header declares.  The headers stay apart, one per feature; HEADERS (below the
# lists) is the one registry of all sixteen.  load() checks the library against it, tests/test_host_cpu.py checks it against the
# headers, and the guard manifest (tests/guard.py) partitions EXPORTS, so that a new export in any header needs a guard test or a
# stated reason why none applies.  A new header joins by its list and its line in HEADERS (and STRUCTS / RETURNS_INT64 where they apply).
SYMBOLS = [
    "lmn_abi_version", "lmn_sizeof_conv_args", "lmn_sizeof_src", "lmn_sizeof_wgrad_args", "lmn_last_error",
    "lmn_conv_pack_size", "lmn_conv_pack", "lmn_conv_pack_batch", "lmn_sizeof_pack_job", "lmn_conv_fwd", "lmn_conv_dma_config", "lmn_conv_chain_ok", "lmn_conv_wgrad", "lmn_conv_wgrad_workspace",
    "lmn_conv_wgrad_job", "lmn_conv_wgrad_up2_ok", "lmn_wgrad_reduce_batch", "lmn_sizeof_reduce_job", "lmn_reparam_fold", "lmn_affine2", "lmn_reparam_wfin", "lmn_bnact_fwd_fin", "lmn_bnact_bwd_fin",
    "lmn_dw_stats", "lmn_dw_fwd", "lmn_dw_merge", "lmn_dw_finalize_merge", "lmn_dw_bwd_stats", "lmn_dw_bwd_coef", "lmn_dw_bwd", "lmn_dw_fwd_bn", "lmn_dw_bwd_bn",
    "lmn_se_fwd", "lmn_se_bwd", "lmn_se_bwd_dm", "lmn_se_bwd_params", "lmn_na_fwd", "lmn_na_bwd", "lmn_plan_host_profile", "lmn_set_deterministic", "lmn_get_deterministic", "lmn_gattn_fwd", "lmn_gattn_bwd",
    "lmn_ln_fwd", "lmn_ln_bwd", "lmn_bnact_fwd", "lmn_bnact_bwd_stats", "lmn_bnact_bwd",
    "lmn_bn_finalize", "lmn_bn_fold", "lmn_bn_bwd_coef", "lmn_up2_fwd", "lmn_up2_bwd", "lmn_avgpool_fwd", "lmn_avgpool_bwd",
    "lmn_nchw_to_nhwc", "lmn_nhwc_to_nchw", "lmn_adamw_step", "lmn_segloss_fwd", "lmn_segloss_bwd", "lmn_confusion", "lmn_preprocess_u8", "lmn_preprocess_u8_ex", "lmn_sizeof_aug_param", "lmn_augment_u8", "lmn_surface_workspace", "lmn_surface_dist", "lmn_post_workspace", "lmn_cc_label", "lmn_sizeof_post_param", "lmn_post_clean", "lmn_post_render", "lmn_confusion_labels", "lmn_fill", "lmn_add", "lmn_colsum", "lmn_copy_slice", "lmn_copy2d",
    "lmn_stream_wait", "lmn_event_record", "lmn_event_wait", "lmn_set_priority_stream", "lmn_plan_create", "lmn_plan_destroy", "lmn_plan_record_begin", "lmn_plan_record_end", "lmn_plan_size",
    "lmn_plan_run", "lmn_prof_begin", "lmn_prof_end",
]

# include/lmnet_oneof.h: the OneOf block of the training augmentations
SYMBOLS_ONEOF = ["lmn_sizeof_oneof_param", "lmn_oneof_workspace", "lmn_augment_oneof_u8"]

# include/lmnet_loss.h: void labels and the focal term of the loss, per-image statistics
SYMBOLS_LOSS = ["lmn_sizeof_loss_param", "lmn_segloss_ex_fwd", "lmn_segloss_ex_bwd", "lmn_image_stats"]

# include/lmnet_sigmoid.h: the loss and the statistics of sigmoid heads
SYMBOLS_SIGMOID = ["lmn_sizeof_sig_param", "lmn_sigloss_fwd", "lmn_sigloss_bwd", "lmn_sigmoid_stats"]

# include/optim/lmnet_optim.h: groups, clipping, the loss-scale skip and EMA of the one-launch AdamW (lm_net_amd.optim.FusedAdamW)
SYMBOLS_OPTIM = ["lmn_sizeof_optim_param", "lmn_optim_workspace", "lmn_optim_prepare", "lmn_adamw_step_ex"]

# include/tiles/lmnet_tiles.h: tiled and flip-averaged inference (lm_net_amd.infer.TiledPredictor)
SYMBOLS_TILES = ["lmn_sizeof_tile_param", "lmn_tile_gather", "lmn_tile_blend"]

# include/curves/lmnet_curves.h: score histograms over a threshold table (lm_net_amd.metrics.CurveMeter)
SYMBOLS_CURVES = ["lmn_curve_workspace", "lmn_curve_hist"]

# include/volume/lmnet_volume.h: per-case 3D surface distances and overlap (lm_net_amd.metrics.VolumeSurfaceMeter)
SYMBOLS_VOLUME = ["lmn_volume_workspace", "lmn_volume_labels", "lmn_volume_dist"]
VOLUME_MAX_SIDE = 1024       # LMN_VOLUME_* of the header
VOLUME_NSTAT_I = 9
VOLUME_NSTAT_F = 2

# include/volpost/lmnet_volpost.h: 3D connected-component cleaning of a label volume (lm_net_amd.post.VolumePostprocess)
SYMBOLS_VOLPOST = ["lmn_volpost_workspace", "lmn_cc3d_label", "lmn_volpost_clean"]
VOLPOST_MAX_SIDE = 1024      # LMN_VOLPOST_* of the header
VOLPOST_MAX_KEEP = 4
VOLPOST_NSTAT = 4

# include/lesion/lmnet_lesion.h: the components of two volumes and the join between them (lm_net_amd.metrics.LesionMeter)
SYMBOLS_LESION = ["lmn_lesion_workspace", "lmn_lesion_match"]
LESION_MAX_SIDE = 1024       # LMN_LESION_* of the header
LESION_MIN_SLOTS = 64
LESION_MAX_SLOTS = 1 << 22
LESION_NCTRL = 4

# include/distmap/lmnet_distmap.h: signed squared distance maps and the losses on them (lm_net_amd.loss.BoundaryLoss, HausdorffDTLoss)
SYMBOLS_DISTMAP = ["lmn_dist_workspace", "lmn_dist_map", "lmn_dist_loss_fwd", "lmn_dist_loss_bwd"]
DISTMAP_MAX_SIDE = 1024      # LMN_DISTMAP_* of the header
DISTMAP_LABELS_U8 = 0
DISTMAP_LABELS_I64 = 1
DISTMAP_SOFTMAX = 0
DISTMAP_SIGMOID = 1
DISTMAP_FLAG_EMPTY = 1
DISTMAP_FLAG_FULL = 2
DISTMAP_BOUNDARY = 0
DISTMAP_HAUSDORFF = 1
DISTMAP_SUMS_WORDS = 4

# include/lovasz/lmnet_lovasz.h: Lovasz-Softmax and the Lovasz hinge on a segmented device sort (lm_net_amd.loss.LovaszLoss)
SYMBOLS_LOVASZ = ["lmn_lovasz_workspace", "lmn_lovasz_order", "lmn_lovasz_fwd", "lmn_lovasz_bwd"]
LOVASZ_TILE = 2048           # LMN_LOVASZ_* of the header
LOVASZ_SCAN_THREADS = 64
LOVASZ_MAX_SEGMENTS = 65535
LOVASZ_LABELS_U8 = 0
LOVASZ_LABELS_I64 = 1
LOVASZ_SOFTMAX = 0
LOVASZ_SIGMOID = 1
LOVASZ_SUMS_WORDS = 4

# include/region/lmnet_region.h: Dice, Jaccard, Tversky and generalized Dice, per batch or per image (lm_net_amd.loss.RegionLoss)
SYMBOLS_REGION = ["lmn_region_workspace", "lmn_region_fwd", "lmn_region_bwd"]
REGION_DICE = 0              # LMN_REGION_* of the header
REGION_JACCARD = 1
REGION_TVERSKY = 2
REGION_GDICE = 3
REGION_LINEAR = 0
REGION_SQUARED = 1
REGION_SOFTMAX = 0
REGION_SIGMOID = 1
REGION_LABELS_U8 = 0
REGION_LABELS_I64 = 1
REGION_MAX_BATCH = 65535

# include/slices/lmnet_slices.h: volume statistics and the gather into fp32 2.5D batches (lm_net_amd.data.VolumeSlicer)
SYMBOLS_SLICES = ["lmn_slices_workspace", "lmn_slices_stats", "lmn_slices_gather"]
SLICES_I16 = 0               # LMN_SLICES_* of the header
SLICES_U8 = 1
SLICES_WINDOW = 0
SLICES_ZSCORE = 1
SLICES_PERCENTILE = 2
SLICES_EDGE_REPLICATE = 0
SLICES_EDGE_ZERO = 1
SLICES_BORDER_REPLICATE = 0
SLICES_BORDER_CONSTANT = 1
SLICES_LABELS_U8 = 0
SLICES_LABELS_I64 = 1
SLICES_MAX_DEPTH = 1024
SLICES_MAX_SIDE = 1024
SLICES_MAX_MODALITIES = 4
SLICES_MAX_CHANNELS = 16
SLICES_MAX_CONTEXT = 7
SLICES_MAX_OUT = 4096
SLICES_MAX_BATCH = 65535
SLICES_NSTAT = 8
SLICES_NO_FOREGROUND = -32769

# include/soft/lmnet_soft.h: soft-target criteria and the Mixup / CutMix mixer (lm_net_amd.loss.SoftSegLoss, DistillLoss, lm_net_amd.data.DeviceMix)
SYMBOLS_SOFT = ["lmn_soft_workspace", "lmn_soft_fwd", "lmn_soft_bwd", "lmn_mix_batch"]
SOFT_PROBS = 0               # LMN_SOFT_* of the header
SOFT_PAIR = 1
SOFT_TEACHER_F32 = 2
SOFT_TEACHER_BF16 = 3
SOFT_SOFTMAX = 0
SOFT_SIGMOID = 1
SOFT_LABELS_U8 = 0
SOFT_LABELS_I64 = 1
SOFT_MAX_BATCH = 65535
MIX_NONE = 0                 # LMN_MIX_* of the header
MIX_MIXUP = 1
MIX_CUTMIX = 2
MIX_ROW_WORDS = 8

# include/hard/lmnet_hard.h: top-k and OHEM cross entropy on a device radix select (lm_net_amd.loss.HardPixelLoss)
SYMBOLS_HARD = ["lmn_hard_workspace", "lmn_hard_fwd", "lmn_hard_bwd"]
HARD_SOFTMAX = 0             # LMN_HARD_* of the header
HARD_SIGMOID = 1
HARD_LABELS_U8 = 0
HARD_LABELS_I64 = 1
HARD_MAX_BATCH = 65535
HARD_MAX_GROUPS = 1024
HARD_RECORD_WORDS = 5
HARD_BINS_HIGH = 2048
HARD_BINS_LOW = 1024

HEADERS = {"lmnet_hip.h": SYMBOLS, "lmnet_oneof.h": SYMBOLS_ONEOF, "lmnet_loss.h": SYMBOLS_LOSS, "lmnet_sigmoid.h": SYMBOLS_SIGMOID,
           "optim/lmnet_optim.h": SYMBOLS_OPTIM, "tiles/lmnet_tiles.h": SYMBOLS_TILES, "curves/lmnet_curves.h": SYMBOLS_CURVES,
           "volume/lmnet_volume.h": SYMBOLS_VOLUME, "volpost/lmnet_volpost.h": SYMBOLS_VOLPOST, "lesion/lmnet_lesion.h": SYMBOLS_LESION,
           "distmap/lmnet_distmap.h": SYMBOLS_DISTMAP, "lovasz/lmnet_lovasz.h": SYMBOLS_LOVASZ, "region/lmnet_region.h": SYMBOLS_REGION,
           "slices/lmnet_slices.h": SYMBOLS_SLICES, "soft/lmnet_soft.h": SYMBOLS_SOFT, "hard/lmnet_hard.h": SYMBOLS_HARD}     # path under include/
EXPORTS = [name for names in HEADERS.values() for name in names]

# every struct mirror whose size the library reports, with the export that reports it.  (DwPre, SeFuse, SeBwd and SeParamsT
# have no lmn_sizeof_* export and stay unchecked.)
STRUCTS = [(ConvArgs, "lmn_sizeof_conv_args"), (SrcT, "lmn_sizeof_src"), (WgradArgs, "lmn_sizeof_wgrad_args"),
           (PackJob, "lmn_sizeof_pack_job"), (ReduceJob, "lmn_sizeof_reduce_job"), (AugParam, "lmn_sizeof_aug_param"),
           (PostParam, "lmn_sizeof_post_param"), (OneOfParam, "lmn_sizeof_oneof_param"), (LossParam, "lmn_sizeof_loss_param"),
           (SigParam, "lmn_sizeof_sig_param"), (OptimParam, "lmn_sizeof_optim_param"), (TileParam, "lmn_sizeof_tile_param")]

# the entries that do not return int: ctypes cuts a 64-bit result to 32 bits unless told (tests/test_host_cpu.py: the headers' prototypes)
RETURNS_INT64 = ["lmn_conv_pack_size", "lmn_conv_wgrad_workspace", "lmn_surface_workspace", "lmn_post_workspace", "lmn_plan_record_end",
                 "lmn_plan_size", "lmn_plan_host_profile", "lmn_prof_end", "lmn_oneof_workspace", "lmn_optim_workspace", "lmn_curve_workspace",
                 "lmn_volume_workspace", "lmn_volpost_workspace", "lmn_lesion_workspace", "lmn_dist_workspace", "lmn_lovasz_workspace",
                 "lmn_region_workspace", "lmn_slices_workspace", "lmn_soft_workspace", "lmn_hard_workspace"]
RETURNS_OTHER = {"lmn_last_error": C.c_char_p, "lmn_plan_create": C.c_void_p}

_lib = None


def load():
    """Load the HIP library (once).  Raises if it has not been built -- there is no CPU/torch fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            "lm_net_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C lm_net_amd/csrc`). The LM-Net hot path has no non-HIP fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise RuntimeError("lm_net_amd: %s does not export %s" % (LIB_PATH, name))
    for name in RETURNS_INT64:
        getattr(lib, name).restype = C.c_int64
    for name, restype in RETURNS_OTHER.items():
        getattr(lib, name).restype = restype
    # (the only entries with a 64-bit integer or a float ahead of the pointer block: declared, so that a Python int cannot be cut)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    lib.lmn_hard_workspace.argtypes = [ci] * 6
    lib.lmn_hard_fwd.restype = ci
    lib.lmn_hard_fwd.argtypes = [vp, vp, ci, ci, ci, cf, C.c_int64, cf, cf, ci, ci, ci, ci, vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.lmn_hard_bwd.restype = ci
    lib.lmn_hard_bwd.argtypes = [vp, vp, ci, ci, ci, cf, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    if lib.lmn_abi_version() != ABI_VERSION:
        raise RuntimeError("lm_net_amd: ABI version mismatch")
    for struct, sizeof in STRUCTS:
        n = getattr(lib, sizeof)()
        if n != C.sizeof(struct):
            raise RuntimeError("lm_net_amd: layout of %s differs between hip.py (%d bytes) and the library (%s() = %d)"
                               % (struct.__name__, C.sizeof(struct), sizeof, n))
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("lm_net_amd.%s failed (code %d): %s" % (what, rc, load().lmn_last_error().decode()))


def _host_size(name, n):
    """The result of a size entry that is host arithmetic: negative means refused, with the reason in lmn_last_error."""
    if n < 0:
        raise ValueError("lm_net_amd.%s: " % name + load().lmn_last_error().decode())
    return int(n)


def _p(t):
    """fp32 device pointer (parameters, statistics, workspaces, fp32 boundary tensors)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("lm_net_amd: device tensor required (got a CPU tensor); the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise RuntimeError("lm_net_amd: fp32 tensor required, got %s" % t.dtype)
    return C.c_void_p(t.data_ptr())


def _pa(t):
    """activation pointer: fp32 or bf16 storage (the call's act_dtype says which, see _dt)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("lm_net_amd: device tensor required (got a CPU tensor); the HIP path has no CPU fallback")
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("lm_net_amd: fp32 or bf16 activation tensor required, got %s" % t.dtype)
    return C.c_void_p(t.data_ptr())


def _dt(*ts):
    """act_dtype of a call: the storage type shared by all of its activation tensors."""
    d = None
    for t in ts:
        if t is None:
            continue
        t = t.t if isinstance(t, V) else t
        if d is None:
            d = t.dtype
        elif t.dtype != d:
            raise RuntimeError("lm_net_amd: activation tensors of one call must share a storage type (%s vs %s)" % (d, t.dtype))
    return BF16 if d == torch.bfloat16 else F32


_ALLOC = [None]    # allocator of the pass in flight (engine.begin_pass): fn(device, shape) -> fp32 tensor


def _default_alloc(device, shape):
    return torch.empty(shape, device=device, dtype=torch.float32)


_SEED_CTR = [None]  # device int32[1] added to every dropout seed (graph mode: bumped once per step), or None
_STREAM = [None]   # stream handle of the pass in flight (engine.begin_pass): torch.cuda.current_stream() costs ~3 us


def _stream():
    return _STREAM[0] if _STREAM[0] is not None else C.c_void_p(torch.cuda.current_stream().cuda_stream)


def stream_key():
    """The launch stream as a dictionary key: its handle as an int (0 = the legacy default stream; `c_void_p(0).value` is None,
    which once made the deferred reductions of a serial run on the default stream unreachable)."""
    v = _STREAM[0].value if _STREAM[0] is not None else torch.cuda.current_stream().cuda_stream
    return int(v or 0)


def _i64(v):
    return C.c_int64(int(v))


def _f(v):
    return C.c_float(float(v))


def rp4(t):
    """Mark ``t`` (shape [B, H, W, C], contiguous) as ROW-PLANAR: its memory holds element (b, y, x, c) at
    ((b*H + y) * (C/4) + (c >> 2)) * 4*W + 4*x + (c & 3) (include/lmnet_hip.h, Conventions) -- the layout of the E-wide tensors
    inside a ReparamConv block.  The shape stays [B, H, W, C] (it names the sizes); the conv family picks the layout up from the
    mark (lmn_src_t.rp_w / out_rp_w / aux_rp_w / dy_rp_w), the depthwise family takes nothing else.
    The mark is a Python attribute: clone() / view() / detach() / slicing return UNMARKED tensors -- the depthwise wrappers
    refuse those (_rp_req) instead of reading NHWC memory as row-planar."""
    if t.dim() != 4 or not t.is_contiguous() or t.shape[-1] % 4 != 0:
        raise RuntimeError("lm_net_amd: rp4() takes a contiguous [B, H, W, C] tensor with C %% 4 == 0 (got shape %s, contiguous=%s)"
                           % (tuple(t.shape), t.is_contiguous()))
    t._lmn_rp = True
    return t


def is_rp4(t):
    return getattr(t, "_lmn_rp", False)


def _rp_req(name, **ts):
    """The depthwise family reads and writes row-planar tensors only: every activation operand must carry the rp4 mark."""
    for k, t in ts.items():
        if t is not None and not getattr(t, "_lmn_rp", False):
            raise RuntimeError("lm_net_amd: %s: operand `%s` is not marked row-planar (hip.rp4 / hip.nhwc_to_rp4); "
                               "an NHWC tensor here would be read with permuted channels" % (name, k))


def nhwc_to_rp4(t):
    """torch-side layout conversion (tests, debugging): NHWC values -> a row-planar tensor of the same shape."""
    B, H, W, Cn = t.shape
    return rp4(t.reshape(B, H, W, Cn // 4, 4).permute(0, 1, 3, 2, 4).contiguous().reshape(B, H, W, Cn))


def rp4_to_nhwc(t):
    """torch-side layout conversion (tests, debugging): the NHWC values of a row-planar tensor."""
    B, H, W, Cn = t.shape
    return t.reshape(B, H, Cn // 4, W, 4).permute(0, 1, 3, 2, 4).contiguous().reshape(B, H, W, Cn)


class V:
    """A channel slice [off, off+C) of an NHWC tensor ``t`` of shape [..., Ctot] (contiguous); rp: image width W when the
    tensor is row-planar (whole tensors only), else 0."""
    __slots__ = ("t", "off", "C", "rp")

    def __init__(self, t, off=0, Cn=None):
        assert t.is_contiguous()
        self.t, self.off = t, off
        self.C = t.shape[-1] - off if Cn is None else Cn
        self.rp = 0
        if getattr(t, "_lmn_rp", False):
            assert off == 0 and self.C == t.shape[-1] and t.dim() == 4, "row-planar tensors are used whole"
            self.rp = t.shape[2]

    @property
    def ptr(self):
        if not self.t.is_cuda or self.t.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("lm_net_amd: fp32 or bf16 device tensor required")
        return self.t.data_ptr() + self.t.element_size() * self.off

    @property
    def cstride(self):
        return self.t.shape[-1]


def _as_view(x):
    return x if isinstance(x, V) else V(x)


def _fill_src(dst, s):
    """s: V | tensor | dict(view=, scale=, flags=, drop_seed=, drop_p=)"""
    if isinstance(s, dict):
        v = _as_view(s["view"])
        scale = s.get("scale")
        dst.ptr, dst.C, dst.cstride, dst.rp_w = v.ptr, v.C, v.cstride, v.rp
        dst.scale = scale.data_ptr() if scale is not None else None
        dst.flags = s.get("flags", 0)
        dst.drop_seed = s.get("drop_seed", 0)
        dst.drop_p = s.get("drop_p", 0.0)
        ln = s.get("ln")          # (gamma, beta, eps, stats [pixels, 2] or None): LayerNorm on load (SRC_LN is set here)
        if ln is not None:
            g_, b_, eps_, st_ = ln
            dst.flags |= SRC_LN
            dst.ln_gamma, dst.ln_beta, dst.ln_eps = _p(g_).value, _p(b_).value, float(eps_)
            dst.ln_stats = _p(st_).value if st_ is not None else None
        else:
            dst.ln_gamma = dst.ln_beta = dst.ln_stats = None
            dst.ln_eps = 0.0
    else:
        v = _as_view(s)
        dst.ptr, dst.C, dst.cstride, dst.rp_w = v.ptr, v.C, v.cstride, v.rp
        dst.scale, dst.flags, dst.drop_seed, dst.drop_p = None, 0, 0, 0.0
        dst.ln_gamma = dst.ln_beta = dst.ln_stats = None
        dst.ln_eps = 0.0
    return v.C


# ------------------------------------------------------------------------------------------ conv family
def conv_pack_size(ksize, rows, src_channels):
    arr = (C.c_int32 * len(src_channels))(*src_channels)
    return int(load().lmn_conv_pack_size(ksize, rows, len(src_channels), arr))


class PackPlan:
    """Packed forms of the PERSISTENT weights (nn.Parameter storage) used by one pass (forward or backward).

    The first pass runs every pack as its own launch and records it; later passes re-pack all recorded jobs
    with ONE ``lmn_conv_pack_batch`` launch in ``refresh()`` and ``conv_pack``/``conv_pack_t`` then only look
    their buffer up.  Jobs hold a reference to the weight tensor; if a parameter's storage moved
    (``model.to(...)``) the plan is dropped and re-recorded."""

    def __init__(self):
        self.jobs = {}        # key -> [weight tensor, packed tensor, PackJob fields]
        self.buffers = {}     # key -> plan-owned buffer that several jobs pack slices of
        self.table = None     # device copy of the job array
        self.blocks = 0
        self.fresh = False

    def refresh(self):
        self.fresh = False
        if not self.jobs:
            return
        if any(j[0].data_ptr() != j[2]["w"] for j in self.jobs.values()):
            self.jobs, self.buffers, self.table = {}, {}, None
            return
        if self.table is None:
            arr = (PackJob * len(self.jobs))()
            blk = 0
            for i, (wt, out, f) in enumerate(self.jobs.values()):
                a = arr[i]
                a.w, a.wpack, a.total, a.first_block = f["w"], out.data_ptr(), out.numel(), blk
                a.ksize, a.Cout, a.Cin, a.nsrc = f["ksize"], f["Cout"], f["Cin"], len(f["c"])
                for k, cc in enumerate(f["c"]):
                    a.c[k] = cc
                a.transposed, a.row_off, a.rows = f["transposed"], f["row_off"], f["rows"]
                a.dtype = f.get("dtype", F32)
                blk += (out.numel() + 1023) // 1024
            dev = next(iter(self.jobs.values()))[1].device
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self.table, self.blocks = host.to(dev), blk
        _check(load().lmn_conv_pack_batch(C.c_void_p(self.table.data_ptr()), len(self.jobs), _i64(self.blocks), _stream()),
               "conv_pack_batch")
        self.fresh = True

    def buffer(self, key, n, device):
        b = self.buffers.get(key)
        if b is None or b.numel() != n or b.device != device:
            b = self.buffers[key] = torch.empty(n, device=device, dtype=torch.float32)
        return b

    def lookup(self, key):
        j = self.jobs.get(key) if self.fresh else None
        return j[1] if j is not None else None

    def record(self, key, w, out, fields):
        self.jobs[key] = [w, out, fields]
        self.table = None     # rebuilt by the next refresh()


_PLAN = [None]                # the plan of the pass in flight (set by engine.begin_pass)


def _planned(w, out, persistent):
    return _PLAN[0] is not None and (out is None or persistent) and isinstance(w, torch.nn.Parameter)


def conv_pack(w, ksize, src_channels, out=None, persistent=False):
    """Pack a torch-layout weight [Cout, Cin(,k,k)] for the forward operator.  ``persistent``: ``out`` is a
    slice of a ``PackPlan.buffer`` (so the job may be recorded and replayed by the plan)."""
    cout, cin = w.shape[0], w.shape[1]
    planned = _planned(w, out, persistent)
    dt = _MMA[0]
    if planned:
        key = (w.data_ptr(), ksize, tuple(src_channels), 0, 0, 0, out.data_ptr() if out is not None else 0, dt)
        hit = _PLAN[0].lookup(key)
        if hit is not None:
            return hit
    n = conv_pack_size(ksize, cout, src_channels)      # floats of the fp32 form (the bf16 form fills the first half)
    if out is None:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    arr = (C.c_int32 * len(src_channels))(*src_channels)
    _check(load().lmn_conv_pack(_p(w), _p(out), ksize, cout, cin, len(src_channels), arr, 0, 0, 0, dt, _stream()), "conv_pack")
    if planned:
        _PLAN[0].record(key, w, out, dict(w=w.data_ptr(), ksize=ksize, Cout=cout, Cin=cin, c=list(src_channels),
                                          transposed=0, row_off=0, rows=0, dtype=dt))
    return out


def conv_pack_t(w, ksize, row_off=0, rows=None, out=None, cred=None, persistent=False):
    """Pack the data-gradient operator of a forward weight [Cout, Cin(,k,k)]: rows = input channels
    [row_off, row_off+rows), reduction over Cout.  `rows` may exceed the weight's Cin and `cred` (channels of the dy
    operand) its Cout by the zero padding to a multiple of 4 (RGB input as NHWC4, 2-class head on 4 rows)."""
    cout, cin = w.shape[0], w.shape[1]
    rows = cin - row_off if rows is None else rows
    cred = cout if cred is None else cred
    planned = _planned(w, out, persistent)
    dt = _MMA[0]
    if planned:
        key = (w.data_ptr(), ksize, (cred,), 1, row_off, rows, out.data_ptr() if out is not None else 0, dt)
        hit = _PLAN[0].lookup(key)
        if hit is not None:
            return hit
    n = conv_pack_size(ksize, rows, [cred])
    if out is None:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    arr = (C.c_int32 * 1)(cred)
    _check(load().lmn_conv_pack(_p(w), _p(out), ksize, cout, cin, 1, arr, 1, row_off, rows, dt, _stream()), "conv_pack_t")
    if planned:
        _PLAN[0].record(key, w, out, dict(w=w.data_ptr(), ksize=ksize, Cout=cout, Cin=cin, c=[cred],
                                          transposed=1, row_off=row_off, rows=rows, dtype=dt))
    return out


def conv_fwd(srcs, wpack, out, *, B, Hin, Win, Hout, Wout, Cout, ksize=1, stride=1, transposed=0, bias=None, bias2=None,
             epilogue=EP_LINEAR, act=ACT_NONE, p=(), aux=None, residual=None, stats=None, stats_mode=STATS_NONE,
             drop_p=0.0, drop_seed=0, stats_rep=1, stats_snap=False, fin=None, chain=None, query_chain=False):
    """chain: dict(wpack=, Cout=, out=, bias=None, shift=None, aux=None, stats=None, epilogue=EP_LINEAR, stats_mode=STATS_NONE, stats_rep=1,
    stats_snap=False) -- a second 1x1 conv on the output tile (lmn_conv_chain_t); query_chain=True: nothing is launched, returns whether
    the library takes the call with its chain (lmn_conv_chain_ok).
    fin: dict(mode=FIN_BN | FIN_BN_BWD, sums=[nrep(+1), 2, C] tensor, nrep, count, ...) -- in-kernel BatchNorm bookkeeping
    (lmn_bn_fin_t): tensors for gamma / beta / about / mean / rstd / A / shift / rmean / rvar / Ain / dgamma / dbeta."""
    a = ConvArgs()
    a.B, a.Hout, a.Wout, a.Hin, a.Win = B, Hout, Wout, Hin, Win
    a.ksize, a.stride, a.transposed, a.nsrc, a.Cout = ksize, stride, transposed, len(srcs), Cout
    for i, s in enumerate(srcs):
        _fill_src(a.src[i], s)
    a.wpack = wpack.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.bias2 = bias2.data_ptr() if bias2 is not None else None
    ps = [t.data_ptr() if t is not None else None for t in p] + [None] * (7 - len(p))
    a.p0, a.p1, a.p2, a.p3, a.p4, a.p5, a.p6 = ps
    if aux is not None:
        v = _as_view(aux)
        a.aux, a.aux_cstride, a.aux_rp_w = v.ptr, v.cstride, v.rp
    if residual is not None:
        v = _as_view(residual)
        assert not v.rp, "conv_fwd: a row-planar residual is not supported"
        a.residual, a.res_cstride = v.ptr, v.cstride
    if out is not None:
        v = _as_view(out)
        a.out, a.out_cstride, a.out_rp_w = v.ptr, v.cstride, v.rp
    a.stats = stats.data_ptr() if stats is not None else None
    a.stats_rep = stats_rep
    a.stats_snap = int(bool(stats_snap))
    if fin is not None:
        _fill_fin(a.fin, fin)
    a.epilogue, a.act, a.stats_mode = epilogue, act, stats_mode
    a.drop_p, a.drop_seed = drop_p, drop_seed
    a.mma_dtype = _MMA[0]
    a.act_dtype = _dt(*[(s["view"] if isinstance(s, dict) else s) for s in srcs], aux, residual, out)
    a.seed_ctr = _SEED_CTR[0].data_ptr() if _SEED_CTR[0] is not None else None
    if chain is not None:
        c = a.chain
        c.wpack = chain["wpack"].data_ptr()
        c.bias = chain["bias"].data_ptr() if chain.get("bias") is not None else None
        c.shift = chain["shift"].data_ptr() if chain.get("shift") is not None else None
        c.stats = chain["stats"].data_ptr() if chain.get("stats") is not None else None
        vo = _as_view(chain["out"])
        c.out, c.out_cstride, c.out_rp_w, c.Cout = vo.ptr, vo.cstride, vo.rp, chain["Cout"]
        if chain.get("aux") is not None:
            va = _as_view(chain["aux"])
            c.aux, c.aux_cstride, c.aux_rp_w = va.ptr, va.cstride, va.rp
        c.epilogue, c.stats_mode = chain.get("epilogue", EP_LINEAR), chain.get("stats_mode", STATS_NONE)
        c.stats_rep, c.stats_snap = chain.get("stats_rep", 1), int(bool(chain.get("stats_snap", False)))
    if query_chain:
        return bool(load().lmn_conv_chain_ok(C.byref(a)))
    _check(load().lmn_conv_fwd(C.byref(a), _stream()), "conv_fwd")


def conv_dma_config(mode=-1, min_tiles=-1):
    """lmn_conv_dma_config: which LDS-DMA kernel forms lmn_conv_fwd may pick (bit 0 conv_dma3, bit 1 conv_dma1, bit 2 conv_dmaM; 0 = the
    LDS-tiled kernels everywhere), smallest call (in 8x16-pixel tiles) that takes the small-channel forms; -1 keeps a value.  Returns the
    previous mode (-1: not set yet, the LMN_CONV_DMA default applies)."""
    return int(load().lmn_conv_dma_config(int(mode), int(min_tiles)))


def conv_wgrad_up2_ok(src, dy, *, B, Hin, Win, Cout):
    """True when conv_wgrad takes `src` (the half-resolution map) with SRC_UP2 for a 3x3 stride-1 weight gradient over the Hin x Win
    upsampled image (lmn_conv_wgrad_up2_ok: the library's own launch predicate, host arithmetic only)."""
    a = WgradArgs()
    a.B, a.Hout, a.Wout, a.Hin, a.Win = B, Hin, Win, Hin, Win
    a.ksize, a.stride, a.nsrc, a.Cout = 3, 1, 1, Cout
    _fill_src(a.src[0], dict(view=src, flags=SRC_UP2))
    v = _as_view(dy)
    a.dy, a.dy_cstride, a.dy_rp_w = v.ptr, v.cstride, v.rp
    a.dW = 0x1000   # (any non-null pointer: the query touches no memory)
    a.mma_dtype = _MMA[0]
    a.act_dtype = _dt(src, dy)
    return bool(load().lmn_conv_wgrad_up2_ok(C.byref(a)))


def conv_wgrad(srcs, dy, dW, db, *, B, Hin, Win, Hout, Wout, Cout, ksize=1, stride=1, dy_flags=0, dy_seed=0, dy_p=0.0,
               dW_src=None, db2=None, defer=False):
    """dW_src: optional list (one entry per source, None = use the columns of dW) of per-source gradient tensors.
    defer: leave the second stage of the K-split reduction to `wgrad_reduce_flush()` (one launch for all deferred calls of the
    launch stream); the call then writes its block partials to a workspace of its own.  Returns that workspace (or None)."""
    a = WgradArgs()
    a.B, a.Hout, a.Wout, a.Hin, a.Win = B, Hout, Wout, Hin, Win
    a.ksize, a.stride, a.nsrc, a.Cout = ksize, stride, len(srcs), Cout
    for i, s in enumerate(srcs):
        _fill_src(a.src[i], s)
    v = _as_view(dy)
    a.dy, a.dy_cstride, a.dy_rp_w = v.ptr, v.cstride, v.rp
    a.dy_flags, a.dy_seed, a.dy_p = dy_flags, dy_seed, dy_p
    a.dW = dW.data_ptr() if dW is not None else None
    a.db = db.data_ptr() if db is not None else None
    a.db2 = db2.data_ptr() if db2 is not None else None
    a.mma_dtype = _MMA[0]
    a.act_dtype = _dt(*[(s["view"] if isinstance(s, dict) else s) for s in srcs], dy)
    if dW_src is not None:
        for i, t in enumerate(dW_src):
            a.dW_src[i] = t.data_ptr() if t is not None else None
    lib = load()
    need = int(lib.lmn_conv_wgrad_workspace(C.byref(a)))
    ws = None
    if need > 0 and defer:
        # the call's own workspace, sized to the partials it will really write (lmn_conv_wgrad_workspace is the upper bound)
        a.workspace, a.workspace_floats = 0x1000, need      # (any non-null pointer: the geometry query does not touch it)
        job = ReduceJob()
        _check(lib.lmn_conv_wgrad_job(C.byref(a), C.byref(job)), "conv_wgrad_job")
        if job.nblk > 0:
            nfl = job.gy * job.nblk * job.per
            ws = (_ALLOC[0] or _default_alloc)(v.t.device, (nfl,))
            a.workspace, a.workspace_floats = ws.data_ptr(), nfl
            a.defer_reduce = 1
            job.partial = ws.data_ptr()
            _RJOBS.setdefault(stream_key(), []).append((job, ws))
        else:
            a.workspace, a.workspace_floats = None, 0
            need = 0
    elif need > 0:
        wsh = _workspace(v.t.device, need)
        a.workspace, a.workspace_floats = wsh.data_ptr(), wsh.numel()
    a.seed_ctr = _SEED_CTR[0].data_ptr() if _SEED_CTR[0] is not None else None
    _check(lib.lmn_conv_wgrad(C.byref(a), _stream()), "conv_wgrad")
    return ws


_RJOBS = {}          # launch stream handle -> [(ReduceJob, workspace tensor)] deferred since the last flush on that stream
_RTABLES = {}        # bytes of a job table -> its device copy (pointers repeat from step to step: no H2D copy per flush)


def wgrad_reduce_pending(key=None):
    key = int(key or 0) if key is not None else stream_key()
    return len(_RJOBS.get(key, ()))


def _reduce_targets(j):
    return {int(v) for v in (j.dW, j.dW_src[0], j.dW_src[1], j.dW_src[2], j.db, j.db2) if v}


def wgrad_reduce_flush():
    """Sum the block partials of every deferred weight gradient of the CURRENT launch stream in one launch.  Returns the
    device job tables (the caller keeps them alive while a recorded plan references them); [] when nothing was pending.
    The batched kernel adds into its destinations with plain read-modify-writes, so two jobs of one launch must not share a
    destination (a weight used twice, a module called twice, accumulation into one explicit dW): such jobs are split into
    consecutive launches, which the stream serialises as the per-layer reduce launches used to.
    A job table whose bytes were not seen before is uploaded with a BLOCKING copy from pageable memory on torch's current stream:
    the host waits for everything queued on that stream.  Pointers repeat from step to step on an idle stream, so a steady host-
    launched step hits the cache and does not wait; behind a stalled caller's stream the allocator hands out other blocks, every
    flush misses and the step waits for the stream (tests/test_busy_model_gpu.py pins this; recorded plans do not flush from the
    host and never wait).  The wait is load-bearing: see DESIGN 5u before replacing it with a non-blocking copy."""
    key = stream_key()
    jobs = _RJOBS.pop(key, None)
    if not jobs:
        return []
    groups, seen = [[]], set()
    for job in jobs:
        t = _reduce_targets(job[0])
        if groups[-1] and (t & seen):
            groups.append([])
            seen = set()
        groups[-1].append(job)
        seen |= t
    tabs = []
    for grp in groups:
        arr = (ReduceJob * len(grp))()
        blk = 0
        for i, (j, _) in enumerate(grp):
            j.first_block = blk
            C.memmove(C.byref(arr[i]), C.byref(j), C.sizeof(ReduceJob))
            blk += j.gy * j.blocks_per_set
        raw = bytes(arr)
        dev = grp[0][1].device
        tab = _RTABLES.get((dev, raw))
        if tab is None:
            if len(_RTABLES) > 4096:
                _RTABLES.clear()
            tab = _RTABLES[(dev, raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
        _check(load().lmn_wgrad_reduce_batch(C.c_void_p(tab.data_ptr()), len(grp), _i64(blk), _stream()), "wgrad_reduce_batch")
        tabs.append(tab)
    return tabs


def wgrad_reduce_drop():
    """Forget deferred jobs (a pass that raised)."""
    _RJOBS.clear()


_ws_cache = {}


def _workspace(device, nfloats):
    """Scratch buffer of the weight-gradient K-split reduction, one per (device, launch stream): users of one
    stream reuse it in stream order.  Allocated once at the library's cap (lmn_conv_wgrad_workspace never asks for
    more than 16 M floats), so it is never re-allocated under kernels still in flight on another stream."""
    key = (device, stream_key())
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nfloats:
        ws = torch.empty(max(nfloats, 16 << 20), device=device, dtype=torch.float32)
        _ws_cache[key] = ws
    return ws


# ------------------------------------------------------------------------------------------ depthwise block
def dw_stats(x1, w5, w3, wv, wh, stats, zpre=None):
    """zpre: the tensor is z (z-path, see _dw_pre); with zpre['fin'] the expand conv's BatchNorm is finalised here."""
    B, H, W, E = x1.shape
    _rp_req("dw_stats", x1=x1)
    _check(load().lmn_dw_stats(_pa(x1), B, H, W, E, _p(w5), _p(w3), _p(wv), _p(wh), _p(stats), _dw_pre(zpre), _dt(x1), _stream()), "dw_stats")


def dw_merge(w5, w3, wv, wh, A, shift, keff, beff):
    _check(load().lmn_dw_merge(_p(w5), _p(w3), _p(wv), _p(wh), _p(A), _p(shift), _p(keff), _p(beff), w5.shape[0],
                               _stream()), "dw_merge")


def dw_fwd(x1, pre, gsum, keff, beff, se=None, zpre=None):
    """se: squeeze-excite gate formed inside the pass (see _se_fuse), or None; zpre: the tensor is z (see _dw_pre)."""
    B, H, W, E = x1.shape
    _rp_req("dw_fwd", x1=x1, pre=pre)
    _check(load().lmn_dw_fwd(_pa(x1), _pa(pre), _p(gsum), B, H, W, E, _p(keff), _p(beff), _se_fuse(se), _dw_pre(zpre), _dt(x1, pre), _stream()), "dw_fwd")


def dw_finalize_merge(stats, count, bns, ws, mean, rstd, A, keff, beff):
    """bns: the four BatchNorm2d modules (branch order 5x5, 3x3, 3x1, 1x3); ws: the four depthwise weights."""
    P4 = C.c_void_p * 4
    F4 = C.c_float * 4
    E = mean.shape[-1]
    _check(load().lmn_dw_finalize_merge(
        _p(stats), _f(count), P4(*[b.weight.data_ptr() for b in bns]), P4(*[b.bias.data_ptr() for b in bns]),
        P4(*[b.running_mean.data_ptr() for b in bns]), P4(*[b.running_var.data_ptr() for b in bns]),
        F4(*[b.eps for b in bns]), F4(*[(b.momentum if b.momentum is not None else 0.1) for b in bns]),
        _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(ws[3]), _p(mean), _p(rstd), _p(A), _p(keff), _p(beff), E, _stream()),
        "dw_finalize_merge")


def dw_fwd_bn(x1, pre, gsum, stats, count, bns, ws, mean, rstd, A, se=None, zpre=None):
    """dw_finalize_merge + dw_fwd in one launch (training): bns / ws as in dw_finalize_merge."""
    P4 = C.c_void_p * 4
    F4 = C.c_float * 4
    B, H, W, E = x1.shape
    _rp_req("dw_fwd_bn", x1=x1, pre=pre)
    _check(load().lmn_dw_fwd_bn(
        _pa(x1), _pa(pre), _p(gsum), B, H, W, E, _p(stats), _f(count), P4(*[b.weight.data_ptr() for b in bns]),
        P4(*[b.bias.data_ptr() for b in bns]), P4(*[b.running_mean.data_ptr() for b in bns]),
        P4(*[b.running_var.data_ptr() for b in bns]), F4(*[b.eps for b in bns]),
        F4(*[(b.momentum if b.momentum is not None else 0.1) for b in bns]), _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(ws[3]),
        _p(mean), _p(rstd), _p(A), _se_fuse(se), _dw_pre(zpre), _dt(x1, pre), _stream()), "dw_fwd_bn")


def dw_bwd_bn(x1, dpre, dx1, w5, w3, wv, wh, bstats, mean, rstd, A, count, batch_stats, dgs, dbs, dw5, dw3, dwv, dwh, part=0,
              zpre=None, hstats=None):
    """dw_bwd_coef + dw_bwd in one launch (part 1: dx1 + gamma / beta gradients only, part 2: the weight gradients only).
    zpre / hstats: z-path -- x1 is z, `dx1` receives dh = dx1 * Hardswish'(A z + shift), hstats [2][E] += (sum dh, sum dh z)."""
    P4 = C.c_void_p * 4
    B, H, W, E = x1.shape
    _rp_req("dw_bwd_bn", x1=x1, dpre=dpre, dx1=dx1)
    _check(load().lmn_dw_bwd_bn(_pa(x1), _pa(dpre), _pa(dx1), B, H, W, E, _p(w5), _p(w3), _p(wv), _p(wh), _p(bstats), _p(mean),
                                _p(rstd), _p(A), _f(count), int(batch_stats), P4(*[t.data_ptr() for t in dgs]),
                                P4(*[t.data_ptr() for t in dbs]), _p(dw5), _p(dw3), _p(dwv), _p(dwh), part, _dw_pre(zpre),
                                _p(hstats), _dt(x1, dpre, dx1), _stream()), "dw_bwd_bn")


def dw_bwd_stats(x1, pre, u, s, dm, dpre, w5, w3, wv, wh, bstats, seb=None, zpre=None):
    """seb: dict(ds, fc1w, fc2w, hidden, dvec, inv_hw) -- the squeeze-excite backward formed inside the pass (dm may be None)."""
    B, H, W, E = x1.shape
    sb = None
    if seb is not None:
        f = SeBwd()
        f.ds, f.w1, f.w2, f.hidden, f.dvec = (_p(seb[k]).value for k in ("ds", "fc1w", "fc2w", "hidden", "dvec"))
        f.inv_hw, f.R = float(seb["inv_hw"]), seb["fc1w"].shape[0]
        sb = C.byref(f)
    _rp_req("dw_bwd_stats", x1=x1, pre=pre, u=u, dpre=dpre)
    _check(load().lmn_dw_bwd_stats(_pa(x1), _pa(pre), _pa(u), _p(s), _p(dm), _pa(dpre), B, H, W, E, _p(w5), _p(w3), _p(wv),
                                   _p(wh), _p(bstats), sb, _dw_pre(zpre), _dt(x1, pre, u, dpre), _stream()), "dw_bwd_stats")


def dw_bwd_coef(bstats, mean, rstd, A, count, batch_stats, cA, cC, cD, dgs, dbs):
    E = A.shape[-1]
    _check(load().lmn_dw_bwd_coef(_p(bstats), _p(mean), _p(rstd), _p(A), _f(count), int(batch_stats), _p(cA), _p(cC),
                                  _p(cD), *[_p(t) for t in dgs], *[_p(t) for t in dbs], E, _stream()), "dw_bwd_coef")


def dw_bwd(x1, dpre, dx1, w5, w3, wv, wh, cA, cC, cD, dw5, dw3, dwv, dwh):
    B, H, W, E = x1.shape
    _rp_req("dw_bwd", x1=x1, dpre=dpre, dx1=dx1)
    _check(load().lmn_dw_bwd(_pa(x1), _pa(dpre), _pa(dx1), B, H, W, E, _p(w5), _p(w3), _p(wv), _p(wh), _p(cA), _p(cC),
                             _p(cD), _p(dw5), _p(dw3), _p(dwv), _p(dwh), _dt(x1, dpre, dx1), _stream()), "dw_bwd")


def se_fwd(gsum, inv_hw, w1, b1, w2, b2, s, hidden):
    B, E = gsum.shape
    _check(load().lmn_se_fwd(_p(gsum), _f(inv_hw), _p(w1), _p(b1), _p(w2), _p(b2), _p(s), _p(hidden), B, E, w1.shape[0],
                             _stream()), "se_fwd")


def se_bwd(ds, gsum, inv_hw, w1, b1, w2, b2, hidden, dm, dw1, db1, dw2, db2):
    B, E = gsum.shape
    _check(load().lmn_se_bwd(_p(ds), _p(gsum), _f(inv_hw), _p(w1), _p(b1), _p(w2), _p(b2), _p(hidden), _p(dm), _p(dw1),
                             _p(db1), _p(dw2), _p(db2), B, E, w1.shape[0], _stream()), "se_bwd")


def se_bwd_dm(ds, s, inv_hw, w1, w2, hidden, dm, dvec):
    B, E = s.shape
    _check(load().lmn_se_bwd_dm(_p(ds), _p(s), _f(inv_hw), _p(w1), _p(w2), _p(hidden), _p(dm), _p(dvec), B, E, w1.shape[0],
                                _stream()), "se_bwd_dm")


def se_bwd_params(dvec, gsum, inv_hw, hidden, dw1, db1, dw2, db2):
    B, E = gsum.shape
    _check(load().lmn_se_bwd_params(_p(dvec), _p(gsum), _f(inv_hw), _p(hidden), _p(dw1), _p(db1), _p(dw2), _p(db2), B, E,
                                    dw1.shape[0], _stream()), "se_bwd_params")


# ------------------------------------------------------------------------------------------ attention
def _na_k(rpb, heads, direct):
    K = (rpb.shape[-1] + 1) // 2          # rpb: [heads][2K-1][2K-1]
    assert tuple(rpb.shape) == (heads, 2 * K - 1, 2 * K - 1), tuple(rpb.shape)
    return -K if direct else K            # negative: the direct (run-time K) kernels also at K = 3


def na_fwd(qkv, rpb, out, heads, direct=False):
    B, H, W, C3 = qkv.shape
    hd = C3 // 3 // heads
    _check(load().lmn_na_fwd(_pa(qkv), _p(rpb), _pa(out), B, H, W, heads, hd, _na_k(rpb, heads, direct), _f(hd ** -0.5),
                             _dt(qkv, out), _stream()), "na_fwd")


def na_bwd(qkv, rpb, dout, dqkv, drpb, heads, stat=None, direct=False):
    B, H, W, C3 = qkv.shape
    hd = C3 // 3 // heads
    if stat is None:
        stat = (_ALLOC[0] or _default_alloc)(qkv.device, (B * H * W * 2 * heads,))
    _check(load().lmn_na_bwd(_pa(qkv), _p(rpb), _pa(dout), _pa(dqkv), _p(drpb), _p(stat), B, H, W, heads, hd,
                             _na_k(rpb, heads, direct), _f(hd ** -0.5), _dt(qkv, dout, dqkv), _stream()), "na_bwd")


def gattn_fwd(qkv, out, lse, heads):
    B, N, C3 = qkv.shape
    hd = C3 // 3 // heads
    _check(load().lmn_gattn_fwd(_pa(qkv), _pa(out), _p(lse), B, N, heads, hd, _f(hd ** -0.5), _dt(qkv, out), _stream()), "gattn_fwd")


def gattn_bwd(qkv, out, dout, lse, dqkv, delta, heads):
    B, N, C3 = qkv.shape
    hd = C3 // 3 // heads
    _check(load().lmn_gattn_bwd(_pa(qkv), _pa(out), _pa(dout), _p(lse), _pa(dqkv), _p(delta), B, N, heads, hd,
                                _f(hd ** -0.5), _dt(qkv, out, dout, dqkv), _stream()), "gattn_bwd")


# ------------------------------------------------------------------------------------------ norms
def ln_fwd(x, gamma, beta, y):
    Cn = x.shape[-1]
    _check(load().lmn_ln_fwd(_pa(x), _p(gamma), _p(beta), _pa(y), _i64(x.numel() // Cn), Cn, _dt(x, y), _stream()), "ln_fwd")


def ln_bwd(x, gamma, dy, dres, dx, dgamma, dbeta):
    Cn = x.shape[-1]
    _check(load().lmn_ln_bwd(_pa(x), _p(gamma), _pa(dy), _pa(dres), _pa(dx), _p(dgamma), _p(dbeta), _i64(x.numel() // Cn),
                             Cn, _dt(x, dy, dres, dx), _stream()), "ln_bwd")


def bnact_fwd(z, a, b, y, act):
    Cn = z.shape[-1]
    _check(load().lmn_bnact_fwd(_pa(z), _p(a), _p(b), _pa(y), _i64(z.numel() // Cn), Cn, act, _dt(z, y), _stream()), "bnact_fwd")


def bnact_fwd_fin(z, fin, y, act):
    """lmn_bnact_fwd_fin: y = act(A z + shift) with A / shift formed in the kernel from the batch sums (fin: dict as for conv_fwd)."""
    Cn = z.shape[-1]
    f = BnFin()
    _fill_fin(f, fin)
    _check(load().lmn_bnact_fwd_fin(_pa(z), C.byref(f), _pa(y), _i64(z.numel() // Cn), Cn, act, _dt(z, y), _stream()), "bnact_fwd_fin")


def bnact_bwd_fin(z, dy, mean, rstd, gamma, beta, fin, dz, act):
    """lmn_bnact_bwd_fin: dz with c1 / c2 / c3 formed in the kernel from the sums of bnact_bwd_stats (fin: mode FIN_BN_BWD)."""
    Cn = z.shape[-1]
    f = BnFin()
    _fill_fin(f, fin)
    _check(load().lmn_bnact_bwd_fin(_pa(z), _pa(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), C.byref(f), _pa(dz),
                                    _i64(z.numel() // Cn), Cn, act, _dt(z, dy, dz), _stream()), "bnact_bwd_fin")


def bnact_bwd_stats(z, dy, mean, rstd, gamma, beta, stats, act):
    Cn = z.shape[-1]
    _check(load().lmn_bnact_bwd_stats(_pa(z), _pa(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(stats),
                                      _i64(z.numel() // Cn), Cn, act, _dt(z, dy), _stream()), "bnact_bwd_stats")


def bnact_bwd(z, dy, mean, rstd, gamma, beta, c1, c2, c3, dz, act):
    Cn = z.shape[-1]
    _check(load().lmn_bnact_bwd(_pa(z), _pa(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(c1), _p(c2), _p(c3), _pa(dz),
                                _i64(z.numel() // Cn), Cn, act, _dt(z, dy, dz), _stream()), "bnact_bwd")


def bn_finalize(sums, count, gamma, beta, eps, momentum, mean, rstd, A, shift, running_mean, running_var, about=None):
    """about: the per-channel value the sums were taken about (conv_fwd(..., p=(None,)*4 + (about,))), or None."""
    nrep = sums.shape[0] if sums.dim() == 3 else 1      # [nrep][2][C] slices (conv_fwd(stats_rep=nrep)) or [2][C]
    _check(load().lmn_bn_finalize(_p(sums), nrep, _f(count), _p(gamma), _p(beta), _f(eps), _f(momentum), _p(mean), _p(rstd),
                                  _p(A), _p(shift), _p(running_mean), _p(running_var), _p(about), gamma.numel(), _stream()),
           "bn_finalize")


def bn_fold(running_mean, running_var, gamma, beta, eps, mean, rstd, A, shift):
    _check(load().lmn_bn_fold(_p(running_mean), _p(running_var), _p(gamma), _p(beta), _f(eps), _p(mean), _p(rstd), _p(A),
                              _p(shift), gamma.numel(), _stream()), "bn_fold")


def bn_bwd_coef(bstats, count, A, dgamma, dbeta, c1, c2, c3, batch_stats=True):
    nrep = bstats.shape[0] if bstats.dim() == 3 else 1
    _check(load().lmn_bn_bwd_coef(_p(bstats), nrep, _f(count), int(batch_stats), _p(A), _p(dgamma), _p(dbeta), _p(c1), _p(c2),
                                  _p(c3), A.numel(), _stream()), "bn_bwd_coef")


# ------------------------------------------------------------------------------------------ resampling / layout / utils
def up2_fwd(x, y):
    x, y = _as_view(x), _as_view(y)
    B, Hin, Win = x.t.shape[:3]
    _check(load().lmn_up2_fwd(C.c_void_p(x.ptr), C.c_void_p(y.ptr), B, Hin, Win, x.C, x.cstride, y.cstride, _dt(x, y),
                              _stream()), "up2_fwd")


def up2_bwd(dy, dx):
    dy, dx = _as_view(dy), _as_view(dx)
    B, Hin, Win = dx.t.shape[:3]
    _check(load().lmn_up2_bwd(C.c_void_p(dy.ptr), C.c_void_p(dx.ptr), B, Hin, Win, dx.C, dy.cstride, dx.cstride,
                              _dt(dy, dx), _stream()), "up2_bwd")


def avgpool_fwd(x, y, f):
    x, y = _as_view(x), _as_view(y)
    B, Hout, Wout = y.t.shape[:3]
    _check(load().lmn_avgpool_fwd(C.c_void_p(x.ptr), C.c_void_p(y.ptr), B, Hout, Wout, f, x.C, x.cstride, y.cstride,
                                  _dt(x, y), _stream()), "avgpool_fwd")


def avgpool_bwd(dy, dx, f, accumulate):
    dy, dx = _as_view(dy), _as_view(dx)
    B, Hout, Wout = dy.t.shape[:3]
    _check(load().lmn_avgpool_bwd(C.c_void_p(dy.ptr), C.c_void_p(dx.ptr), B, Hout, Wout, f, dx.C, dy.cstride,
                                  dx.cstride, int(accumulate), _dt(dy, dx), _stream()), "avgpool_bwd")


def nchw_to_nhwc(x, y):
    B, Cn, H, W = x.shape
    _check(load().lmn_nchw_to_nhwc(_p(x), _pa(y), B, Cn, H, W, y.shape[-1], _dt(y), _stream()), "nchw_to_nhwc")


def nhwc_to_nchw(x, y):
    B, Cn, H, W = y.shape
    _check(load().lmn_nhwc_to_nchw(_pa(x), _p(y), B, Cn, H, W, x.shape[-1], _dt(x), _stream()), "nhwc_to_nchw")


def _pl(t):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
        raise RuntimeError("lm_net_amd: contiguous int64 device tensor required for labels")
    return C.c_void_p(t.data_ptr())


def _dims(logits):
    """B, C and the pixels per plane of logits [B, C, ...]"""
    B, Cn = logits.shape[0], logits.shape[1]
    return B, Cn, logits.numel() // (B * Cn)


def segloss_fwd(logits, target, w_ce, w_dice, label_smoothing, smooth, sums, coef, loss):
    B, Cn, hw = _dims(logits)
    _check(load().lmn_segloss_fwd(_p(logits), _pl(target), _p(w_ce), _p(w_dice), B, Cn, _i64(hw), _f(label_smoothing),
                                  _f(smooth), _p(sums), _p(coef), _p(loss), _stream()), "segloss_fwd")


def segloss_bwd(logits, target, w_ce, coef, gscale, dlogits):
    B, Cn, hw = _dims(logits)
    _check(load().lmn_segloss_bwd(_p(logits), _pl(target), _p(w_ce), _p(coef), _p(gscale), B, Cn, _i64(hw), _p(dlogits),
                                  _stream()), "segloss_bwd")


def confusion(logits, target, counts):
    """counts[t*C + p] += pixels with label t and arg-max p of fp32 logits [B, C, ...] (lmn_confusion); counts: C*C floats.  The cells
    are floats: 2^24 pixels or more in one call are refused, so a call on zeroed counts is exact (ConfusionMeter splits larger inputs)."""
    B, Cn, hw = _dims(logits)
    if counts.numel() != Cn * Cn or target.numel() != B * hw:
        raise ValueError("lm_net_amd.confusion: logits %s need %d x %d counts and %d labels, got counts %s and target %s"
                         % (tuple(logits.shape), Cn, Cn, B * hw, tuple(counts.shape), tuple(target.shape)))
    _check(load().lmn_confusion(_p(logits), _pl(target), B, Cn, _i64(hw), _p(counts), _stream()), "confusion")


def loss_param(ignore_index=None, label_smoothing=0.0, smooth=1e-5, ce_scale=1.0, dice_scale=1.0, focal_scale=0.0, focal_gamma=2.0,
               focal_alpha=0.25):
    """A LossParam (lmn_loss_param_t) from Python values; ignore_index None: no ignore label."""
    p = LossParam()
    p.has_ignore, p.ignore_index = (0, 0) if ignore_index is None else (1, int(ignore_index))
    p.label_smoothing, p.smooth = float(label_smoothing), float(smooth)
    p.ce_scale, p.dice_scale, p.focal_scale = float(ce_scale), float(dice_scale), float(focal_scale)
    p.focal_gamma, p.focal_alpha = float(focal_gamma), float(focal_alpha)
    return p


def segloss_ex_fwd(logits, target, w_ce, w_dice, param, sums, coef, loss4):
    """loss4 = [total, ce, dice, focal] with void labels and the focal term (lmn_segloss_ex_fwd); param: a LossParam; sums / coef:
    fp32 workspaces of at least loss_sums_floats(C) / loss_coef_floats(C)."""
    B, Cn, hw = _dims(logits)
    if sums.numel() < loss_sums_floats(Cn) or coef.numel() < loss_coef_floats(Cn) or loss4.numel() < 4:
        raise ValueError("lm_net_amd.segloss_ex_fwd: workspace too small for %d classes" % Cn)
    _check(load().lmn_segloss_ex_fwd(_p(logits), _pl(target), _p(w_ce), _p(w_dice), B, Cn, _i64(hw), C.byref(param), _p(sums), _p(coef),
                                     _p(loss4), _stream()), "segloss_ex_fwd")


def segloss_ex_bwd(logits, target, w_ce, coef, gscale, param, dlogits):
    """dlogits = gscale[0] * d total / d logits (gscale None: 1) from the coef of segloss_ex_fwd (lmn_segloss_ex_bwd)."""
    B, Cn, hw = _dims(logits)
    if coef.numel() < loss_coef_floats(Cn) or dlogits.numel() != logits.numel():
        raise ValueError("lm_net_amd.segloss_ex_bwd: coef or dlogits does not match %d classes" % Cn)
    _check(load().lmn_segloss_ex_bwd(_p(logits), _pl(target), _p(w_ce), _p(coef), _p(gscale), B, Cn, _i64(hw), C.byref(param), _p(dlogits),
                                     _stream()), "segloss_ex_bwd")


def image_stats(pred, target, n_classes, ignore_index, stats):
    """stats [B, C, 4] int64 = tp, fp, fn, tn per image and class (lmn_image_stats).  pred: fp32 logits [B, C, H, W] or a uint8 label
    map [B, H, W] (values >= C: no class); target int64 [B, H, W]; labels outside [0, C) are void."""
    B = target.shape[0]
    hw = target.numel() // B
    logits = pred if pred.dim() == 4 else None
    labels = pred if pred.dim() == 3 else None
    if (logits is None) == (labels is None) or pred.shape[0] != B or pred.numel() != target.numel() * (n_classes if labels is None else 1):
        raise ValueError("lm_net_amd.image_stats: pred %s does not match target %s with %d classes"
                         % (tuple(pred.shape), tuple(target.shape), n_classes))
    if logits is not None and not logits.is_contiguous():
        raise ValueError("lm_net_amd.image_stats: contiguous logits required")
    if stats.numel() != B * n_classes * 4:
        raise ValueError("lm_net_amd.image_stats: stats must hold [%d, %d, 4] int64" % (B, n_classes))
    _check(load().lmn_image_stats(_p(logits), _raw(labels, torch.uint8, "image_stats"), _pl(target), B, int(n_classes), _i64(hw),
                                  0 if ignore_index is None else 1, _i64(0 if ignore_index is None else ignore_index),
                                  _raw(stats, torch.int64, "image_stats"), _stream()), "image_stats")


def sig_param(smooth=1e-5, bce_scale=1.0, dice_scale=1.0, focal_scale=0.0, focal_gamma=2.0, focal_alpha=0.25, target_kind=SIG_T_I64):
    """A SigParam (lmn_sig_param_t) from Python values."""
    p = SigParam()
    p.smooth, p.bce_scale, p.dice_scale, p.focal_scale = float(smooth), float(bce_scale), float(dice_scale), float(focal_scale)
    p.focal_gamma, p.focal_alpha, p.target_kind = float(focal_gamma), float(focal_alpha), int(target_kind)
    return p


def sig_target_kind(target):
    """LMN_SIG_T_* of a target tensor: uint8 or int64."""
    if target.dtype == torch.uint8:
        return SIG_T_U8
    if target.dtype == torch.int64:
        return SIG_T_I64
    raise ValueError("lm_net_amd: sigmoid targets are uint8 or int64, got %s" % target.dtype)


def _logit_f32(thr):
    """log(thr / (1 - thr)) of thr in [0, 1], in float64, rounded once to fp32: -inf at 0, exactly 0 at 0.5, +inf at 1."""
    with np.errstate(divide="ignore"):
        return float(np.float32(np.log(np.float64(thr) / (1.0 - np.float64(thr)))))


def sig_logit_threshold(threshold):
    """log(thr / (1 - thr)) in float64, rounded to fp32: the logit at which sigmoid crosses thr (exactly 0 at 0.5)."""
    thr = float(threshold)
    if not 0.0 < thr < 1.0:
        raise ValueError("lm_net_amd: threshold = %g outside (0, 1)" % thr)
    return _logit_f32(thr)


def _sig_dims(logits, target, what):
    B, Cn = logits.shape[0], logits.shape[1]
    hw = logits.numel() // max(B * Cn, 1)
    if logits.dim() < 3 or not logits.is_contiguous():
        raise ValueError("lm_net_amd.%s: contiguous logits [B, C, ...] required" % what)
    if target is not None and (target.numel() != logits.numel() or not target.is_contiguous() or not target.is_cuda):
        raise ValueError("lm_net_amd.%s: target %s does not match logits %s (contiguous device tensor of the same size)"
                         % (what, tuple(target.shape), tuple(logits.shape)))
    return B, Cn, hw


def sigloss_fwd(logits, target, w_bce, pos_weight, w_dice, param, sums, coef, loss4):
    """loss4 = [total, bce, dice, focal] of fp32 logits [B, C, ...] against a uint8 / int64 target of the same size, every class a
    binary problem of its own (lmn_sigloss_fwd); param: a SigParam whose target_kind matches the target; sums: int32 workspace of at
    least sig_sums_words(C); coef: fp32 workspace of at least sig_coef_floats(C)."""
    B, Cn, hw = _sig_dims(logits, target, "sigloss_fwd")
    if param.target_kind != sig_target_kind(target):
        raise ValueError("lm_net_amd.sigloss_fwd: param.target_kind does not match the target's dtype %s" % target.dtype)
    if sums.numel() < sig_sums_words(Cn) or coef.numel() < sig_coef_floats(Cn) or loss4.numel() < 4:
        raise ValueError("lm_net_amd.sigloss_fwd: workspace too small for %d classes" % Cn)
    if min(w_bce.numel(), pos_weight.numel(), w_dice.numel()) < Cn:
        raise ValueError("lm_net_amd.sigloss_fwd: a weight vector is shorter than %d classes" % Cn)
    _check(load().lmn_sigloss_fwd(_p(logits), C.c_void_p(target.data_ptr()), _p(w_bce), _p(pos_weight), _p(w_dice), B, Cn, _i64(hw),
                                  C.byref(param), _raw(sums, torch.int32, "sigloss_fwd"), _p(coef), _p(loss4), _stream()), "sigloss_fwd")


def sigloss_bwd(logits, target, pos_weight, coef, gscale, param, dlogits):
    """dlogits = gscale[0] * d total / d logits (gscale None: 1) from the coef of sigloss_fwd (lmn_sigloss_bwd)."""
    B, Cn, hw = _sig_dims(logits, target, "sigloss_bwd")
    if param.target_kind != sig_target_kind(target):
        raise ValueError("lm_net_amd.sigloss_bwd: param.target_kind does not match the target's dtype %s" % target.dtype)
    if coef.numel() < sig_coef_floats(Cn) or dlogits.numel() != logits.numel() or pos_weight.numel() < Cn:
        raise ValueError("lm_net_amd.sigloss_bwd: coef, pos_weight or dlogits does not match %d classes" % Cn)
    _check(load().lmn_sigloss_bwd(_p(logits), C.c_void_p(target.data_ptr()), _p(pos_weight), _p(coef), _p(gscale), B, Cn, _i64(hw),
                                  C.byref(param), _p(dlogits), _stream()), "sigloss_bwd")


def sigmoid_stats(logits, target, logit_threshold, stats=None, labels_out=None):
    """Thresholded statistics and / or label maps of fp32 logits [B, C, ...] (lmn_sigmoid_stats): stats int64 [B, C, 4] = tp, fp, fn,
    tn over the valid elements (target 0 or 1) of each plane, overwritten; labels_out uint8 of the logits' size = (z >= logit_threshold).
    target: uint8 or int64 of the logits' size, or None for the label maps alone."""
    B, Cn, hw = _sig_dims(logits, target, "sigmoid_stats")
    if stats is None and labels_out is None:
        raise ValueError("lm_net_amd.sigmoid_stats: at least one of stats and labels_out must be given")
    if stats is not None and (target is None or stats.numel() != B * Cn * 4):
        raise ValueError("lm_net_amd.sigmoid_stats: stats needs a target and must hold [%d, %d, 4] int64" % (B, Cn))
    if labels_out is not None and labels_out.numel() != logits.numel():
        raise ValueError("lm_net_amd.sigmoid_stats: labels_out must hold one uint8 per logit")
    kind = SIG_T_U8 if target is None else sig_target_kind(target)
    _check(load().lmn_sigmoid_stats(_p(logits), None if target is None else C.c_void_p(target.data_ptr()), kind, _f(logit_threshold),
                                    B, Cn, _i64(hw), _raw(stats, torch.int64, "sigmoid_stats"),
                                    _raw(labels_out, torch.uint8, "sigmoid_stats"), _stream()), "sigmoid_stats")


def curve_thresholds(thresholds):
    """The thresholds of a curve as a float64 array.  An integer N in [2, 1024]: t_k = k / (N - 1), k = 0 .. N - 1 (torchmetrics'
    binned thresholds); a sequence: 1 .. 1024 non-decreasing values inside [0, 1].  Anything else raises ValueError."""
    if isinstance(thresholds, (int, np.integer)) and not isinstance(thresholds, bool):
        n = int(thresholds)
        if not 2 <= n <= CURVE_MAX_EDGES:
            raise ValueError("lm_net_amd.curve_edges: %d thresholds, expected 2 .. %d" % (n, CURVE_MAX_EDGES))
        return np.arange(n, dtype=np.float64) / np.float64(n - 1)
    try:
        t = np.array([float(v) for v in thresholds], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("lm_net_amd.curve_edges: thresholds must be an integer or a sequence of numbers, got %r" % (thresholds,))
    if not 1 <= t.size <= CURVE_MAX_EDGES:
        raise ValueError("lm_net_amd.curve_edges: %d thresholds, expected 1 .. %d" % (t.size, CURVE_MAX_EDGES))
    if not bool(np.all((t >= 0.0) & (t <= 1.0))) or bool(np.any(np.diff(t) < 0)):       # (a NaN fails the first test)
        raise ValueError("lm_net_amd.curve_edges: thresholds must be non-decreasing values inside [0, 1]")
    return t


def curve_edges(thresholds, kind):
    """The fp32 edge table of lmn_curve_hist (numpy) from thresholds (curve_thresholds).  kind "logit": each threshold through the
    arithmetic of sig_logit_threshold (0 -> -inf, 1 -> +inf), for logits scored as they are; kind "probability": np.float32(t)."""
    if kind not in ("logit", "probability"):
        raise ValueError("lm_net_amd.curve_edges: kind=%r, expected 'logit' or 'probability'" % (kind,))
    t = curve_thresholds(thresholds)
    if kind == "probability":
        return t.astype(np.float32)
    return np.array([_logit_f32(v) for v in t], dtype=np.float32)


def curve_workspace(score_kind, B, hw):
    """Bytes of scratch lmn_curve_hist needs: 0 for CURVE_RAW, 4 * B * hw for CURVE_SOFTMAX (host arithmetic, no GPU)."""
    return _host_size("curve_workspace", load().lmn_curve_workspace(int(score_kind), int(B), _i64(hw)))


def curve_hist(values, target, target_form, score_kind, edges, hist, workspace=None):
    """hist int64 [B, C, 2, n_edges + 1], overwritten: per (image, class) plane of fp32 values [B, C, ...] the histogram of the scores of
    the negative ([.., 0, :]) and the positive ([.., 1, :]) valid elements over the bins of the fp32 device table `edges`
    (lmn_curve_hist; bin = number of edges <= score).  target: uint8 or int64, of the values' size (CURVE_PLANES: 1 / 0 / void) or a
    label map [B, ...] (CURVE_LABELS); score_kind CURVE_SOFTMAX needs a uint8 workspace of curve_workspace(...) bytes."""
    B, Cn, hw = _sig_dims(values, None, "curve_hist")
    if target_form not in (CURVE_PLANES, CURVE_LABELS) or score_kind not in (CURVE_RAW, CURVE_SOFTMAX):
        raise ValueError("lm_net_amd.curve_hist: unknown target_form %r or score_kind %r" % (target_form, score_kind))
    n = edges.numel()
    if not 1 <= n <= CURVE_MAX_EDGES or hist.numel() != B * Cn * 2 * (n + 1):
        raise ValueError("lm_net_amd.curve_hist: %d edges (1 .. %d) need hist [%d, %d, 2, %d] int64, got %s"
                         % (n, CURVE_MAX_EDGES, B, Cn, n + 1, tuple(hist.shape)))
    if not target.is_cuda or not target.is_contiguous() or target.numel() != (values.numel() if target_form == CURVE_PLANES else B * hw):
        raise ValueError("lm_net_amd.curve_hist: target %s does not match values %s (contiguous device tensor, %s)"
                         % (tuple(target.shape), tuple(values.shape), "planes" if target_form == CURVE_PLANES else "a label map"))
    need = 4 * B * hw if score_kind == CURVE_SOFTMAX else 0
    if need and (workspace is None or workspace.numel() < need):
        raise ValueError("lm_net_amd.curve_hist: the softmax form needs a workspace of %d bytes" % need)
    _check(load().lmn_curve_hist(_p(values), C.c_void_p(target.data_ptr()), sig_target_kind(target), int(target_form), int(score_kind),
                                 _raw(edges, torch.float32, "curve_hist"), n, B, Cn, _i64(hw), _raw(workspace, torch.uint8, "curve_hist"),
                                 _raw(hist, torch.int64, "curve_hist"), _stream()), "curve_hist")


def surface_workspace(B, nk, H, W):
    """Bytes of scratch lmn_surface_dist needs for B samples x nk classes of H x W pixels (host arithmetic, no GPU)."""
    return _host_size("surface_workspace", load().lmn_surface_workspace(int(B), int(nk), int(H), int(W)))


def surface_dist(pred, target, n_classes, classes, workspace, stats_i, stats_f):
    """Raw surface-distance statistics of one batch (lmn_surface_dist).  pred: fp32 logits [B,C,H,W] or int64 labels [B,H,W];
    target int64 [B,H,W]; classes: the class ids scored (host list); workspace: uint8 device tensor of at least
    surface_workspace(B, len(classes), H, W) bytes; stats_i int64 [B,nk,8] and stats_f float64 [B,nk,2] device tensors."""
    nk = len(classes)
    B, H, W = target.shape
    for t, dt in ((workspace, torch.uint8), (stats_i, torch.int64), (stats_f, torch.float64)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError("lm_net_amd.surface_dist: contiguous %s device tensor required" % dt)
    if stats_i.numel() != B * nk * 8 or stats_f.numel() != B * nk * 2:
        raise ValueError("lm_net_amd.surface_dist: statistics buffers do not match B=%d, %d classes" % (B, nk))
    logits = pred if pred.dim() == 4 else None
    labels = pred if pred.dim() == 3 else None
    if (logits is None) == (labels is None) or tuple(pred.shape[-2:]) != (H, W) or pred.shape[0] != B:
        raise ValueError("lm_net_amd.surface_dist: pred %s does not match target %s" % (tuple(pred.shape), tuple(target.shape)))
    if logits is not None and (logits.shape[1] != n_classes or not logits.is_contiguous()):
        raise ValueError("lm_net_amd.surface_dist: contiguous logits with %d channels required" % n_classes)
    ids = (C.c_int32 * nk)(*[int(k) for k in classes])
    _check(load().lmn_surface_dist(_p(logits), _pl(labels), _pl(target), B, int(n_classes), H, W, ids, nk,
                                   C.c_void_p(workspace.data_ptr()), _i64(workspace.numel()), C.c_void_p(stats_i.data_ptr()),
                                   C.c_void_p(stats_f.data_ptr()), _stream()), "surface_dist")


def volume_workspace(D, H, W, nk):
    """Bytes of scratch lmn_volume_dist needs for nk classes of a D x H x W volume, exactly (host arithmetic, no GPU)."""
    return _host_size("volume_workspace", load().lmn_volume_workspace(int(D), int(H), int(W), int(nk)))


def volume_span(shape, spacing):
    """(kz (D-1))^2 + (ky (H-1))^2 + (kx (W-1))^2 of a volume [D, H, W] with integer pitches: the largest squared distance, which
    lmn_volume_dist requires below 2^31 (Python integers: no overflow)."""
    return sum((int(k) * (int(n) - 1)) ** 2 for k, n in zip(spacing, shape))


def _volume_case(lab_pred, lab_target, what):
    if lab_pred.dim() != 3 or lab_pred.shape != lab_target.shape:
        raise ValueError("lm_net_amd.%s: case buffers %s, %s: two uint8 volumes [D, H, W] of one shape required"
                         % (what, tuple(lab_pred.shape), tuple(lab_target.shape)))
    return tuple(int(d) for d in lab_pred.shape)


def volume_labels(pred, target, n_classes, lab_pred, lab_target, z0=0):
    """Narrow n slices of a case to uint8 class ids (255: no class) into slices [z0, z0 + n) of the case buffers lab_pred / lab_target
    (uint8 [D_cap, H, W] device tensors; lmn_volume_labels).  pred: fp32 logits [n, C, H, W] or int64 labels [n, H, W]; target int64
    [n, H, W]."""
    cap, H, W = _volume_case(lab_pred, lab_target, "volume_labels")
    logits = pred if pred.dim() == 4 else None
    labels = pred if pred.dim() == 3 else None
    n = int(target.shape[0])
    if (logits is None) == (labels is None) or target.dim() != 3 or tuple(pred.shape[-2:]) != (H, W) or tuple(target.shape[1:]) != (H, W) \
            or pred.shape[0] != n:
        raise ValueError("lm_net_amd.volume_labels: pred %s, target %s do not match case buffers of %dx%d slices"
                         % (tuple(pred.shape), tuple(target.shape), H, W))
    if logits is not None and (logits.shape[1] != n_classes or not logits.is_contiguous()):
        raise ValueError("lm_net_amd.volume_labels: contiguous logits with %d channels required" % n_classes)
    if n < 1 or z0 < 0 or z0 + n > cap:
        raise ValueError("lm_net_amd.volume_labels: slices [%d, %d) outside the case buffer of %d slices" % (z0, z0 + n, cap))
    _check(load().lmn_volume_labels(_p(logits), _pl(labels), _pl(target), n, int(n_classes), H, W, _raw(lab_pred, torch.uint8, "volume_labels"),
                                    _raw(lab_target, torch.uint8, "volume_labels"), cap, int(z0), _stream()), "volume_labels")


def volume_dist(lab_pred, lab_target, n_classes, classes, spacing, workspace, stats_i, stats_f):
    """Raw 3D surface-distance and overlap statistics of one case (lmn_volume_dist).  lab_pred / lab_target: uint8 [D, H, W] device
    tensors as volume_labels writes them; classes: the class ids scored (host list); spacing: integer pitches (kz, ky, kx); workspace:
    uint8 device tensor of at least volume_workspace(D, H, W, len(classes)) bytes; stats_i int64 [nk, 9] and stats_f float64 [nk, 2]
    device tensors."""
    D, H, W = _volume_case(lab_pred, lab_target, "volume_dist")
    nk = len(classes)
    if stats_i.numel() != nk * VOLUME_NSTAT_I or stats_f.numel() != nk * VOLUME_NSTAT_F:
        raise ValueError("lm_net_amd.volume_dist: statistics buffers do not match %d classes" % nk)
    if len(spacing) != 3 or any(int(k) != k or k < 1 for k in spacing):
        raise ValueError("lm_net_amd.volume_dist: spacing %r: three positive integers (kz, ky, kx) required" % (spacing,))
    ids = (C.c_int32 * nk)(*[int(k) for k in classes])
    _check(load().lmn_volume_dist(_raw(lab_pred, torch.uint8, "volume_dist"), _raw(lab_target, torch.uint8, "volume_dist"), D, H, W,
                                  int(n_classes), ids, nk, int(spacing[0]), int(spacing[1]), int(spacing[2]),
                                  _raw(workspace, torch.uint8, "volume_dist"), _i64(workspace.numel()), _raw(stats_i, torch.int64, "volume_dist"),
                                  _raw(stats_f, torch.float64, "volume_dist"), _stream()), "volume_dist")


def volpost_workspace(D, H, W):
    """Bytes of scratch lmn_volpost_clean needs for a D x H x W volume, exactly (host arithmetic, no GPU)."""
    return _host_size("volpost_workspace", load().lmn_volpost_workspace(int(D), int(H), int(W)))


def cc3d_label(labels, connectivity, roots, sizes):
    """Connected components of ONE uint8 label volume [D, H, W] under connectivity 6, 18 or 26 into int32 roots / sizes [D, H, W]
    (lmn_cc3d_label)."""
    if labels.dim() != 3 or roots.numel() != labels.numel() or sizes.numel() != labels.numel():
        raise ValueError("lm_net_amd.cc3d_label: roots / sizes do not match a label volume [D, H, W] (labels %s)" % (tuple(labels.shape),))
    D, H, W = (int(d) for d in labels.shape)
    _check(load().lmn_cc3d_label(_raw(labels, torch.uint8, "cc3d_label"), D, H, W, int(connectivity), _raw(roots, torch.int32, "cc3d_label"),
                                 _raw(sizes, torch.int32, "cc3d_label"), _stream()), "cc3d_label")


def volpost_clean(labels, n_classes, connectivity, class_mask, keep_largest, min_volume, hole_limit, workspace, labels_out, stats):
    """lmn_volpost_clean of ONE case: labels uint8 [D, H, W] (L0) -> labels_out uint8 [D, H, W] (L2) and stats int32 [C, 4].
    class_mask: bit k = class k is cleaned; keep_largest / min_volume: host sequences of C ints indexed by class; workspace: uint8 device
    tensor of at least volpost_workspace(D, H, W) bytes."""
    n = int(n_classes)
    if labels.dim() != 3 or labels_out.numel() != labels.numel() or stats.numel() != n * VOLPOST_NSTAT:
        raise ValueError("lm_net_amd.volpost_clean: output buffers do not match C=%d and a label volume [D, H, W] (labels %s)"
                         % (n, tuple(labels.shape)))
    if len(keep_largest) != n or len(min_volume) != n:
        raise ValueError("lm_net_amd.volpost_clean: keep_largest and min_volume need one entry per class (%d)" % n)
    D, H, W = (int(d) for d in labels.shape)
    keep = (C.c_int32 * n)(*[int(v) for v in keep_largest])
    minv = (C.c_int32 * n)(*[int(v) for v in min_volume])
    _check(load().lmn_volpost_clean(_raw(labels, torch.uint8, "volpost_clean"), D, H, W, n, int(connectivity), C.c_uint64(int(class_mask)),
                                    keep, minv, int(hole_limit), _raw(workspace, torch.uint8, "volpost_clean"), _i64(workspace.numel()),
                                    _raw(labels_out, torch.uint8, "volpost_clean"), _raw(stats, torch.int32, "volpost_clean"), _stream()),
           "volpost_clean")


def lesion_workspace(D, H, W):
    """Bytes of scratch lmn_lesion_match needs for a D x H x W volume, exactly (host arithmetic, no GPU)."""
    return _host_size("lesion_workspace", load().lmn_lesion_workspace(int(D), int(H), int(W)))


def lesion_match(pred, target, n_classes, connectivity, class_mask, workspace, comp_keys, comp_sizes, pair_keys, pair_counts, ctrl):
    """lmn_lesion_match of ONE case: pred / target uint8 [D, H, W] device tensors -> the component records comp_keys int64 [M] /
    comp_sizes int32 [M] (key = side << 40 | class << 32 | root), the pair table pair_keys int64 [S] / pair_counts int32 [S]
    (key = root_p << 32 | root_g; S a power of two in [64, 2^22]) and ctrl int32 [4] (lesions found, pairs stored, insertions that
    found the table full, 0).  Unused slots hold -1 / 0; the slot of a record depends on arrival order.  class_mask: bit k = class k
    is scored; workspace: uint8 device tensor of at least lesion_workspace(D, H, W) bytes."""
    if pred.dim() != 3 or pred.shape != target.shape:
        raise ValueError("lm_net_amd.lesion_match: pred %s, target %s: two uint8 volumes [D, H, W] of one shape required"
                         % (tuple(pred.shape), tuple(target.shape)))
    if comp_keys.dim() != 1 or comp_sizes.shape != comp_keys.shape or pair_keys.dim() != 1 or pair_counts.shape != pair_keys.shape \
            or ctrl.numel() != LESION_NCTRL:
        raise ValueError("lm_net_amd.lesion_match: record buffers %s / %s, %s / %s, ctrl %s: keys and sizes [M], keys and counts [S] and "
                         "ctrl [%d] required" % (tuple(comp_keys.shape), tuple(comp_sizes.shape), tuple(pair_keys.shape),
                                                 tuple(pair_counts.shape), tuple(ctrl.shape), LESION_NCTRL))
    D, H, W = (int(d) for d in pred.shape)
    _check(load().lmn_lesion_match(_raw(pred, torch.uint8, "lesion_match"), _raw(target, torch.uint8, "lesion_match"), D, H, W, int(n_classes),
                                   int(connectivity), C.c_uint64(int(class_mask)), _raw(workspace, torch.uint8, "lesion_match"),
                                   _i64(workspace.numel()), _raw(comp_keys, torch.int64, "lesion_match"),
                                   _raw(comp_sizes, torch.int32, "lesion_match"), int(comp_keys.numel()),
                                   _raw(pair_keys, torch.int64, "lesion_match"), _raw(pair_counts, torch.int32, "lesion_match"),
                                   int(pair_keys.numel()), _raw(ctrl, torch.int32, "lesion_match"), _stream()), "lesion_match")


# ---- what the wrappers of the three criteria (distance maps, Lovasz, region overlap) share
assert (DISTMAP_LABELS_U8, LOVASZ_LABELS_U8, REGION_LABELS_U8, DISTMAP_LABELS_I64, LOVASZ_LABELS_I64, REGION_LABELS_I64) == (0, 0, 0, 1, 1, 1)


def label_kind(t):
    """LMN_*_LABELS_U8 / _I64 (0 / 1 in each of the three headers) of a label or target tensor: uint8 or int64."""
    if t.dtype == torch.uint8:
        return 0
    if t.dtype == torch.int64:
        return 1
    raise ValueError("lm_net_amd: a uint8 or int64 target required, got %s" % t.dtype)


def _nk(class_mask):
    """the number of classes a class_mask scores"""
    return bin(int(class_mask) & (2 ** 64 - 1)).count("1")


def _loss_dims(what, logits, target, softmax):
    """(B, C, H, W) of contiguous logits [B, C, H, W] and their contiguous device target: a label map [B, H, W] under a softmax head,
    planes [B, C, H, W] under a sigmoid head."""
    if logits.dim() != 4 or not logits.is_contiguous():
        raise ValueError("lm_net_amd.%s: contiguous logits [B, C, H, W] required, got %s" % (what, tuple(logits.shape)))
    B, Cn, H, W = logits.shape
    want = (B, H, W) if softmax else (B, Cn, H, W)
    if tuple(target.shape) != want or not target.is_cuda or not target.is_contiguous():
        raise ValueError("lm_net_amd.%s: target %s, expected a contiguous device tensor %s" % (what, tuple(target.shape), want))
    return B, Cn, H, W


def dist_workspace(B, nk, H, W):
    """Bytes of scratch lmn_dist_map needs for B samples x nk classes of H x W pixels, exactly (host arithmetic, no GPU)."""
    return _host_size("dist_workspace", load().lmn_dist_workspace(int(B), int(nk), int(H), int(W)))


def dist_map(src, n_classes, class_mask, workspace, sd2, flags, mode=None, threshold=0.0):
    """sd2 int32 [B, nk, H, W] and flags int32 [B, nk] of the masks of the classes of class_mask (lmn_dist_map).  src: a uint8 / int64
    label map [B, H, W] (mode None), or fp32 logits [B, C, H, W] with mode DISTMAP_SOFTMAX (threshold: a probability) or
    DISTMAP_SIGMOID (threshold: a logit); workspace: uint8 device tensor of at least dist_workspace(B, nk, H, W) bytes."""
    nk = _nk(class_mask)
    from_logits = mode is not None
    if src.dim() != (4 if from_logits else 3) or not src.is_contiguous() or (from_logits and src.shape[1] != n_classes):
        want = "logits [B, %d, H, W]" % n_classes if from_logits else "labels [B, H, W]"
        raise ValueError("lm_net_amd.dist_map: src %s: contiguous %s required" % (tuple(src.shape), want))
    B, H, W = src.shape[0], src.shape[-2], src.shape[-1]
    if sd2.numel() != B * nk * H * W or flags.numel() != B * nk:
        raise ValueError("lm_net_amd.dist_map: sd2 %s / flags %s do not hold [%d, %d, %d, %d] / [%d, %d]"
                         % (tuple(sd2.shape), tuple(flags.shape), B, nk, H, W, B, nk))
    logits = _p(src) if from_logits else None
    labels = None if from_logits else _raw(src, src.dtype, "dist_map")
    kind = DISTMAP_LABELS_U8 if from_logits else label_kind(src)
    _check(load().lmn_dist_map(logits, labels, kind, _f(threshold), int(mode or 0), B, int(n_classes), H, W, C.c_uint64(int(class_mask)),
                               _raw(workspace, torch.uint8, "dist_map"), _i64(workspace.numel()), _raw(sd2, torch.int32, "dist_map"),
                               _raw(flags, torch.int32, "dist_map"), _stream()), "dist_map")


def _dist_loss_dims(what, logits, target, head, class_mask, sd2_g, sd2_p):
    B, Cn, H, W = _loss_dims(what, logits, target, head == DISTMAP_SOFTMAX)
    nk = _nk(class_mask)
    for m in (sd2_g, sd2_p):
        if m is not None and tuple(m.shape) != (B, nk, H, W):
            raise ValueError("lm_net_amd.%s: distance map %s, expected %s" % (what, tuple(m.shape), (B, nk, H, W)))
    return B, Cn, H, W


def dist_loss_fwd(logits, target, head, term, alpha, scale, class_mask, sd2_g, sd2_p, sums, loss):
    """loss[0] = scale * the boundary (DISTMAP_BOUNDARY, sd2_p None) or Hausdorff (DISTMAP_HAUSDORFF) term of fp32 logits [B, C, H, W]
    under a softmax head (target: label map [B, H, W]) or a sigmoid head (target: planes [B, C, H, W]), uint8 or int64, on the maps
    int32 [B, nk, H, W] of dist_map (lmn_dist_loss_fwd); sums: int32 workspace of DISTMAP_SUMS_WORDS words, read by dist_loss_bwd."""
    B, Cn, H, W = _dist_loss_dims("dist_loss_fwd", logits, target, head, class_mask, sd2_g, sd2_p)
    if sums.numel() < DISTMAP_SUMS_WORDS or loss.numel() < 1:
        raise ValueError("lm_net_amd.dist_loss_fwd: sums needs %d words and loss one float" % DISTMAP_SUMS_WORDS)
    _check(load().lmn_dist_loss_fwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(term), _f(alpha),
                                    _f(scale), B, Cn, H, W, C.c_uint64(int(class_mask)), _raw(sd2_g, torch.int32, "dist_loss_fwd"),
                                    _raw(sd2_p, torch.int32, "dist_loss_fwd"), _raw(sums, torch.int32, "dist_loss_fwd"), _p(loss),
                                    _stream()), "dist_loss_fwd")


def dist_loss_bwd(logits, target, head, term, alpha, class_mask, sd2_g, sd2_p, sums, gscale, dlogits):
    """dlogits = gscale[0] * d loss / d logits (gscale None: 1) from the sums of dist_loss_fwd on the same arguments
    (lmn_dist_loss_bwd); every element of dlogits is written."""
    B, Cn, H, W = _dist_loss_dims("dist_loss_bwd", logits, target, head, class_mask, sd2_g, sd2_p)
    if sums.numel() < DISTMAP_SUMS_WORDS or tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous():
        raise ValueError("lm_net_amd.dist_loss_bwd: sums needs %d words and dlogits the logits' shape" % DISTMAP_SUMS_WORDS)
    _check(load().lmn_dist_loss_bwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(term), _f(alpha),
                                    B, Cn, H, W, C.c_uint64(int(class_mask)), _raw(sd2_g, torch.int32, "dist_loss_bwd"),
                                    _raw(sd2_p, torch.int32, "dist_loss_bwd"), _raw(sums, torch.int32, "dist_loss_bwd"), _p(gscale),
                                    _p(dlogits), _stream()), "dist_loss_bwd")


def lovasz_workspace(S, P):
    """Bytes of scratch lmn_lovasz_order / lmn_lovasz_fwd need for S segments of P elements, exactly (host arithmetic, no GPU)."""
    return _host_size("lovasz_workspace", load().lmn_lovasz_workspace(int(S), _i64(P)))


def lovasz_order(keys, workspace, perm):
    """perm int32 [S, P]: the stable ascending order of every row of keys [S, P] (lmn_lovasz_order): perm[s][r] is the index of the
    r-th smallest key of row s, ties by index ascending.  keys: an int32 device tensor whose bits are read as uint32; workspace: uint8
    device tensor of at least lovasz_workspace(S, P) bytes."""
    if keys.dim() != 2 or tuple(perm.shape) != tuple(keys.shape):
        raise ValueError("lm_net_amd.lovasz_order: keys %s and perm %s must both be [S, P]" % (tuple(keys.shape), tuple(perm.shape)))
    S, P = keys.shape
    _check(load().lmn_lovasz_order(_raw(keys, torch.int32, "lovasz_order"), int(S), _i64(P), _raw(workspace, torch.uint8, "lovasz_order"),
                                   _i64(workspace.numel()), _raw(perm, torch.int32, "lovasz_order"), _stream()), "lovasz_order")


def lovasz_segments(B, nk, H, W, per_image):
    """(S, P) of a batch: one segment per scored class over the batch's pixels, or per (image, class) with per_image."""
    return (B * nk, H * W) if per_image else (nk, B * H * W)


def _lovasz_dims(what, logits, target, head, class_mask, coef):
    B, Cn, H, W = _loss_dims(what, logits, target, head == LOVASZ_SOFTMAX)
    nk = _nk(class_mask)
    if tuple(coef.shape) != (B, nk, H, W):
        raise ValueError("lm_net_amd.%s: coef %s, expected %s" % (what, tuple(coef.shape), (B, nk, H, W)))
    return B, Cn, H, W, nk


def lovasz_fwd(logits, target, head, per_image, present, class_mask, scale, workspace, errors, perm, counts, coef, sums, loss):
    """loss[0] = scale * the Lovasz-Softmax loss (LOVASZ_SOFTMAX: target a label map [B, H, W]) or the Lovasz hinge (LOVASZ_SIGMOID:
    target planes [B, C, H, W]) of fp32 logits [B, C, H, W] over the classes of class_mask (lmn_lovasz_fwd).  With (S, P) =
    lovasz_segments(...): errors fp32 [S, P], perm int32 [S, P], counts int32 [S, 2], coef fp32 [B, nk, H, W], sums int32 workspace of
    LOVASZ_SUMS_WORDS words (read by lovasz_bwd), workspace uint8 of at least lovasz_workspace(S, P) bytes."""
    B, Cn, H, W, nk = _lovasz_dims("lovasz_fwd", logits, target, head, class_mask, coef)
    S, P = lovasz_segments(B, nk, H, W, per_image)
    if tuple(errors.shape) != (S, P) or tuple(perm.shape) != (S, P) or tuple(counts.shape) != (S, 2):
        raise ValueError("lm_net_amd.lovasz_fwd: errors %s / perm %s / counts %s do not hold [%d, %d] / [%d, %d] / [%d, 2]"
                         % (tuple(errors.shape), tuple(perm.shape), tuple(counts.shape), S, P, S, P, S))
    if sums.numel() < LOVASZ_SUMS_WORDS or loss.numel() < 1:
        raise ValueError("lm_net_amd.lovasz_fwd: sums needs %d words and loss one float" % LOVASZ_SUMS_WORDS)
    _check(load().lmn_lovasz_fwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(bool(per_image)),
                                 int(bool(present)), _f(scale), B, Cn, H, W, C.c_uint64(int(class_mask)),
                                 _raw(workspace, torch.uint8, "lovasz_fwd"), _i64(workspace.numel()), _raw(errors, torch.float32, "lovasz_fwd"),
                                 _raw(perm, torch.int32, "lovasz_fwd"), _raw(counts, torch.int32, "lovasz_fwd"),
                                 _raw(coef, torch.float32, "lovasz_fwd"), _raw(sums, torch.int32, "lovasz_fwd"), _p(loss), _stream()),
           "lovasz_fwd")


def lovasz_bwd(logits, target, head, class_mask, coef, sums, gscale, dlogits):
    """dlogits = gscale[0] * d loss / d logits (gscale None: 1) from the coef and sums of lovasz_fwd on the same arguments
    (lmn_lovasz_bwd); every element of dlogits is written."""
    B, Cn, H, W, nk = _lovasz_dims("lovasz_bwd", logits, target, head, class_mask, coef)
    if sums.numel() < LOVASZ_SUMS_WORDS or tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous():
        raise ValueError("lm_net_amd.lovasz_bwd: sums needs %d words and dlogits the logits' shape" % LOVASZ_SUMS_WORDS)
    _check(load().lmn_lovasz_bwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), B, Cn, H, W,
                                 C.c_uint64(int(class_mask)), _raw(coef, torch.float32, "lovasz_bwd"), _raw(sums, torch.int32, "lovasz_bwd"),
                                 _p(gscale), _p(dlogits), _stream()), "lovasz_bwd")


def region_workspace(head, B, Cn, H, W, class_mask):
    """Bytes of the deterministic-mode slots of lmn_region_fwd, exactly (host arithmetic, no GPU)."""
    return _host_size("region_workspace", load().lmn_region_workspace(int(head), int(B), int(Cn), int(H), int(W), C.c_uint64(int(class_mask))))


def _region_dims(what, logits, target, head, per_image, class_mask, coef):
    B, Cn, H, W = _loss_dims(what, logits, target, head == REGION_SOFTMAX)
    nk = _nk(class_mask)
    G = B if per_image else 1
    if tuple(coef.shape) != (G, nk, 3):
        raise ValueError("lm_net_amd.%s: coef %s, expected %s" % (what, tuple(coef.shape), (G, nk, 3)))
    return B, Cn, H, W, G, nk


def region_fwd(logits, target, head, kind, denominator, per_image, alpha, beta, smooth, exponent, scale, class_mask, weight, workspace,
               sums, counts, coef, per_class, loss):
    """loss[0] = the region-overlap loss (lmn_region_fwd) of fp32 logits [B, C, H, W] under REGION_SOFTMAX (target a label map
    [B, H, W]) or REGION_SIGMOID (target planes [B, C, H, W]) over the classes of class_mask.  With G = B (per_image) or 1: sums fp32
    [G, nk, 3] (I, P1, P2), counts int32 [G, nk, 2] (T, N), coef fp32 [G, nk, 3] (read by region_bwd), per_class fp32 [G, nk]; weight
    fp32 [nk] or None; workspace uint8 of at least region_workspace(...) bytes (None outside deterministic mode)."""
    B, Cn, H, W, G, nk = _region_dims("region_fwd", logits, target, head, per_image, class_mask, coef)
    if tuple(sums.shape) != (G, nk, 3) or tuple(counts.shape) != (G, nk, 2) or tuple(per_class.shape) != (G, nk) or loss.numel() < 1:
        raise ValueError("lm_net_amd.region_fwd: sums %s / counts %s / per_class %s do not hold [%d, %d, 3] / [%d, %d, 2] / [%d, %d]"
                         % (tuple(sums.shape), tuple(counts.shape), tuple(per_class.shape), G, nk, G, nk, G, nk))
    if weight is not None and weight.numel() != nk:
        raise ValueError("lm_net_amd.region_fwd: weight holds %d values for %d scored classes" % (weight.numel(), nk))
    _check(load().lmn_region_fwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(kind), int(denominator),
                                 int(bool(per_image)), _f(alpha), _f(beta), _f(smooth), _f(exponent), _f(scale), B, Cn, H, W,
                                 C.c_uint64(int(class_mask)), _raw(weight, torch.float32, "region_fwd"), _raw(workspace, torch.uint8, "region_fwd"),
                                 _i64(0 if workspace is None else workspace.numel()), _raw(sums, torch.float32, "region_fwd"),
                                 _raw(counts, torch.int32, "region_fwd"), _raw(coef, torch.float32, "region_fwd"),
                                 _raw(per_class, torch.float32, "region_fwd"), _p(loss), _stream()), "region_fwd")


def region_bwd(logits, target, head, per_image, class_mask, coef, gscale, dlogits):
    """dlogits = gscale[0] * d loss / d logits (gscale None: 1) from the coef of region_fwd on the same arguments (lmn_region_bwd);
    every element of dlogits is written."""
    B, Cn, H, W, G, nk = _region_dims("region_bwd", logits, target, head, per_image, class_mask, coef)
    if tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous():
        raise ValueError("lm_net_amd.region_bwd: dlogits needs the logits' shape")
    _check(load().lmn_region_bwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(bool(per_image)), B, Cn,
                                 H, W, C.c_uint64(int(class_mask)), _raw(coef, torch.float32, "region_bwd"), _p(gscale), _p(dlogits), _stream()),
           "region_bwd")


def soft_workspace(reader, head, B, Cn, H, W):
    """Bytes of the deterministic-mode slots of lmn_soft_fwd, exactly (host arithmetic, no GPU)."""
    return _host_size("soft_workspace", load().lmn_soft_workspace(int(reader), int(head), int(B), int(Cn), int(H), int(W)))


def _soft_args(what, logits, reader, head, target, ya, yb, lam):
    """The checked tensors of lmn_soft_fwd / _bwd -> (B, C, H, W, label kind)."""
    if logits.dim() != 4 or not logits.is_contiguous():
        raise ValueError("lm_net_amd.%s: contiguous logits [B, C, H, W] required, got %s" % (what, tuple(logits.shape)))
    B, Cn, H, W = logits.shape
    full, lab = (B, Cn, H, W), ((B, H, W) if head == SOFT_SOFTMAX else (B, Cn, H, W))
    dev = lambda t: t.is_cuda and t.is_contiguous()
    if reader == SOFT_PAIR:
        if target is not None or ya is None or yb is None or lam is None:
            raise ValueError("lm_net_amd.%s: the pair reader takes ya, yb and lam and no target" % what)
        if tuple(ya.shape) != lab or tuple(yb.shape) != lab or ya.dtype != yb.dtype or not dev(ya) or not dev(yb):
            raise ValueError("lm_net_amd.%s: ya %s %s / yb %s %s, expected two contiguous device label maps %s of one type"
                             % (what, ya.dtype, tuple(ya.shape), yb.dtype, tuple(yb.shape), lab))
        if lam.dtype != torch.float32 or tuple(lam.shape) != (B,) or not dev(lam):
            raise ValueError("lm_net_amd.%s: lam must be a contiguous fp32 device tensor [%d]" % (what, B))
    else:
        want = {SOFT_PROBS: torch.float32, SOFT_TEACHER_F32: torch.float32, SOFT_TEACHER_BF16: torch.bfloat16}.get(reader)
        if want is None:
            raise ValueError("lm_net_amd.%s: unknown reader %r" % (what, reader))
        if target is None or target.dtype != want or tuple(target.shape) != full or not dev(target):
            raise ValueError("lm_net_amd.%s: reader %d takes a contiguous %s device target %s" % (what, reader, want, full))
        if yb is not None or lam is not None or (reader == SOFT_PROBS and ya is not None):
            raise ValueError("lm_net_amd.%s: reader %d takes neither yb nor lam (and the probability reader no label map)" % (what, reader))
        if ya is not None and (tuple(ya.shape) != lab or not dev(ya)):
            raise ValueError("lm_net_amd.%s: the valid map %s, expected a contiguous device tensor %s" % (what, tuple(ya.shape), lab))
    return B, Cn, H, W, (SOFT_LABELS_U8 if ya is None else label_kind(ya))


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def soft_fwd(logits, reader, head, target, ya, yb, lam, temperature, eps, smooth, ce_scale, dice_scale, w_ce, w_dice, workspace, sums,
             counts, coef, terms):
    """terms[0:3] = the soft-target loss and its terms (lmn_soft_fwd) of fp32 logits [B, C, H, W].  reader SOFT_PROBS: target fp32 q
    [B, C, H, W]; SOFT_PAIR: label maps ya, yb [B, H, W] and lam fp32 [B]; SOFT_TEACHER_F32 / _BF16: target the teacher's logits, ya
    an optional valid map (a label map under SOFT_SOFTMAX, planes under SOFT_SIGMOID), ce_scale the factor of the term.  sums fp32
    [1 + 3 C], counts int32 [1], coef fp32 [1 + 2 C] (read by soft_bwd), terms fp32 [3]; w_ce / w_dice fp32 [C] or None; workspace
    uint8 of at least soft_workspace(...) bytes (None outside deterministic mode)."""
    B, Cn, H, W, kind = _soft_args("soft_fwd", logits, reader, head, target, ya, yb, lam)
    if sums.numel() != 1 + 3 * Cn or counts.numel() != 1 or coef.numel() != 1 + 2 * Cn or terms.numel() != 3:
        raise ValueError("lm_net_amd.soft_fwd: sums %d / counts %d / coef %d / terms %d values, expected %d / 1 / %d / 3"
                         % (sums.numel(), counts.numel(), coef.numel(), terms.numel(), 1 + 3 * Cn, 1 + 2 * Cn))
    for w in (w_ce, w_dice):
        if w is not None and w.numel() != Cn:
            raise ValueError("lm_net_amd.soft_fwd: a class weight holds %d values for %d classes" % (w.numel(), Cn))
    f32 = torch.float32
    _check(load().lmn_soft_fwd(_p(logits), int(reader), int(head), _vp(target), _vp(ya), _vp(yb), kind, _raw(lam, f32, "soft_fwd"),
                               _f(temperature), _f(eps), _f(smooth), _f(ce_scale), _f(dice_scale), B, Cn, H, W, _raw(w_ce, f32, "soft_fwd"),
                               _raw(w_dice, f32, "soft_fwd"), _raw(workspace, torch.uint8, "soft_fwd"),
                               _i64(0 if workspace is None else workspace.numel()), _raw(sums, f32, "soft_fwd"),
                               _raw(counts, torch.int32, "soft_fwd"), _raw(coef, f32, "soft_fwd"), _raw(terms, f32, "soft_fwd"), _stream()),
           "soft_fwd")


def soft_bwd(logits, reader, head, target, ya, yb, lam, temperature, eps, w_ce, coef, gscale, dlogits):
    """dlogits = gscale[0] * d loss / d logits (gscale None: 1) from the coef of soft_fwd on the same arguments (lmn_soft_bwd); every
    element of dlogits is written."""
    B, Cn, H, W, kind = _soft_args("soft_bwd", logits, reader, head, target, ya, yb, lam)
    if tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous() or coef.numel() != 1 + 2 * Cn:
        raise ValueError("lm_net_amd.soft_bwd: dlogits needs the logits' shape and coef %d values" % (1 + 2 * Cn))
    f32 = torch.float32
    _check(load().lmn_soft_bwd(_p(logits), int(reader), int(head), _vp(target), _vp(ya), _vp(yb), kind, _raw(lam, f32, "soft_bwd"),
                               _f(temperature), _f(eps), B, Cn, H, W, _raw(w_ce, f32, "soft_bwd"), _raw(coef, f32, "soft_bwd"), _p(gscale),
                               _p(dlogits), _stream()), "soft_bwd")


def hard_workspace(head, per_image, B, Cn, H, W):
    """Bytes of the histograms, counts and slots of lmn_hard_fwd, exactly (host arithmetic, no GPU)."""
    return _host_size("hard_workspace", load().lmn_hard_workspace(int(head), int(bool(per_image)), int(B), int(Cn), int(H), int(W)))


def hard_cut(thresh):
    """The fp32 value cut of a probability threshold: float32(-log(thresh)), the logarithm taken in double; -1 (not given) for None."""
    if thresh is None:
        return -1.0
    return float(np.float32(-np.log(np.float64(thresh)))) + 0.0


def _hard_dims(what, logits, target, head, per_image, weight, values, selection):
    B, Cn, H, W = _loss_dims(what, logits, target, head == HARD_SOFTMAX)
    G = B if per_image else 1
    want = (B, H, W) if head == HARD_SOFTMAX else (B, Cn, H, W)
    if tuple(values.shape) != want or not values.is_contiguous() or tuple(selection.shape) != (G, HARD_RECORD_WORDS):
        raise ValueError("lm_net_amd.%s: values %s / selection %s do not hold %s / [%d, %d]"
                         % (what, tuple(values.shape), tuple(selection.shape), want, G, HARD_RECORD_WORDS))
    if weight is not None and weight.numel() != Cn:
        raise ValueError("lm_net_amd.%s: weight holds %d values for %d classes" % (what, weight.numel(), Cn))
    return B, Cn, H, W, G


def hard_fwd(logits, target, head, per_image, keep, min_kept, cut, scale, weight, workspace, values, selection, terms, loss):
    """loss[0] = the hard-pixel loss (lmn_hard_fwd) of fp32 logits [B, C, H, W] under HARD_SOFTMAX (target a label map [B, H, W]) or
    HARD_SIGMOID (target planes [B, C, H, W]).  keep in [0, 1] (0: not given), min_kept >= 0, cut = hard_cut(thresh).  With G = B
    (per_image) or 1: values fp32 [B, H, W] (sigmoid: [B, C, H, W]; -1 at a void element), selection int32 [G, HARD_RECORD_WORDS]
    (N, K, n_gt, n_eq, the bits of tau), terms fp32 [G]; weight fp32 [C] or None; workspace uint8 of at least hard_workspace(...)
    bytes."""
    B, Cn, H, W, G = _hard_dims("hard_fwd", logits, target, head, per_image, weight, values, selection)
    if terms.numel() != G or loss.numel() < 1:
        raise ValueError("lm_net_amd.hard_fwd: terms needs %d floats and loss one" % G)
    _check(load().lmn_hard_fwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(bool(per_image)), float(keep),
                               int(min_kept), float(cut), float(scale), B, Cn, H, W, _raw(weight, torch.float32, "hard_fwd"),
                               _raw(workspace, torch.uint8, "hard_fwd"), workspace.numel(), _raw(values, torch.float32, "hard_fwd"),
                               _raw(selection, torch.int32, "hard_fwd"), _raw(terms, torch.float32, "hard_fwd"), _p(loss), _stream()),
           "hard_fwd")


def hard_bwd(logits, target, head, per_image, scale, weight, values, selection, gscale, dlogits):
    """dlogits = gscale[0] * d loss / d logits (gscale None: 1) from the values and the selection of hard_fwd on the same arguments
    (lmn_hard_bwd); every element of dlogits is written."""
    B, Cn, H, W, G = _hard_dims("hard_bwd", logits, target, head, per_image, weight, values, selection)
    if tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous():
        raise ValueError("lm_net_amd.hard_bwd: dlogits needs the logits' shape")
    _check(load().lmn_hard_bwd(_p(logits), C.c_void_p(target.data_ptr()), label_kind(target), int(head), int(bool(per_image)), float(scale),
                               B, Cn, H, W, _raw(weight, torch.float32, "hard_bwd"), _raw(values, torch.float32, "hard_bwd"),
                               _raw(selection, torch.int32, "hard_bwd"), _p(gscale), _p(dlogits), _stream()), "hard_bwd")


def mix_rows(partner, mode, lam, boxes):
    """The host table of lmn_mix_batch: int32 [B, MIX_ROW_WORDS] = partner, mode, lam, 1 - lam (both as fp32 bits; the difference is
    formed in fp32 here, on the host), y0, x0, y1, x1."""
    lam = np.asarray(lam, dtype=np.float32).reshape(-1)
    rows = np.zeros((lam.size, MIX_ROW_WORDS), dtype=np.int32)
    rows[:, 0], rows[:, 1] = np.asarray(partner, dtype=np.int32), np.asarray(mode, dtype=np.int32)
    rows[:, 2], rows[:, 3] = lam.view(np.int32), (np.float32(1.0) - lam).astype(np.float32).view(np.int32)
    rows[:, 4:] = np.asarray(boxes, dtype=np.int32).reshape(lam.size, 4)
    return rows


def mix_batch(x, y, rows, rows_dev, x_out, ya_out, yb_out, lam_out):
    """Mixup / CutMix of a device batch through lmn_mix_batch: x fp32 [B, Cin, H, W] and y uint8 / int64 [B, H, W] -> x_out, ya_out,
    yb_out (None when no row is a mixup row) and lam_out fp32 [B], out of place.  rows: the host table of mix_rows; rows_dev: int32
    device tensor [B, MIX_ROW_WORDS] that receives it."""
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("lm_net_amd.mix_batch: contiguous x [B, Cin, H, W] required, got %s" % (tuple(x.shape),))
    B, Cin, H, W = x.shape
    rows = np.ascontiguousarray(rows, dtype=np.int32)            # (kept alive across the call)
    labels = [t for t in (y, ya_out, yb_out) if t is not None]
    if (tuple(rows.shape) != (B, MIX_ROW_WORDS) or rows_dev.numel() != B * MIX_ROW_WORDS or tuple(x_out.shape) != tuple(x.shape)
            or not x_out.is_contiguous() or lam_out.numel() != B or y is None or ya_out is None
            or any(tuple(t.shape) != (B, H, W) or t.dtype != y.dtype or not t.is_cuda or not t.is_contiguous() for t in labels)):
        raise ValueError("lm_net_amd.mix_batch: tensor sizes or types do not match B=%d, %d channel(s), %dx%d" % (B, Cin, H, W))
    _check(load().lmn_mix_batch(_p(x), _vp(y), label_kind(y), rows.ctypes.data_as(C.POINTER(C.c_int32)), _raw(rows_dev, torch.int32, "mix_batch"),
                                B, Cin, H, W, _p(x_out), _vp(ya_out), _vp(yb_out), _p(lam_out), _stream()), "mix_batch")


def slices_workspace(M, D, Hs, Ws):
    """Bytes of the workspace of lmn_slices_stats for M modalities of D x Hs x Ws voxels, exactly (host arithmetic, no GPU)."""
    return _host_size("slices_workspace", load().lmn_slices_workspace(int(M), int(D), int(Hs), int(Ws)))


def _slices_volume(what, volume):
    """(vol_kind, M, D, Hs, Ws) of a contiguous int16 or uint8 device volume [M, D, Hs, Ws]"""
    if volume.dim() != 4 or volume.dtype not in (torch.int16, torch.uint8) or not volume.is_cuda or not volume.is_contiguous():
        raise ValueError("lm_net_amd.%s: a contiguous int16 or uint8 device volume [M, D, Hs, Ws] required, got %s %s"
                         % (what, volume.dtype, tuple(volume.shape)))
    return (SLICES_I16 if volume.dtype == torch.int16 else SLICES_U8,) + tuple(int(d) for d in volume.shape)


def slices_stats(volume, foreground, q_lo_ppm, q_hi_ppm, specs, workspace, stats, table):
    """stats int64 [M, 8] (n, sum v, sum v^2, min, max, v_lo, v_hi, 0) and table fp32 [S, 4] (lo, hi, a, b) of an int16 / uint8
    volume [M, D, Hs, Ws] (lmn_slices_stats).  foreground: M ints (SLICES_NO_FOREGROUND: every voxel); q_*_ppm: the two ranks in parts
    per million; specs: S tuples (modality, SLICES_WINDOW / _ZSCORE / _PERCENTILE, level, width), modalities not decreasing;
    workspace: uint8 device tensor of at least slices_workspace(...) bytes."""
    kind, M, D, Hs, Ws = _slices_volume("slices_stats", volume)
    S = len(specs)
    if len(foreground) != M or tuple(stats.shape) != (M, SLICES_NSTAT) or tuple(table.shape) != (S, 4):
        raise ValueError("lm_net_amd.slices_stats: foreground (%d) / stats %s / table %s do not hold %d / [%d, %d] / [%d, 4]"
                         % (len(foreground), tuple(stats.shape), tuple(table.shape), M, M, SLICES_NSTAT, S))
    fg = (C.c_int32 * M)(*[int(v) for v in foreground])
    mod, knd = (C.c_int32 * max(S, 1))(*[int(s[0]) for s in specs]), (C.c_int32 * max(S, 1))(*[int(s[1]) for s in specs])
    lev, wid = (C.c_double * max(S, 1))(*[float(s[2]) for s in specs]), (C.c_double * max(S, 1))(*[float(s[3]) for s in specs])
    _check(load().lmn_slices_stats(C.c_void_p(volume.data_ptr()), kind, M, D, Hs, Ws, fg, int(q_lo_ppm), int(q_hi_ppm), S, mod, knd, lev, wid,
                                   _raw(workspace, torch.uint8, "slices_stats"), _i64(workspace.numel()),
                                   _raw(stats, torch.int64, "slices_stats"), _p(table), _stream()), "slices_stats")


def slices_gather(volume, labels, z, params, table, spec_mod, context, stride, edge, border, border_value, label_border, x, y):
    """x fp32 [n, S * (2 context + 1), h, w] from an int16 / uint8 volume [M, D, Hs, Ws] and / or y uint8 / int64 [n, h, w] from uint8
    labels [D, Hs, Ws], at the slices z (device int32 [n]) under the rows params (device fp32 [n, 8]: the inverse map m0 .. m5, gain,
    bias) (lmn_slices_gather).  table: fp32 [S, 4] of slices_stats; spec_mod: the modality of each of its rows; border_value: M
    floats.  volume, table and x None: label-only mode."""
    what = "slices_gather"
    if (volume is None) != (x is None) or (labels is None) != (y is None) or (volume is None and labels is None):
        raise ValueError("lm_net_amd.slices_gather: a volume needs x, labels need y, and one of the two is required")
    if labels is not None and (labels.dim() != 3 or labels.dtype != torch.uint8 or not labels.is_cuda or not labels.is_contiguous()):
        raise ValueError("lm_net_amd.slices_gather: contiguous uint8 device labels [D, Hs, Ws] required, got %s %s" % (labels.dtype, tuple(labels.shape)))
    if volume is not None:
        kind, M, D, Hs, Ws = _slices_volume(what, volume)
        if labels is not None and tuple(labels.shape) != (D, Hs, Ws):
            raise ValueError("lm_net_amd.slices_gather: labels %s beside a volume %s" % (tuple(labels.shape), tuple(volume.shape)))
    else:
        kind, M, (D, Hs, Ws) = SLICES_I16, 1, (int(d) for d in labels.shape)
    n = int(z.numel())
    S = 0 if volume is None else len(spec_mod)
    K = 2 * int(context) + 1
    dst = x if x is not None else y
    h, w = int(dst.shape[-2]), int(dst.shape[-1])
    if tuple(params.shape) != (n, 8) or (x is not None and tuple(x.shape) != (n, S * K, h, w)) or (y is not None and tuple(y.shape) != (n, h, w)):
        raise ValueError("lm_net_amd.slices_gather: params %s / x %s / y %s do not hold [%d, 8] / [%d, %d, %d, %d] / [%d, %d, %d]"
                         % (tuple(params.shape), None if x is None else tuple(x.shape), None if y is None else tuple(y.shape), n, n, S * K, h, w,
                            n, h, w))
    if volume is not None and (tuple(table.shape) != (S, 4) or len(border_value) != M):
        raise ValueError("lm_net_amd.slices_gather: table %s / border_value (%d) do not hold [%d, 4] / %d" % (tuple(table.shape), len(border_value), S, M))
    mod = None if volume is None else (C.c_int32 * max(S, 1))(*[int(v) for v in spec_mod])
    bv = None if volume is None else (C.c_float * M)(*[float(v) for v in border_value])
    _check(load().lmn_slices_gather(None if volume is None else C.c_void_p(volume.data_ptr()), kind, _raw(labels, torch.uint8, what), M, D, Hs, Ws,
                                    _raw(z, torch.int32, what), _p(params), n, _p(table), S, mod, int(context), int(stride), int(edge), int(border),
                                    bv, int(label_border), h, w, _p(x), None if y is None else _raw(y, y.dtype, what),
                                    0 if y is None else label_kind(y), _stream()), what)


def _raw(t, dt, what):
    """device pointer of a contiguous tensor of dtype dt (None passes through)"""
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
        raise RuntimeError("lm_net_amd.%s: contiguous %s device tensor required" % (what, dt))
    return C.c_void_p(t.data_ptr())


def confusion_labels(pred, target, counts):
    """counts[t*C + p] += pixels with label t and prediction p, for a uint8 label-map prediction [B,H,W] (lmn_confusion_labels).
    Float cells, as confusion(): 2^24 pixels or more in one call are refused."""
    B = pred.shape[0]
    hw = pred.numel() // B
    if target.numel() != pred.numel():
        raise ValueError("lm_net_amd.confusion_labels: pred %s does not match target %s" % (tuple(pred.shape), tuple(target.shape)))
    n = int(counts.shape[0])
    if counts.numel() != n * n:
        raise ValueError("lm_net_amd.confusion_labels: counts %s is not a square [C, C] matrix" % (tuple(counts.shape),))
    _check(load().lmn_confusion_labels(_raw(pred, torch.uint8, "confusion_labels"), _pl(target), B, n, _i64(hw), _p(counts), _stream()),
           "confusion_labels")


def post_workspace(B, H, W):
    """Bytes of scratch lmn_post_clean needs for B samples of H x W pixels (host arithmetic, no GPU)."""
    return _host_size("post_workspace", load().lmn_post_workspace(int(B), int(H), int(W)))


def cc_label(labels, connectivity, roots, areas):
    """Connected components of uint8 label maps [B,H,W] into int32 roots / areas [B,H,W] (lmn_cc_label)."""
    B, H, W = labels.shape
    if roots.numel() != labels.numel() or areas.numel() != labels.numel():
        raise ValueError("lm_net_amd.cc_label: roots / areas do not match labels %s" % (tuple(labels.shape),))
    _check(load().lmn_cc_label(_raw(labels, torch.uint8, "cc_label"), B, H, W, int(connectivity), None, _i64(0),
                               _raw(roots, torch.int32, "cc_label"), _raw(areas, torch.int32, "cc_label"), _stream()), "cc_label")


def post_clean(pred, n_classes, params, workspace, labels_out, stats):
    """lmn_post_clean: pred = fp32 logits [B,C,H,W] or a uint8 / int64 label map [B,H,W]; params: PostParam (host); workspace uint8
    of at least post_workspace(B, H, W) bytes; labels_out uint8 [B,H,W]; stats int32 [B,C,4].  With nothing cleaned or filled in params,
    workspace and stats may be None: labels_out is then the arg-max / clamped map L0 alone (one kernel)."""
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    logits = l8 = l64 = None
    if pred.dim() == 4 and pred.dtype == torch.float32:
        if pred.shape[1] != n_classes:
            raise ValueError("lm_net_amd.post_clean: logits with %d channels, n_classes = %d" % (pred.shape[1], n_classes))
        logits = _raw(pred, torch.float32, "post_clean")
    elif pred.dim() == 3 and pred.dtype == torch.uint8:
        l8 = _raw(pred, torch.uint8, "post_clean")
    elif pred.dim() == 3 and pred.dtype == torch.int64:
        l64 = _raw(pred, torch.int64, "post_clean")
    else:
        raise ValueError("lm_net_amd.post_clean: pred must be fp32 logits [B,C,H,W] or a uint8 / int64 label map [B,H,W]")
    if labels_out.numel() != B * H * W or (stats is not None and stats.numel() != B * n_classes * 4):
        raise ValueError("lm_net_amd.post_clean: output buffers do not match B=%d, C=%d, %dx%d" % (B, n_classes, H, W))
    _check(load().lmn_post_clean(logits, l8, l64, B, int(n_classes), H, W, C.byref(params), _raw(workspace, torch.uint8, "post_clean"),
                                 _i64(0 if workspace is None else workspace.numel()), _raw(labels_out, torch.uint8, "post_clean"),
                                 _raw(stats, torch.int32, "post_clean"), _stream()), "post_clean")


def post_render(labels_net, src_hw, Hs, Ws, frames, palette, n_classes, alpha256, mode, labels_out, overlay):
    """lmn_post_render: labels_net uint8 [B,H,W] -> labels_out uint8 [B,Hs,Ws] and / or overlay uint8 [B,Hs,Ws,3] over frames uint8
    [B,Hs,Ws,3] or [B,Hs,Ws(,1)].  src_hw: host int32 numpy [B,2] or None; palette: host uint8 numpy [C,3]."""
    B, H, W = labels_net.shape
    channels = 3
    if frames is not None:
        channels = 1 if frames.dim() == 3 else int(frames.shape[3])
        if tuple(frames.shape[:3]) != (B, Hs, Ws) or channels not in (1, 3):
            raise ValueError("lm_net_amd.post_render: frames %s do not match B=%d, %dx%d with 1 or 3 channels"
                             % (tuple(frames.shape), B, Hs, Ws))
    if ((labels_out is not None and labels_out.numel() != B * Hs * Ws) or (overlay is not None and overlay.numel() != B * Hs * Ws * 3)
            or (src_hw is not None and tuple(src_hw.shape) != (B, 2))):
        raise ValueError("lm_net_amd.post_render: buffers do not match B=%d, frame %dx%d" % (B, Hs, Ws))
    hw_arr = None if src_hw is None else np.ascontiguousarray(src_hw, dtype=np.int32)
    hw = None if hw_arr is None else hw_arr.ctypes.data_as(C.POINTER(C.c_int32))
    pal = np.ascontiguousarray(palette, dtype=np.uint8)
    if tuple(pal.shape) != (n_classes, 3):
        raise ValueError("lm_net_amd.post_render: palette %s is not [%d, 3]" % (tuple(pal.shape), n_classes))
    _check(load().lmn_post_render(_raw(labels_net, torch.uint8, "post_render"), B, H, W, hw, int(Hs), int(Ws),
                                  _raw(frames, torch.uint8, "post_render"), channels, pal.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  int(n_classes), int(alpha256), int(mode), _raw(labels_out, torch.uint8, "post_render"),
                                  _raw(overlay, torch.uint8, "post_render"), _stream()), "post_render")


def preprocess_u8(images, masks, flips, out, labels, mean, std):
    """uint8 HWC images [B,Hs,Ws,3] / masks [B,Hs,Ws] -> fp32 NCHW `out` [B,3,H,W] / int64 `labels` [B,H,W]."""
    ref = images if images is not None else masks
    B, Hs, Ws = ref.shape[0], ref.shape[1], ref.shape[2]
    dst = out if out is not None else labels
    H, W = dst.shape[-2], dst.shape[-1]
    m3, s3 = (C.c_double * 3)(*[float(v) for v in mean]), (C.c_double * 3)(*[float(v) for v in std])
    u8, what = torch.uint8, "preprocess_u8"
    _check(load().lmn_preprocess_u8(_raw(images, u8, what), _raw(masks, u8, what), _raw(flips, u8, what), B, Hs, Ws,
                                    H, W, m3, s3, _p(out), _raw(labels, torch.int64, what), _stream()), what)


def preprocess_u8_ex(images, masks, flips, out, labels, mean, std, channels, mask_mode):
    """uint8 images [B,Hs,Ws,channels] (channels 1: also [B,Hs,Ws]) / masks [B,Hs,Ws] -> fp32 NCHW `out` [B,channels,H,W] / int64
    `labels` [B,H,W]; mask_mode 0 thresholds the mask at 127 into {0, 1}, 1 passes class ids through."""
    ref = images if images is not None else masks
    B, Hs, Ws = ref.shape[0], ref.shape[1], ref.shape[2]
    dst = out if out is not None else labels
    H, W = dst.shape[-2], dst.shape[-1]
    if len(mean) != channels or len(std) != channels:
        raise ValueError("lm_net_amd.preprocess_u8_ex: mean and std need %d entries" % channels)
    if ((images is not None and (images.numel() != B * Hs * Ws * channels or out is None or out.numel() != B * channels * H * W))
            or (masks is not None and (masks.numel() != B * Hs * Ws or labels is None or labels.numel() != B * H * W))
            or (flips is not None and flips.numel() != B)):
        raise ValueError("lm_net_amd.preprocess_u8_ex: tensor sizes do not match B=%d, %dx%d -> %dx%d, %d channel(s)"
                         % (B, Hs, Ws, H, W, channels))
    mc, sc = (C.c_double * channels)(*[float(v) for v in mean]), (C.c_double * channels)(*[float(v) for v in std])
    u8, what = torch.uint8, "preprocess_u8_ex"
    _check(load().lmn_preprocess_u8_ex(_raw(images, u8, what), _raw(masks, u8, what), _raw(flips, u8, what), B, Hs, Ws,
                                       H, W, int(channels), int(mask_mode), mc, sc, _p(out), _raw(labels, torch.int64, what), _stream()),
           what)



def augment_u8(images, masks, params, src_hw, params_dev, scratch, gray_sum, out, labels, mean, std, channels, mask_mode):
    """uint8 images [B,Hs,Ws,channels] (channels 1: also [B,Hs,Ws]) / masks [B,Hs,Ws] -> fp32 NCHW `out` [B,channels,H,W] / int64
    `labels` [B,H,W] through lmn_augment_u8.  params: host ctypes array of B AugParam (checked and copied into the device buffer
    params_dev, uint8 [B * sizeof(AugParam)]); src_hw: host int32 numpy array [B,2] or None; scratch: uint8 [B,H,W,channels];
    gray_sum: int64 [B] (the kernels' uint64 sums)."""
    ref = images if images is not None else masks
    if ref is None:
        raise ValueError("lm_net_amd.augment_u8: images or masks required")
    B, Hs, Ws = ref.shape[0], ref.shape[1], ref.shape[2]
    dst = out if out is not None else labels
    if dst is None:
        raise ValueError("lm_net_amd.augment_u8: out or labels required")
    H, W = dst.shape[-2], dst.shape[-1]
    if channels not in (1, 3) or mask_mode not in (0, 1):
        raise ValueError("lm_net_amd.augment_u8: channels %r / mask_mode %r" % (channels, mask_mode))
    if len(mean) != channels or len(std) != channels:
        raise ValueError("lm_net_amd.augment_u8: mean and std need %d entries" % channels)
    if ((images is not None and (images.numel() != B * Hs * Ws * channels or out is None or out.numel() != B * channels * H * W
                                 or scratch is None or scratch.numel() != B * H * W * channels
                                 or gray_sum is None or gray_sum.numel() != B))
            or (masks is not None and (masks.numel() != B * Hs * Ws or labels is None or labels.numel() != B * H * W))
            or len(params) != B or params_dev.numel() != B * C.sizeof(AugParam)
            or (src_hw is not None and tuple(src_hw.shape) != (B, 2))):
        raise ValueError("lm_net_amd.augment_u8: tensor sizes do not match B=%d, %dx%d -> %dx%d, %d channel(s)"
                         % (B, Hs, Ws, H, W, channels))
    hw_arr = None if src_hw is None else np.ascontiguousarray(src_hw, dtype=np.int32)   # (kept alive across the call)
    hw = None if hw_arr is None else hw_arr.ctypes.data_as(C.POINTER(C.c_int32))
    mc, sc = (C.c_double * channels)(*[float(v) for v in mean]), (C.c_double * channels)(*[float(v) for v in std])
    u8, i64, what = torch.uint8, torch.int64, "augment_u8"
    _check(load().lmn_augment_u8(_raw(images, u8, what), _raw(masks, u8, what), params, hw, _raw(params_dev, u8, what), B, Hs,
                                 Ws, H, W, int(channels), int(mask_mode), mc, sc, _raw(scratch, u8, what),
                                 _raw(gray_sum, i64, what), _p(out), _raw(labels, i64, what), _stream()), what)


def oneof_workspace(B, H, W, channels, n_elastic):
    """Bytes of the workspace lmn_augment_oneof_u8 needs (lmn_oneof_workspace)."""
    n = int(load().lmn_oneof_workspace(int(B), int(H), int(W), int(channels), int(n_elastic)))
    if n < 0:
        raise ValueError("lm_net_amd.oneof_workspace: B=%r, %rx%r, %r channel(s), %r elastic" % (B, H, W, channels, n_elastic))
    return n


def augment_oneof_u8(images, masks, params, src_hw, params_dev, scratch, gray_sum, out, labels, mean, std, channels, mask_mode,
                     oneof, oneof_dev, tables, tables_dev, lab_tables, scratch2, labels_tmp, workspace):
    """augment_u8 with the OneOf block between ColorJitter and Normalize (lmn_augment_oneof_u8, include/lmnet_oneof.h).  The first
    thirteen arguments are augment_u8's.  oneof: host ctypes array of B OneOfParam (checked, copied into oneof_dev, uint8 [B *
    sizeof(OneOfParam)]); tables: host float32 numpy array (grid-distortion maps, elastic weights and noise) or None, copied into
    tables_dev (fp32, same length); lab_tables: int32 [LAB_TABLE_INTS] device tensor or None; scratch2: uint8 like scratch;
    labels_tmp: int64 like labels or None; workspace: uint8, at least oneof_workspace(...) bytes."""
    ref = images if images is not None else masks
    dst = out if out is not None else labels
    if ref is None or dst is None:
        raise ValueError("lm_net_amd.augment_oneof_u8: images or masks, and out or labels, required")
    B, Hs, Ws = ref.shape[0], ref.shape[1], ref.shape[2]
    H, W = dst.shape[-2], dst.shape[-1]
    if channels not in (1, 3) or mask_mode not in (0, 1) or len(mean) != channels or len(std) != channels:
        raise ValueError("lm_net_amd.augment_oneof_u8: channels %r / mask_mode %r / mean, std" % (channels, mask_mode))
    nt = 0 if tables is None else int(tables.size)
    if ((images is not None and (images.numel() != B * Hs * Ws * channels or out is None or out.numel() != B * channels * H * W
                                 or scratch is None or scratch.numel() != B * H * W * channels or scratch2 is None
                                 or scratch2.numel() != B * H * W * channels or gray_sum is None or gray_sum.numel() != B))
            or (masks is not None and (masks.numel() != B * Hs * Ws or labels is None or labels.numel() != B * H * W
                                       or (labels_tmp is not None and labels_tmp.numel() != B * H * W)))
            or len(params) != B or params_dev.numel() != B * C.sizeof(AugParam)
            or len(oneof) != B or oneof_dev.numel() != B * C.sizeof(OneOfParam)
            or (nt and (tables.dtype != np.float32 or tables_dev is None or tables_dev.numel() != nt))
            or (lab_tables is not None and lab_tables.numel() != LAB_TABLE_INTS)
            or (src_hw is not None and tuple(src_hw.shape) != (B, 2))):
        raise ValueError("lm_net_amd.augment_oneof_u8: tensor sizes do not match B=%d, %dx%d -> %dx%d, %d channel(s)"
                         % (B, Hs, Ws, H, W, channels))
    hw_arr = None if src_hw is None else np.ascontiguousarray(src_hw, dtype=np.int32)   # (kept alive across the call)
    hw = None if hw_arr is None else hw_arr.ctypes.data_as(C.POINTER(C.c_int32))
    tab_arr = None if not nt else np.ascontiguousarray(tables)                           # (kept alive across the call)
    tab = None if not nt else tab_arr.ctypes.data_as(C.POINTER(C.c_float))
    mc, sc = (C.c_double * channels)(*[float(v) for v in mean]), (C.c_double * channels)(*[float(v) for v in std])
    u8, i64, what = torch.uint8, torch.int64, "augment_oneof_u8"
    _check(load().lmn_augment_oneof_u8(
        _raw(images, u8, what), _raw(masks, u8, what), params, hw, _raw(params_dev, u8, what), B, Hs, Ws, H, W, int(channels),
        int(mask_mode), mc, sc, _raw(scratch, u8, what), _raw(gray_sum, i64, what), _p(out), _raw(labels, i64, what), oneof,
        _raw(oneof_dev, u8, what), tab, C.c_int64(nt), _p(tables_dev) if nt else None, _raw(lab_tables, torch.int32, what),
        _raw(scratch2, u8, what), _raw(labels_tmp, i64, what), _raw(workspace, u8, what), C.c_int64(workspace.numel()), _stream()),
        what)


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2):
    _check(load().lmn_adamw_step(_p(p), _p(g), _p(m), _p(v), _i64(p.numel()), _f(lr), _f(beta1), _f(beta2), _f(eps),
                                 _f(weight_decay), _f(bias_corr1), _f(bias_corr2), _stream()), "adamw_step")


def optim_workspace(n):
    """4-byte words of the workspace of optim_prepare / adamw_step_ex for n floats (lmn_optim_workspace)."""
    return int(load().lmn_optim_workspace(_i64(n)))


def optim_param(betas=(0.9, 0.999), eps=1e-8, max_norm=None, ema_decay=None, flags=0, n_groups=1):
    """An OptimParam (lmn_optim_param_t) from Python values; max_norm None: no clipping, ema_decay None: no EMA.  Clipping and
    OPTIM_SKIP_NONFINITE switch OPTIM_NORM on."""
    p = OptimParam()
    p.beta1, p.beta2, p.eps = float(betas[0]), float(betas[1]), float(eps)
    p.max_norm = 0.0 if max_norm is None else float(max_norm)
    p.ema_decay = -1.0 if ema_decay is None else float(ema_decay)
    p.flags = int(flags) | (OPTIM_NORM if (p.max_norm > 0 or int(flags) & OPTIM_SKIP_NONFINITE) else 0)
    p.n_groups = int(n_groups)
    return p


def _optim_dims(what, g, qgroup, ws):
    n = g.numel()
    if n % 4 or qgroup.numel() != n // 4:
        raise ValueError("lm_net_amd.%s: %d floats need %d group bytes, got %d" % (what, n, n // 4, qgroup.numel()))
    if ws.numel() < optim_workspace_words(n):
        raise ValueError("lm_net_amd.%s: workspace of %d words, %d needed" % (what, ws.numel(), optim_workspace_words(n)))
    return n


def optim_prepare(g, qgroup, param, ws, grad_scale=None, found_inf=None):
    """The control block of one step from the flat gradient g (lmn_optim_prepare): non-finite count, gradient norm, clip coefficient,
    step count and bias corrections, left in ws for adamw_step_ex.  qgroup: uint8 [n / 4]; param: an OptimParam; ws: fp32 workspace
    of at least optim_workspace(n) words whose group table the caller has filled; grad_scale / found_inf: the device scalars of
    torch.amp.GradScaler, or None."""
    n = _optim_dims("optim_prepare", g, qgroup, ws)
    _check(load().lmn_optim_prepare(_p(g), _i64(n), _raw(qgroup, torch.uint8, "optim_prepare"), C.byref(param), _p(ws), _p(grad_scale),
                                    _p(found_inf), _stream()), "optim_prepare")


def adamw_step_ex(p, g, m, v, ema, qgroup, param, ws):
    """One AdamW step over the flat buffers from the control block optim_prepare left in ws (lmn_adamw_step_ex); ema None: no EMA.
    g is read-only: it is not unscaled or clipped in place."""
    n = _optim_dims("adamw_step_ex", g, qgroup, ws)
    if not (p.numel() == m.numel() == v.numel() == n) or (ema is not None and ema.numel() != n):
        raise ValueError("lm_net_amd.adamw_step_ex: the flat buffers differ in size")
    _check(load().lmn_adamw_step_ex(_p(p), _p(g), _p(m), _p(v), _p(ema), _i64(n), _raw(qgroup, torch.uint8, "adamw_step_ex"),
                                    C.byref(param), _p(ws), _stream()), "adamw_step_ex")


def tile_param(batch, channels, height, width, tile, stride, pad="reflect", flips=(), average="logits"):
    """A TileParam (lmn_tile_param_t) from Python values.  tile / stride: (h, w) in pixels; flips: a subset of ("h", "v", "hv") in the
    order of the entries after the identity; channels: of the source for tile_gather, of the tile outputs for tile_blend."""
    for name, value, table in (("pad", pad, TILE_PADS), ("average", average, TILE_AVERAGES)):
        if value not in table:
            raise ValueError("lm_net_amd.tile_param: %s=%r, expected one of %s" % (name, value, sorted(table)))
    flips = tuple(flips)
    if any(f not in TILE_FLIPS for f in flips) or len(set(flips)) != len(flips):
        raise ValueError("lm_net_amd.tile_param: flips=%r, expected distinct members of ('h', 'v', 'hv')" % (flips,))
    p = TileParam()
    p.batch, p.channels, p.height, p.width = int(batch), int(channels), int(height), int(width)
    p.tile_h, p.tile_w, p.stride_h, p.stride_w = int(tile[0]), int(tile[1]), int(stride[0]), int(stride[1])
    p.pad, p.average, p.n_flip = TILE_PADS[pad], TILE_AVERAGES[average], 1 + len(flips)
    for k, f in enumerate(flips):
        p.flip[1 + k] = TILE_FLIPS[f]
    return p


def tile_entries(param):
    """Entries (tiles x mirrored copies) of ONE image of the geometry: n_y * n_x * n_flip."""
    return (tile_axis(param.height, param.tile_h, param.stride_h)[2] * tile_axis(param.width, param.tile_w, param.stride_w)[2]
            * param.n_flip)


def tile_gather(src, param, first, count, tiles):
    """tiles[count, channels, tile_h, tile_w] = the entries first .. first + count - 1 of src [batch, channels, H, W]: padded, cut and
    mirrored, a bit-exact copy (lmn_tile_gather)."""
    if (src.numel() != param.batch * param.channels * param.height * param.width
            or tiles.numel() != int(count) * param.channels * param.tile_h * param.tile_w):
        raise ValueError("lm_net_amd.tile_gather: tensor sizes do not match %d x %d x %dx%d -> %d tiles of %dx%d"
                         % (param.batch, param.channels, param.height, param.width, count, param.tile_h, param.tile_w))
    _check(load().lmn_tile_gather(_raw(src, torch.float32, "tile_gather"), C.byref(param), _i64(first), _i64(count),
                                  _raw(tiles, torch.float32, "tile_gather"), _stream()), "tile_gather")


def tile_blend(z, param, wy, wx, out, labels=None):
    """out[batch, C, H, W] = the windowed, flip-averaged blend of the tile outputs z [batch * entries, C, tile_h, tile_w] in a fixed
    order (lmn_tile_blend); wy / wx: the fp32 window tables; labels: uint8 [batch, H, W] for the arg-max, or None."""
    n = param.batch * tile_entries(param)
    if (z.numel() != n * param.channels * param.tile_h * param.tile_w or wy.numel() != param.tile_h or wx.numel() != param.tile_w
            or out.numel() != param.batch * param.channels * param.height * param.width
            or (labels is not None and labels.numel() != param.batch * param.height * param.width)):
        raise ValueError("lm_net_amd.tile_blend: tensor sizes do not match %d entries of %d x %dx%d -> %d x %d x %dx%d"
                         % (n, param.channels, param.tile_h, param.tile_w, param.batch, param.channels, param.height, param.width))
    f32 = torch.float32
    _check(load().lmn_tile_blend(_raw(z, f32, "tile_blend"), C.byref(param), _raw(wy, f32, "tile_blend"), _raw(wx, f32, "tile_blend"),
                                 _raw(out, f32, "tile_blend"), _raw(labels, torch.uint8, "tile_blend"), _stream()), "tile_blend")


def reparam_fold(hstats, mean, rstd, A, count, batch_stats, w_expand, b_expand, w_shortcut, rows, cred, wpack, kbias, coef, dgamma,
                 dbeta):
    """lmn_reparam_fold: BatchNorm backward of the expand conv folded into the packed operators of ONE three-source conv."""
    E, cinw = w_expand.shape[0], w_expand.shape[1]
    _check(load().lmn_reparam_fold(_p(hstats), _p(mean), _p(rstd), _p(A), _f(count), int(batch_stats), _p(w_expand), _p(b_expand),
                                   _p(w_shortcut), E, rows, cinw, cred, w_shortcut.shape[0], _p(wpack), _p(kbias), _p(coef),
                                   _p(dgamma), _p(dbeta), _MMA[0], _stream()), "reparam_fold")


class SeParamsT(C.Structure):
    _fields_ = [("dvec", C.c_void_p), ("gsum", C.c_void_p), ("hidden", C.c_void_p), ("dw1", C.c_void_p), ("db1", C.c_void_p),
                ("dw2", C.c_void_p), ("db2", C.c_void_p), ("inv_hw", C.c_float), ("B", C.c_int32), ("E", C.c_int32), ("R", C.c_int32)]


def reparam_wfin(R, M, m, coef, hstats, w_expand, b_expand, count, dW, db, se=None):
    """lmn_reparam_wfin: expand-conv weight / bias gradient from the raw gradient R = sum dh x^T and the moments of x.
    se = dict(dvec, gsum, inv_hw, hidden, dw1, db1, dw2, db2): the squeeze-excite parameter gradients of the same block in the same launch."""
    E, cinw = w_expand.shape[0], w_expand.shape[1]
    sp = None
    if se is not None:
        Bn, En = se["gsum"].shape
        sp = SeParamsT(*[_p(se[k]).value for k in ("dvec", "gsum", "hidden", "dw1", "db1", "dw2", "db2")],
                       float(se["inv_hw"]), Bn, En, se["dw1"].shape[0])
    _check(load().lmn_reparam_wfin(_p(R), _p(M), _p(m), _p(coef), _p(hstats), _p(w_expand), _p(b_expand), _f(count), E, R.shape[1],
                                   cinw, _p(dW), _p(db), C.byref(sp) if sp is not None else None, _stream()), "reparam_wfin")


def affine2(u, v, coef, y):
    """y = coef[0] * u + coef[1] * v + coef[2] per channel (activation tensors of shape [..., C])."""
    Cn = u.shape[-1]
    rp = is_rp4(u)
    assert rp == is_rp4(v) == is_rp4(y), "affine2: operands of one layout"
    _check(load().lmn_affine2(_pa(u), _pa(v), _p(coef), _pa(y), _i64(u.numel() // Cn), Cn, u.shape[2] if rp else 0, _dt(u, v, y), _stream()), "affine2")


def fill(t, v):
    _check(load().lmn_fill(_p(t), _f(v), _i64(t.numel()), _stream()), "fill")


def add(a, b, c=None, d=None, out=None):
    out = a if out is None else out
    _check(load().lmn_add(_pa(a), _pa(b), _pa(c), _pa(d), _pa(out), _i64(a.numel()), _dt(a, b, c, d, out), _stream()), "add")
    return out


def colsum(x, out):
    x = _as_view(x)
    rows = x.t.numel() // x.cstride
    _check(load().lmn_colsum(C.c_void_p(x.ptr), _p(out), _i64(rows), x.C, x.cstride, _dt(x), _stream()), "colsum")


def copy_slice(x, y):
    x, y = _as_view(x), _as_view(y)
    rows = x.t.numel() // x.cstride
    _check(load().lmn_copy_slice(C.c_void_p(x.ptr), C.c_void_p(y.ptr), _i64(rows), x.C, x.cstride, y.cstride, _dt(x, y),
                                 _stream()), "copy_slice")


def copy2d(x, y, rows, cols, x_stride, y_stride):
    """y[r][0:cols] = x[r][0:cols] (row strides in floats); any cols."""
    _check(load().lmn_copy2d(_p(x), _p(y), _i64(rows), cols, x_stride, y_stride, _stream()), "copy2d")


# ------------------------------------------------------------------------------------------ streams, plans, kernel timer
def stream_wait(waiter, waited):
    """`waiter` (torch stream) waits for everything enqueued on `waited` so far; recorded when a plan is recording."""
    if waiter.cuda_stream == waited.cuda_stream:
        return
    _check(load().lmn_stream_wait(C.c_void_p(waiter.cuda_stream), C.c_void_p(waited.cuda_stream)), "stream_wait")


def event_record(slot, stream):
    _check(load().lmn_event_record(slot, C.c_void_p(stream.cuda_stream)), "event_record")


def event_wait(slot, stream):
    _check(load().lmn_event_wait(slot, C.c_void_p(stream.cuda_stream)), "event_wait")


_PRIO_STREAMS = {}


def set_priority_stream(stream, level=3):
    """Wave priority 0..3 of the kernels launched on a torch stream (include/lmnet_hip.h, lmn_set_priority_stream).  Process-wide."""
    key = stream.cuda_stream
    if _PRIO_STREAMS.get(key, 0) == level:
        return
    _check(load().lmn_set_priority_stream(C.c_void_p(key), level), "set_priority_stream")
    if len(_PRIO_STREAMS) >= 8:      # (the library's table holds 8 streams and replaces the oldest: forget what this side believes is registered)
        _PRIO_STREAMS.clear()
    _PRIO_STREAMS[key] = level


class Plan:
    """A recorded pass (see include/lmnet_hip.h, lmn_plan_*): every C-ABI entry issued between record_begin() and
    record_end() is remembered with its arguments; run() re-issues them in one FFI crossing."""

    def __init__(self):
        self.h = C.c_void_p(load().lmn_plan_create())
        self.marks = []            # op counts at the segment boundaries reported during recording

    def record_begin(self):
        _check(load().lmn_plan_record_begin(self.h), "plan_record_begin")

    def record_end(self, seal=True):
        return int(load().lmn_plan_record_end(self.h, 1 if seal else 0))

    def size(self):
        return int(load().lmn_plan_size(self.h))

    def mark(self):
        self.marks.append(self.size())

    def run(self, lo=0, hi=-1):
        _check(load().lmn_plan_run(self.h, _i64(lo), _i64(hi)), "plan_run")

    def host_profile(self):
        """Runs the plan once; -> {entry point: (ops, host microseconds)}"""
        lib = load()
        buf = C.create_string_buffer(1 << 16)
        n = int(lib.lmn_plan_host_profile(self.h, buf, _i64(1 << 16)))
        if n < 0:
            raise RuntimeError("plan_host_profile failed: " + last_error())
        return {a: (int(b), float(c)) for a, b, c in (ln.split("\t") for ln in buf.value.decode().splitlines())}

    def __del__(self):
        try:
            if self.h is not None and _lib is not None:
                _lib.lmn_plan_destroy(self.h)
        except Exception:
            pass
        self.h = None


def set_deterministic(on):
    """Fixed-order reductions in every kernel (include/lmnet_hip.h, lmn_set_deterministic): bit-reproducible steps, slower."""
    _check(load().lmn_set_deterministic(1 if on else 0), "set_deterministic")


def get_deterministic():
    return bool(load().lmn_get_deterministic())


def prof_begin(filter_=None):
    """Time (HIP events on the launch stream) every kernel launch whose name contains one of the '|'-separated substrings."""
    _check(load().lmn_prof_begin(filter_.encode() if filter_ else None), "prof_begin")


def prof_end():
    """-> {kernel name: dict(launches, total_us, flops, bytes)} since prof_begin (synchronises the device)."""
    lib = load()
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        need = int(lib.lmn_prof_end(buf, _i64(cap)))
        if need <= cap:
            break
        cap = need + 16
        # the records are kept until the next prof_begin: a second call re-reads them
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, us, fl, by = line.split("\t")
        out[name] = dict(launches=int(n), total_us=float(us), flops=float(fl), bytes=float(by))
    return out


def prof_timeline():
    """After prof_begin("!..."): -> [(kernel, stream, start_us, end_us)] per launch, on the device clock of the first launch."""
    lib = load()
    cap = 1 << 20
    while True:
        buf = C.create_string_buffer(cap)
        need = int(lib.lmn_prof_end(buf, _i64(cap)))
        if need <= cap:
            break
        cap = need + 16
    out = []
    for line in buf.value.decode().splitlines():
        name, st, t0, t1, _ = line.split("\t")
        out.append((name.strip("()"), int(st, 16), float(t0), float(t1)))
    return out
