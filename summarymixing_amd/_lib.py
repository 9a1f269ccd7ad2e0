"""ctypes binding of libsmx.so (include/smx.h).  The product path has NO fallback: if the HIP library is
missing or a call fails, a RuntimeError is raised."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMX_LIB: another build of the same library (e.g. libsmx_diag.so = csrc/build.sh with SMX_DIAG=1, for the ablation tools)
LIB_PATH = os.environ.get("SMX_LIB") or os.path.join(_HERE, "libsmx.so")

c_i, c_i64, c_f, c_vp, c_sz = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
c_d = ctypes.c_double
LR_NOAM, LR_WARM_EXP_DECAY = 0, 1      # include/smx.h SMX_LR_*
SGD_MAX_BLOCKS = 2048                  # include/smx.h SMX_SGD_MAX_BLOCKS (blocks of 256 lanes x 4 elements)

# enums of include/smx.h
F32, BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_SWISH, ACT_LEAKY_RELU, ACT_RELU = 0, 1, 2, 3, 4
C0_NONE, C0_ROW, C0_GROUP, C0_MOD = 0, 1, 2, 3
GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
OUT_T, OUT_F32, OUT_ATOMIC_F32 = 0, 1, 2
EPI_C0_POST = 1
EPI_ACT_GRAD = 2
EPI_LN_BWD = 4
EPI_LN_FWD = 8
IO_RES_F32, IO_LNX_F32, IO_LNFY_F32 = 1, 2, 4
PAD_ZERO, PAD_REFLECT = 0, 1
DW_TILED, DW_WINDOW, DW_ROLL, DW_ROLL_CSGU = 0, 1, 2, 3
SPECAUG_WARP, SPECAUG_TIME, SPECAUG_FREQ = 1, 2, 4
ACTS = {"none": ACT_NONE, "identity": ACT_NONE, "gelu": ACT_GELU, "swish": ACT_SWISH,
        "leaky_relu": ACT_LEAKY_RELU, "relu": ACT_RELU}


class ReduceJob(ctypes.Structure):
    _fields_ = [("src", c_vp), ("dst", c_vp), ("src_stride", c_i64), ("ldd", c_i64), ("nsrc", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("alpha", c_f), ("vec", ctypes.c_int32),
                ("src_ld", ctypes.c_int32)]


class WgradItem(ctypes.Structure):
    _fields_ = [("dZ", c_vp), ("lddz", c_i64), ("X", c_vp), ("ldx", c_i64), ("workspace", c_vp),
                ("M", ctypes.c_int32), ("K", ctypes.c_int32), ("want_bias", ctypes.c_int32), ("pad", ctypes.c_int32)]


class WgradDirectItem(ctypes.Structure):
    """smx_wgrad_direct_item of include/smx.h."""
    _fields_ = [("dZ", c_vp), ("lddz", c_i64), ("X", c_vp), ("ldx", c_i64), ("dW", c_vp), ("lddw", c_i64), ("dbias", c_vp),
                ("M", ctypes.c_int32), ("K", ctypes.c_int32)]


WGRAD_GROUP_MAX = 16


class GemmPlan(ctypes.Structure):
    """smx_gemm_plan of include/smx.h: the instantiation smx_gemm would launch (smx_gemm_plan_query)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kernel", "a_kc", "b_kc", "tile_n", "tile_m", "vec", "lnf", "gather")]


class Epilogue(ctypes.Structure):
    _fields_ = [("bias", c_vp), ("bias_batch_stride", c_i64),
                ("c0", c_vp), ("ldc0", c_i64), ("c0_mode", ctypes.c_int32), ("c0_div", ctypes.c_int32),
                ("act", ctypes.c_int32), ("out_mode", ctypes.c_int32),
                ("z", c_vp), ("ldz", c_i64),
                ("row_mask", c_vp),
                ("res", c_vp), ("ldr", c_i64),
                ("alpha", c_f), ("flags", ctypes.c_int32),
                ("drop_p", c_f), ("drop_cols", ctypes.c_int32), ("drop_seed", ctypes.c_uint64),
                ("colsum", c_vp), ("workspace", c_vp),
                ("ln_x", c_vp), ("ln_ldx", c_i64), ("ln_stats", c_vp), ("ln_gamma", c_vp), ("ln_partial", c_vp),
                ("ln_dx2", c_vp), ("ln_lddx2", c_i64), ("ln_mask2", c_vp), ("ln_alpha2", c_f), ("ln_drop_p2", c_f),
                ("ln_drop_seed2", ctypes.c_uint64),
                ("lnf_gamma", c_vp), ("lnf_beta", c_vp), ("lnf_y", c_vp), ("lnf_ldy", c_i64), ("lnf_stats", c_vp),
                ("lnf_eps", c_f), ("lnf_act", ctypes.c_int32),
                ("io_flags", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("epoch", c_vp),
                ("lnf2_gamma", c_vp), ("lnf2_beta", c_vp), ("lnf2_y", c_vp), ("lnf2_ldy", c_i64), ("lnf2_stats", c_vp),
                ("lnf2_eps", c_f), ("pad2_", ctypes.c_int32)]


class PackJob(ctypes.Structure):
    """smx_pack_job of include/smx.h (one entry of smx_weight_pack_jobs' device table)."""
    _fields_ = [("W", c_vp), ("ldw", c_i64), ("bias", c_vp), ("packed", c_vp), ("M", ctypes.c_int32), ("K", ctypes.c_int32),
                ("transposed", ctypes.c_int32), ("block_start", ctypes.c_int32)]


class LnFwd(ctypes.Structure):
    """smx_ln_fwd of include/smx.h."""
    _fields_ = [("dtype", ctypes.c_int32), ("x_f32", ctypes.c_int32), ("X", c_vp), ("ldx", c_i64), ("gamma", c_vp), ("beta", c_vp),
                ("Y", c_vp), ("ldy", c_i64), ("stats", c_vp), ("eps", c_f), ("act", ctypes.c_int32), ("N", ctypes.c_int32),
                ("D", ctypes.c_int32), ("gamma2", c_vp), ("beta2", c_vp), ("Y2", c_vp), ("ldy2", c_i64), ("stats2", c_vp),
                ("eps2", c_f), ("dtype2", ctypes.c_int32)]


class LnBwd(ctypes.Structure):
    """smx_ln_bwd of include/smx.h."""
    _fields_ = [("dtype", ctypes.c_int32), ("x_f32", ctypes.c_int32), ("dY", c_vp), ("lddy", c_i64), ("slabs", c_vp),
                ("slab_stride", c_i64), ("nslab", ctypes.c_int32), ("act", ctypes.c_int32), ("X", c_vp), ("ldx", c_i64),
                ("gamma", c_vp), ("beta", c_vp), ("stats", c_vp), ("R", c_vp), ("ldr", c_i64), ("dX", c_vp), ("lddx", c_i64),
                ("dgamma", c_vp), ("dbeta", c_vp), ("workspace", c_vp), ("dX2", c_vp), ("lddx2", c_i64), ("row_mask2", c_vp),
                ("alpha2", c_f), ("drop_p2", c_f), ("drop_seed2", ctypes.c_uint64), ("epoch", c_vp), ("Z", c_vp), ("ldz", c_i64),
                ("zact", ctypes.c_int32), ("N", ctypes.c_int32), ("D", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class DwconvArgs(ctypes.Structure):
    """smx_dwconv_args of include/smx.h (Y / ldy carry dY in the backward)."""
    _fields_ = [("dtype", ctypes.c_int32), ("glu", ctypes.c_int32), ("P", c_vp), ("ldp", c_i64), ("w", c_vp), ("bias", c_vp), ("gate", c_vp),
                ("ldg", c_i64), ("Y", c_vp), ("ldy", c_i64), ("dP", c_vp), ("lddp", c_i64), ("dgate", c_vp), ("lddg", c_i64), ("dw", c_vp),
                ("dbias", c_vp), ("workspace", c_vp)] + [(n, ctypes.c_int32) for n in ("B", "T", "D", "k", "pad_mode", "chunk")] + [
                ("drop_p", c_f), ("pad_", ctypes.c_int32), ("drop_seed", ctypes.c_uint64), ("epoch", c_vp)]


class DwconvPlan(ctypes.Structure):
    """smx_dwconv_plan of include/smx.h: the route and geometry smx_dwconv_fwd / _bwd take (smx_dwconv_plan_query)."""
    _fields_ = [(n, ctypes.c_int32 * 3 if n == "grid" else ctypes.c_int32)
                for n in ("route", "chunked", "deferrable", "partial_rows", "grid", "seg", "nseg", "pad_")]


class CtcCollapse(ctypes.Structure):
    """smx_ctc_collapse_args of include/smx.h."""
    _fields_ = [("tok", c_vp), ("lp", c_vp), ("ld", c_i64), ("in_len", c_vp), ("start", c_vp), ("prev", c_vp), ("seen", c_vp),
                ("n_tok", c_vp), ("score", c_vp), ("tokens", c_vp), ("frames", c_vp)] + [
                (n, ctypes.c_int32) for n in ("B", "T", "blank", "cap")]


class AttnOperand(ctypes.Structure):
    """smx_attn_operand of include/smx.h: base pointer + element strides (batch, row, head, D)."""
    _fields_ = [("p", c_vp), ("sb", c_i64), ("sr", c_i64), ("sh", c_i64), ("sd", c_i64)]


class AttnArgs(ctypes.Structure):
    """smx_attn_args of include/smx.h."""
    _fields_ = [("dtype", ctypes.c_int32), ("causal", ctypes.c_int32)] + [
                (n, AttnOperand) for n in ("q", "k", "v", "o", "dO", "dq", "dk", "dv")] + [
                ("lse", c_vp), ("delta", c_vp), ("attn_bias", c_vp), ("ldbias", c_i64), ("key_pad", c_vp), ("ldpad", c_i64),
                ("weights", c_vp), ("w_sb", c_i64), ("ldw", c_i64)] + [(n, ctypes.c_int32) for n in ("B", "L", "S", "H", "D")] + [
                ("scale", c_f), ("drop_p", c_f), ("pad_", ctypes.c_int32), ("drop_seed", ctypes.c_uint64), ("epoch", c_vp)]


class AttnPlan(ctypes.Structure):
    """smx_attn_plan of include/smx.h (smx_attn_plan_query)."""
    _fields_ = [(n, ctypes.c_int32 * 3 if n == "grid" else ctypes.c_int32)
                for n in ("rows", "key_tile", "d_chunk", "lds_bytes", "threads", "launches", "grid", "pad_")]


ATTN_FWD, ATTN_BWD_DQ, ATTN_BWD_DKV, ATTN_WEIGHTS = 0, 1, 2, 3      # `pass` of smx_attn_plan_query


class AttnStepArgs(ctypes.Structure):
    """smx_attn_step_args of include/smx.h."""
    _fields_ = [("dtype", ctypes.c_int32), ("pad_", ctypes.c_int32)] + [
                (n, AttnOperand) for n in ("q", "k_new", "v_new", "K", "V", "o")] + [
                ("n_keys", c_vp), ("workspace", c_vp)] + [(n, ctypes.c_int32) for n in ("B", "H", "D", "cap")] + [
                ("scale", c_f), ("pad2_", ctypes.c_int32)]


class AttnStepPlan(ctypes.Structure):
    """smx_attn_step_plan of include/smx.h (smx_attn_step_plan_query)."""
    _fields_ = [(n, ctypes.c_int32 * 3 if n == "grid" else ctypes.c_int32)
                for n in ("lanes_per_key", "keys_per_wave", "waves", "threads", "splits", "chunk", "launches", "lds_bytes", "grid",
                          "pad_")] + [("workspace_bytes", c_i64)]


class S2SSelectArgs(ctypes.Structure):
    """smx_s2s_select_args of include/smx.h."""
    _fields_ = [("logits", c_vp), ("ldz", c_i64), ("forced", c_vp), ("tok", c_vp), ("done", c_vp), ("n_tok", c_vp), ("score", c_vp),
                ("tokens", c_vp), ("logp_tok", c_vp), ("inv_temp", ctypes.c_double)] + [
                (n, ctypes.c_int32) for n in ("dtype", "B", "V", "cap", "eos", "min_steps")]


class AttnStepRowsArgs(ctypes.Structure):
    """smx_attn_step_rows_args of include/smx.h."""
    _fields_ = [("s", AttnStepArgs), ("anc", c_vp), ("ld_anc", c_i64), ("kv_div", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class S2SBeamArgs(ctypes.Structure):
    """smx_s2s_beam_args of include/smx.h."""
    _fields_ = [("logits", c_vp), ("ldz", c_i64), ("extra", c_vp), ("ldx", c_i64)] + [
                (n, c_vp) for n in ("tok", "score", "done_row", "done", "n_tok", "tokens", "logp_tok", "anc", "s_tokens", "s_logp", "s_anc",
                                    "cand_val", "cand_lp", "cand_idx", "cand_n", "pool_tokens", "pool_logp", "pool_len", "pool_final",
                                    "pool_sum", "pool_seq", "pool_cnt", "pool_ins", "res_tokens", "res_logp", "res_len", "res_final",
                                    "res_sum")] + [("inv_temp", ctypes.c_double)] + [
                (n, ctypes.c_int32) for n in ("dtype", "B", "W", "V", "cap", "eos", "min_steps", "length_norm")]


class CtcPrefixArgs(ctypes.Structure):
    """smx_ctc_prefix_args of include/smx.h."""
    _fields_ = [("x", c_vp), ("ldx", c_i64), ("enc_len", c_vp), ("score", c_vp), ("done", c_vp), ("n_tok", c_vp), ("tokens", c_vp),
                ("anc", c_vp), ("state", c_vp), ("psi", c_vp), ("logits", c_vp), ("ldz", c_i64), ("extra", c_vp), ("lde", c_i64),
                ("inv_temp", ctypes.c_double), ("weight", ctypes.c_float)] + [
                (n, ctypes.c_int32) for n in ("dtype", "B", "W", "V", "T", "cap", "blank", "eos", "pad_")]


class LmScoreArgs(ctypes.Structure):
    """smx_lm_score_args of include/smx.h."""
    _fields_ = [("logits", c_vp), ("ldz", c_i64), ("extra", c_vp), ("lde", c_i64), ("score", c_vp), ("done", c_vp), ("n_tok", c_vp),
                ("inv_temp", ctypes.c_double), ("weight", ctypes.c_float)] + [
                (n, ctypes.c_int32) for n in ("dtype", "B", "W", "V", "cap", "accumulate", "pad_")]


class TbeamArgs(ctypes.Structure):
    """smx_tbeam_args of include/smx.h."""
    _fields_ = [("enc", c_vp), ("ld_b", c_i64), ("ld_t", c_i64), ("lengths", c_vp), ("WihT", c_vp), ("ldw", c_i64)] + [
                (n, c_vp) for n in ("bias", "Whh", "Wproj", "Wlin", "blin", "cur_tok", "h_in", "c_in", "h_out", "c_out", "pdec", "z",
                                    "lm_logits")] + [("ld_lm", c_i64)] + [
                (n, c_vp) for n in ("lm_h_in", "lm_c_in", "lm_h_out", "lm_c_out", "state", "done", "overflow", "expansions", "frames",
                                    "tokens", "out_len", "scores", "sums", "n_hyps")] + [
                (n, ctypes.c_float) for n in ("lm_weight", "state_beam", "expand_beam")] + [
                (n, ctypes.c_int32) for n in ("dtype", "B", "T", "H", "J", "V", "W", "nbest", "E", "U", "act", "blank", "lm_L", "lm_H",
                                              "pad_")]


# name -> (restype, argtypes); mirrors include/smx.h one to one (tests/test_abi.py checks the export list)
SIGNATURES = {
    "smx_version": (c_i, []),
    "smx_last_error": (ctypes.c_char_p, []),
    "smx_gemm": (c_i, [c_i, c_i, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_i, c_i, c_i, c_i, c_i,
                       ctypes.POINTER(Epilogue), c_vp]),
    "smx_gemm_plan_query": (c_i, [c_i, c_i, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_i, c_i, c_i, c_i, c_i,
                                  ctypes.POINTER(Epilogue), ctypes.POINTER(GemmPlan)]),
    "smx_gemm_colsum_workspace": (c_sz, [c_i, c_i]),
    "smx_gemm_panel_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "smx_weight_pack_bytes": (c_sz, [c_i, c_i]),
    "smx_weight_pack": (c_i, [c_i, c_vp, c_i64, c_i, c_vp, c_i, c_i, c_vp, c_vp]),
    "smx_weight_pack_job_blocks": (c_i, [c_i, c_i]),
    "smx_weight_pack_jobs": (c_i, [c_i, c_vp, c_i, c_i, c_vp]),
    "smx_gemm_panel": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_i64, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_vp]),
    "smx_gemm_ln_fused_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "smx_gemm_ln_pair_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "smx_linear_wgrad_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "smx_linear_wgrad": (c_i, [c_i, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i, c_i, c_i, c_i,
                               c_f, c_vp, c_vp]),
    "smx_linear_wgrad_partial": (c_i, [c_i, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_i, c_i, c_i, c_i, c_i, c_vp,
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_vp]),
    "smx_wgrad_group_splits": (c_i, [c_i, ctypes.POINTER(WgradItem), c_i]),
    "smx_wgrad_group_workspace": (c_sz, [c_i, c_i, c_i]),
    "smx_wgrad_group": (c_i, [c_i, c_i, ctypes.POINTER(WgradItem), c_i, c_i, c_vp]),
    "smx_reduce_job_blocks": (c_i, [ctypes.POINTER(ReduceJob)]),
    "smx_reduce_jobs": (c_i, [c_vp, c_vp, c_i, c_i, c_vp]),
    "smx_layernorm_bwd_blocks": (c_i, [c_i]),
    "smx_linear_act_mask_fwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i,
                                      ctypes.POINTER(Epilogue), c_vp]),
    "smx_act_mask_bwd_workspace": (c_sz, [c_i, c_i]),
    "smx_act_mask_bwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_i, c_i, c_i, c_f, c_vp, c_vp,
                               c_i64, c_i, c_f, ctypes.c_uint64, c_vp, c_vp, c_vp]),
    "smx_masked_mean_workspace": (c_sz, [c_i, c_i, c_i]),
    "smx_masked_mean_fwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp, c_vp]),
    "smx_masked_mean_bwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_i64, c_i, c_i, c_i, c_f, ctypes.c_uint64, c_vp, c_vp]),
    "smx_pool_bcast_ok": (c_i, [c_i, c_i, c_i]),
    "smx_pool_bcast": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i, c_i, c_i, c_i, c_f, ctypes.c_uint64, c_vp, c_vp, c_i64,
                             c_vp, c_i, c_vp]),
    "smx_masked_mean_bwd_act": (c_i, [c_i, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_chunk_mean_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "smx_chunk_mean_fwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp]),
    "smx_chunk_mean_bwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp]),
    "smx_expdecay_mean_workspace": (c_sz, [c_i, c_i, c_i]),
    "smx_expdecay_mean_fwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_f, c_vp, c_vp]),
    "smx_expdecay_mean_bwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_f, c_vp, c_vp]),
    "smx_layernorm_fwd": (c_i, [ctypes.POINTER(LnFwd), c_vp]),
    "smx_layernorm_bwd_workspace": (c_sz, [c_i, c_i]),
    "smx_layernorm_bwd": (c_i, [ctypes.POINTER(LnBwd), c_vp]),
    "smx_dwconv_fwd": (c_i, [ctypes.POINTER(DwconvArgs), c_vp]),
    "smx_dwconv_bwd": (c_i, [ctypes.POINTER(DwconvArgs), c_vp]),
    "smx_dwconv_plan_query": (c_i, [ctypes.POINTER(DwconvArgs), c_i, ctypes.POINTER(DwconvPlan)]),
    "smx_dwconv1d_glu_bwd_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "smx_dft_frames": (c_i, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_frame_window": (c_i, [c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_fbank_workspace": (c_sz, [c_i, c_i, c_i]),
    "smx_mel_db": (c_i, [c_i, c_vp, c_i64, c_i, c_vp, c_i, c_i, c_f, c_f, c_vp, c_i, c_i, c_vp, c_vp]),
    "smx_im2col_s2": (c_i, [c_i, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_col2im_s2": (c_i, [c_i, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_conv1_ln_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "smx_conv1_ln_fwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_f, c_i, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_conv1_ln_bwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_linear_k16_fwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_i64, c_i, c_vp]),
    "smx_conv2d_s2_fwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_conv2d_s2_wgrad_workspace": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "smx_conv2d_s2_wgrad": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp]),
    "smx_conv2d_s2_dgrad": (c_i, [c_i, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_axpby": (c_i, [c_i, c_f, c_vp, c_i64, c_f, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_vp]),
    "smx_dropout": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_f, ctypes.c_uint64, c_vp, c_vp]),
    "smx_add_rowtable": (c_i, [c_i, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_vp]),
    "smx_cast_from_f32": (c_i, [c_i, c_vp, c_vp, c_i64, c_vp]),
    "smx_cast_to_f32": (c_i, [c_i, c_vp, c_vp, c_i64, c_vp]),
    "smx_adamw_step": (c_i, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_f, c_f, c_f, c_f, c_f, c_i, c_f, c_vp, c_vp, c_vp]),
    "smx_adamw_step_lr": (c_i, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_f, c_vp, c_f, c_f, c_f, c_f, c_i, c_f, c_vp, c_vp, c_vp]),
    "smx_sgd_step": (c_i, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f, c_vp, c_f, c_f, c_i, c_f, c_vp, c_vp]),
    "smx_lr_schedule": (c_i, [c_i, c_d, c_d, c_d, c_d, c_d, c_i64, c_vp, c_vp, c_vp]),
    "smx_utt_meanstd": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_f, c_vp]),
    "smx_stats_combine": (c_i, [c_vp, c_vp, c_i, c_i, c_vp, c_vp, c_f, c_vp]),
    "smx_colnorm": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_vp]),
    "smx_log_softmax_fwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_vp]),
    "smx_log_softmax_bwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_vp]),
    "smx_ctc_workspace": (c_sz, [c_i, c_i, c_i]),
    "smx_ctc_loss_fwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp]),
    "smx_ctc_loss_bwd": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_i64, c_vp,
                               c_vp]),
    "smx_transducer_joint_fwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_transducer_joint_bwd_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "smx_transducer_joint_bwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp]),
    "smx_transducer_row_stats": (c_i, [c_i, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp]),
    "smx_transducer_loss_fwd": (c_i, [c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_vp, c_vp]),
    "smx_transducer_loss_bwd": (c_i, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_vp, c_vp]),
    "smx_transducer_logit_grad": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp, c_i64, c_vp]),
    "smx_transducer_fused_ok": (c_i, [c_i, c_i, c_i]),
    "smx_transducer_stats_workspace": (c_sz, [c_i, c_i]),
    "smx_transducer_gemm_stats": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "smx_transducer_gemm_grad": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_vp,
                                       c_i64, c_vp]),
    "smx_lstm_ok": (c_i, [c_i, c_i]),
    "smx_lstm_fwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp]),
    "smx_lstm_bwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp]),
    "smx_onehot_rows": (c_i, [c_i, c_vp, c_vp, c_i64, c_i, c_i, c_i, c_vp]),
    "smx_onehot_gates_fwd": (c_i, [c_i, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_onehot_gates_wgrad": (c_i, [c_i, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_i, c_vp]),
    "smx_lstm_step_ok": (c_i, [c_i, c_i, c_i]),
    "smx_lstm_step": (c_i, [c_i, c_vp, c_i64, c_vp, c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp]),
    "smx_gather_rows": (c_i, [c_i, c_vp, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_vp]),
    "smx_greedy_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "smx_greedy_workspace": (c_sz, [c_i, c_i]),
    "smx_greedy_start": (c_i, [c_i, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_vp]),
    "smx_greedy_decode": (c_i, [c_i, c_vp, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                c_vp, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_vp, c_vp]),
    "smx_get_config": (c_i, [c_vp]),
    "smx_gemm_ln_tile_rows": (c_i, []),
    "smx_gemm_ln_tile_rows_for": (c_i, [c_i, c_i]),
    "smx_gemm_panel_slabs_ok": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "smx_gemm_panel_slabs": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_slab_epilogue_ok": (c_i, [c_i, c_i, c_i, c_i]),
    "smx_slab_epilogue": (c_i, [c_i, c_vp, c_i, c_i64, c_vp, c_i64, c_i, c_i, ctypes.POINTER(Epilogue), c_vp]),
    "smx_chunk_mean_sharded": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_vp, c_i, c_i, c_vp, c_vp]),
    "smx_expdecay_mean_sharded": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_i, c_vp, c_vp, c_vp]),
    "smx_wgrad_group_direct_ok": (c_i, [c_i, c_i, c_i]),
    "smx_wgrad_group_direct": (c_i, [c_i, c_i, ctypes.POINTER(WgradDirectItem), c_i, c_vp]),
    "smx_gemm_panel_rows": (c_i, [c_i, c_i]),
    "smx_step_counter_add": (c_i, [c_vp, ctypes.c_uint64, c_vp]),
    "smx_stream_capture_id": (c_i, [c_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "smx_sumsq_workspace": (c_sz, []),
    "smx_sumsq": (c_i, [c_vp, c_i64, c_vp, c_vp, c_vp]),
    "smx_clip_factor": (c_i, [c_vp, c_f, c_f, c_vp, c_vp]),
    "smx_stream_summary": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_dwconv1d_glu_stream": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_i, c_i, c_i, c_i, c_vp]),
    "smx_stream_advance": (c_i, [c_i, c_vp, c_vp, c_i64, c_i, c_vp, c_i64, c_i, c_i, c_vp]),
    "smx_slot_summary": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_dwconv1d_glu_slots": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_slot_begin": (c_i, [c_i, c_vp, c_vp, c_vp, c_i64, c_i, c_vp, c_i64, c_i, c_i, c_i, c_vp]),
    "smx_slot_advance": (c_i, [c_vp, c_vp, c_i, c_i, c_vp]),
    "smx_specaug_params_bytes": (c_sz, [c_i, c_i, c_i]),
    "smx_specaug_draw": (c_i, [c_vp, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_uint64, c_vp, c_vp]),
    "smx_specaug_apply": (c_i, [c_i, c_vp, c_i64, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_resample_plan": (c_i, [c_i, c_i, c_vp, c_vp, c_vp, c_sz]),
    "smx_resample": (c_i, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i, c_i64, c_vp]),
    "smx_seqloss_fwd": (c_i, [c_i, c_i, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_vp, c_vp, c_vp,
                              c_vp, c_vp, c_vp, c_vp]),
    "smx_seqloss_bwd": (c_i, [c_i, c_i, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_i, c_f, c_f, c_vp, c_vp, c_vp, c_i64,
                              c_vp]),
    "smx_ctc_best_path": (c_i, [c_i, c_vp, c_i64, c_i, c_i, c_vp, c_vp, c_vp]),
    "smx_ctc_head_ok": (c_i, [c_i, c_i, c_i]),
    "smx_ctc_head_workspace": (c_sz, [c_i, c_i]),
    "smx_ctc_head_best_path": (c_i, [c_i, c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_vp, c_vp, c_vp, c_vp]),
    "smx_ctc_collapse": (c_i, [ctypes.POINTER(CtcCollapse), c_vp]),
    "smx_attn_fwd": (c_i, [ctypes.POINTER(AttnArgs), c_vp]),
    "smx_attn_bwd": (c_i, [ctypes.POINTER(AttnArgs), c_vp]),
    "smx_attn_weights": (c_i, [ctypes.POINTER(AttnArgs), c_vp]),
    "smx_attn_plan_query": (c_i, [ctypes.POINTER(AttnArgs), c_i, ctypes.POINTER(AttnPlan)]),
    "smx_tgt_embed_fwd": (c_i, [c_i, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i, c_i, c_i, c_i, c_i, c_vp]),
    "smx_tgt_embed_bwd": (c_i, [c_i, c_vp, c_vp, c_i64, c_vp, c_i64, c_i, c_i, c_i, c_i, c_vp]),
    "smx_attn_step": (c_i, [ctypes.POINTER(AttnStepArgs), c_vp]),
    "smx_attn_step_plan_query": (c_i, [ctypes.POINTER(AttnStepArgs), ctypes.POINTER(AttnStepPlan)]),
    "smx_s2s_embed_step": (c_i, [c_i, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i, c_i, c_i, c_i, c_vp]),
    "smx_s2s_select": (c_i, [ctypes.POINTER(S2SSelectArgs), c_vp]),
    "smx_attn_step_rows": (c_i, [ctypes.POINTER(AttnStepRowsArgs), c_vp]),
    "smx_attn_step_rows_plan_query": (c_i, [ctypes.POINTER(AttnStepRowsArgs), ctypes.POINTER(AttnStepPlan)]),
    "smx_s2s_beam_select": (c_i, [ctypes.POINTER(S2SBeamArgs), c_vp]),
    "smx_ctc_prefix_init": (c_i, [ctypes.POINTER(CtcPrefixArgs), c_vp]),
    "smx_ctc_prefix_score": (c_i, [ctypes.POINTER(CtcPrefixArgs), c_vp]),
    "smx_ctc_prefix_advance": (c_i, [ctypes.POINTER(CtcPrefixArgs), c_vp]),
    "smx_lm_score": (c_i, [ctypes.POINTER(LmScoreArgs), c_vp]),
    "smx_tbeam_ok": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "smx_tbeam_state_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i]),
    "smx_tbeam_init": (c_i, [ctypes.POINTER(TbeamArgs), c_vp]),
    "smx_tbeam_step": (c_i, [ctypes.POINTER(TbeamArgs), c_vp]),
    "smx_tbeam_select": (c_i, [ctypes.POINTER(TbeamArgs), c_vp]),
    "smx_tbeam_resume": (c_i, [ctypes.POINTER(TbeamArgs), c_vp, c_vp, c_vp]),
    "smx_tbeam_select_stream": (c_i, [ctypes.POINTER(TbeamArgs), c_vp, c_vp]),
}

_lib = None


def lib():
    """Load libsmx.so (once).  Fails loudly: there is no CPU / eager fallback for the product path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or bash summarymixing_amd/csrc/build.sh). summarymixing_amd has no fallback path.")
        # torch first: libsmx.so needs libamdhip64.so, and the process must end up with ONE HIP runtime - the one torch
        # ships and initialises.  Loaded the other way round (libsmx pulling /opt/rocm's copy in before `import torch`), the
        # library's launches fail with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


class Config(ctypes.Structure):
    """smx_config of include/smx.h: the knobs the library read from the environment once."""
    _fields_ = [("ln_tile_rows", ctypes.c_int32),
                ("gemm_ablate", ctypes.c_int32), ("wgroup_ablate", ctypes.c_int32), ("dwroll_ablate", ctypes.c_int32),
                ("diag_build", ctypes.c_int32), ("t256", ctypes.c_int32), ("panel_rows", ctypes.c_int32), ("pool_fuse_max_rows", ctypes.c_int32), ("ln_tile64", ctypes.c_int32), ("lnb_lds", ctypes.c_int32)]


def get_config():
    """The knobs in force as a dict (smx_get_config)."""
    c = Config()
    check(lib().smx_get_config(ctypes.byref(c)), "smx_get_config")
    return {name: getattr(c, name) for name, _ in Config._fields_}


def check(code, what):
    if code != 0:
        msg = lib().smx_last_error()
        raise RuntimeError(f"{what} failed with code {code}: {msg.decode() if msg else ''}")
