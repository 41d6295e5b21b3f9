"""Which kernel INSTANCE ran: a recorder over the in-library kernel timer, and the table that gives every instance the training step
launches an owner.

Every launch of liblmnet_hip.so goes through LMN_LAUNCH; between hip.prof_begin(None) and hip.prof_end() the timer files it under its
instantiated name (`conv_dma3_kernel<3, 1, 4>`, `dw_bwd_kernel<float, 0, true, true, 2>`).  Host predicates pick the instance from
channel counts, map size, strides, storage type, deterministic mode and the lmn_conv_dma_config switches, so a check at a small shape
can run another instance than the one its comment names, and pass.  Three uses:

  * ``launched(fn)`` runs ``fn`` under the timer and returns its result and the set of names launched;
  * ``OWNED`` maps the exact name of an instance to its owner: a ``kernel_checks.check_*`` function or a pytest node id
    (``tests/<file>.py::<test>``) that compares THAT instance with a high-precision reference of the operation -- not with another
    kernel.  ``owner_check`` (the decorator of every check_*) and the named tests assert that the owner really launches what it owns;
    tests/test_kernel_census_gpu.py asserts that every instance a training step launches has an owner, and
    tests/test_kernel_census_envelope_gpu.py the same for the wide variants, other windows, class counts and precisions;
  * ``form_row`` turns a claim about dispatch ("the M-split kernel", "two-stage reduction") into a (name, err, tol) row.

A new kernel instance that reaches the step needs an entry here and a case in its owner that selects it (README, tests section).
"""
import functools

from lm_net_amd import hip

_OPEN = []   # name sets of the recordings in progress, innermost last


def launched(fn):
    """fn() between hip.prof_begin(None) and hip.prof_end() -> (fn's result, {instance names launched}).

    The timer holds ONE recording and prof_begin discards it, so never nest raw prof_begin / prof_end pairs.  A launched() inside a
    launched() (a form assertion inside an owner check) is served by splitting: the enclosing recording is closed, its names kept, and
    it is resumed afterwards with the inner names added.  Every prof_end synchronises the device: wrap calls, not inner loops."""
    if _OPEN:
        _OPEN[-1] |= set(hip.prof_end())
    _OPEN.append(set())
    hip.prof_begin(None)
    try:
        out = fn()
    finally:
        names = _OPEN.pop() | set(hip.prof_end())
        if _OPEN:
            _OPEN[-1] |= names
            hip.prof_begin(None)
    return out, names


def owned_by(owner):
    return {k for k, v in OWNED.items() if v == owner}


def owner_check(fn):
    """Decorator of a kernel_checks.check_*: the body runs under launched() and the rows gain
    ("<check>: owned instances not launched: [...]", number missing, 0.0).  A check called from inside another one (check_conv_bf16
    re-runs the fp32 checks with bf16 operands, which selects other instances) runs bare: the outer check's row speaks for it."""
    @functools.wraps(fn)
    def run(*a, **k):
        if _OPEN:
            return fn(*a, **k)
        rows, names = launched(lambda: fn(*a, **k))
        missing = sorted(owned_by(fn.__name__) - names)
        rows.append(("%s: owned instances not launched: %s" % (fn.__name__, missing), float(len(missing)), 0.0))
        return rows
    return run


def form_row(label, names, want=(), never=()):
    """One row for a claim about dispatch: every entry of `want` and no entry of `never` is the start of a launched name (a base
    name with '<' selects the kernel, a longer prefix its leading template arguments, a full name one instance)."""
    hit = lambda p: any(n.startswith(p) for n in names)
    bad = ["missing " + p for p in want if not hit(p)] + ["unexpected " + p for p in never if hit(p)]
    return ("form: " + label + (" -- %s; launched %s" % (", ".join(bad), sorted(names)) if bad else ""), float(len(bad)), 0.5)


OWNED = {
    "avgpool_bwd_kernel<__bf16>": "check_bf16_storage_rows",
    "avgpool_fwd_wave_kernel<__bf16>": "check_bf16_storage_rows",
    "bnact_fwd_fin_kernel<__bf16>": "check_bf16_storage_rows",
    "chan_kernel<0, __bf16>": "check_bf16_storage_rows",
    "chan_kernel<1, __bf16>": "check_bf16_storage_rows",
    "dw_bwd_kernel<__bf16, 0, false, true, 2>": "check_bf16_storage_rows",
    "dw_bwd_kernel<__bf16, 0, true, true, 2>": "check_bf16_storage_rows",
    "dw_fwd_kernel<__bf16, true>": "check_bf16_storage_rows",
    "dw_stats0_kernel<__bf16, true>": "check_bf16_storage_rows",
    "dw_stats1_kernel<__bf16, true>": "check_bf16_storage_rows",
    "gattn_bwd_kv_mfma_kernel<__bf16>": "check_bf16_storage_rows",
    "gattn_bwd_q_mfma_kernel<__bf16>": "check_bf16_storage_rows",
    "gattn_fwd_mfma_kernel<__bf16>": "check_bf16_storage_rows",
    "ln_bwd_kernel<32, __bf16>": "check_bf16_storage_rows",
    "ln_bwd_kernel<64, __bf16>": "check_bf16_storage_rows",
    "na_bwd_fused_kernel<1, 3, __bf16>": "check_bf16_storage_rows",
    "na_bwd_fused_kernel<2, 6, __bf16>": "check_bf16_storage_rows",
    "na_bwd_kv_kernel<4, __bf16>": "check_bf16_storage_rows",
    "na_bwd_kv_kernel<8, __bf16>": "check_bf16_storage_rows",
    "na_bwd_q_kernel<4, __bf16>": "check_bf16_storage_rows",
    "na_bwd_q_kernel<8, __bf16>": "check_bf16_storage_rows",
    "na_fwd_kernel<1, __bf16>": "check_bf16_storage_rows",
    "na_fwd_kernel<2, __bf16>": "check_bf16_storage_rows",
    "na_fwd_kernel<4, __bf16>": "check_bf16_storage_rows",
    "na_fwd_kernel<8, __bf16>": "check_bf16_storage_rows",
    "nchw_to_nhwc_kernel<__bf16>": "check_bf16_storage_rows",
    "nhwc_to_nchw_kernel<__bf16>": "check_bf16_storage_rows",
    "up2_bwd_kernel<__bf16>": "check_bf16_storage_rows",
    "bn_fold_kernel": "check_bn_tail",
    "bnact_fwd_fin_kernel<float>": "check_bn_tail",
    "bnact_fwd_kernel<float>": "check_bn_tail",
    "chan_kernel<0, float>": "check_bn_tail",
    "chan_kernel<1, float>": "check_bn_tail",
    "conv_tileM_kernel<9, 1, 0, 2, false, false>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 0, 0, false, true>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 0, 2, false, false>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 0, 2, false, true>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 2, 2, false, false>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, false, 2, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, false, 2, true, false, true, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, true, 2, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 2, false, 2, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, false, 2, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, false, 2, false, false, true, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, false, 2, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, true, 2, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 2, false, 2, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, false, 2, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, false, 2, false, false, true, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, true, 2, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 2, false, 0, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 2, false, 2, false, false, false, 2>": "check_conv3_storage",
    "wgrad3_kernel<1, 1, 0, false>": "check_conv3_storage",
    "wgrad3_kernel<1, 1, 2, false>": "check_conv3_storage",
    "wgrad3_kernel<1, 1, 2, true>": "check_conv3_storage",
    "wgrad3_kernel<2, 2, 2, false>": "check_conv3_storage",
    "wgrad3_kernel<2, 2, 2, true>": "check_conv3_storage",
    "wgrad_lds_kernel<9, 1, 1, 2>": "check_conv3_storage",
    "wgrad_lds_kernel<9, 2, 2, 2>": "check_conv3_storage",
    "conv_tileM_kernel<1, 1, 1, 0, false, false>": "check_conv_bn_epilogues",
    "conv_tileM_kernel<1, 1, 1, 2, false, false>": "check_conv_bn_epilogues",
    "conv_tileM_kernel<1, 2, 1, 0, false, false>": "check_conv_bn_epilogues",
    "conv_tileM_kernel<1, 2, 1, 2, false, false>": "check_conv_bn_epilogues",
    "conv_tile_kernel<1, 2, 1, false, 0, false, false, false, 2>": "check_conv_bn_epilogues",
    "conv_tile_kernel<1, 2, 1, false, 2, false, false, false, 2>": "check_conv_bn_epilogues",
    "conv_tile_kernel<1, 3, 1, false, 0, false, false, false, 2>": "check_conv_bn_epilogues",
    "conv_tile_kernel<1, 3, 1, false, 2, false, false, false, 2>": "check_conv_bn_epilogues",
    "conv_tile_kernel<9, 1, 0, true, 0, false, false, false, 2>": "check_conv_bwd_data",
    "conv_tile_kernel<9, 2, 0, true, 0, false, false, false, 2>": "check_conv_bwd_data",
    "conv_tile_kernel<9, 3, 0, true, 0, false, false, false, 2>": "check_conv_bwd_data",
    "conv_dma1_kernel<1, 0, 0, 0, 2, 2, false, 2, 4, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<12, 6, 0, 0, 2, 0, true, 1, 2, 3, 2>": "check_conv_dma1",
    "conv_dma1_kernel<12, 6, 0, 0, 2, 0, true, 1, 3, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<3, 0, 0, 0, 2, 2, false, 2, 4, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<3, 0, 0, 6, 2, 5, false, 2, 3, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<6, 0, 0, 0, 3, 2, false, 2, 3, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<6, 0, 0, 12, 3, 5, false, 1, 3, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<6, 3, 0, 0, 1, 0, true, 2, 3, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<6, 3, 0, 0, 1, 0, true, 2, 3, 2, 2>": "check_conv_dma1",
    "conv_dma1_kernel<6, 3, 3, 0, 1, 0, false, 2, 2, 0, 0>": "check_conv_dma1",
    "conv_dma1_kernel<6, 3, 3, 6, 1, 0, false, 1, 3, 2, 5>": "check_conv_dma1",
    "conv_tile_kernel<1, 1, 0, false, 4, false, false, false, 2>": "check_conv_dma1",
    "conv_tile_kernel<1, 2, 0, false, 4, false, false, false, 2>": "check_conv_dma1",
    "conv_tile_kernel<1, 2, 2, false, 4, false, false, false, 2>": "check_conv_dma1",
    "conv_tile_kernel<1, 2, 5, false, 4, false, false, false, 2>": "check_conv_dma1",
    "conv_tile_kernel<1, 3, 2, false, 4, false, false, false, 2>": "check_conv_dma1",
    "conv_tile_kernel<1, 3, 5, false, 4, false, false, false, 2>": "check_conv_dma1",
    "conv_dma3_kernel<3, 1, 4>": "check_conv_dma3",
    "conv_dma3_kernel<3, 2, 4>": "check_conv_dma3",
    "conv_dma3_kernel<6, 1, 2>": "check_conv_dma3",
    "conv_dma3_kernel<6, 2, 2>": "check_conv_dma3",
    "conv_tile_kernel<9, 1, 2, false, 0, false, false, false, 2>": "check_conv_dma3",
    "conv_tile_kernel<9, 2, 2, false, 0, false, false, false, 2>": "check_conv_dma3",
    "det_sum_kernel": "check_conv_dma3",
    "conv_dmaM_kernel<0, 4>": "check_conv_dmaM",
    "conv_dmaM_kernel<2, 3>": "check_conv_dmaM",
    "conv_tileM_kernel<9, 2, 0, 0, false, false>": "check_conv_dmaM",
    "conv_dmaM_kernel<0, 3>": "check_conv_fwd",
    "conv_pack_batch_kernel": "check_conv_fwd",
    "conv_pack_kernel": "check_conv_fwd",
    "conv_tileM_kernel<1, 1, 0, 0, false, false>": "check_conv_fwd",
    "conv_tileM_kernel<1, 2, 0, 0, false, false>": "check_conv_fwd",
    "conv_tileM_kernel<9, 1, 0, 0, false, false>": "check_conv_fwd",
    "conv_tile_kernel<1, 1, 0, false, 0, false, false, false, 2>": "check_conv_fwd",
    "conv_tile_kernel<1, 2, 0, false, 0, false, false, false, 2>": "check_conv_fwd",
    "conv_tile_kernel<1, 3, 0, false, 0, false, false, false, 2>": "check_conv_fwd",
    "conv_tile_kernel<9, 1, 0, false, 0, true, false, false, 2>": "check_conv_fwd",
    "conv_tile_kernel<9, 2, 0, false, 0, false, false, false, 2>": "check_conv_fwd",
    "conv_tile_kernel<9, 3, 0, false, 0, false, false, false, 2>": "check_conv_fwd",
    "conv_tileM_kernel<1, 1, 0, 4, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 2, 4, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 2, 6, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 5, 4, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 5, 6, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 0, 2, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 0, 4, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 0, 6, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 2, 4, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 2, 6, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 5, 4, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 5, 6, false, false>": "check_conv_rp",
    "conv_tile_kernel<1, 1, 0, false, 2, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 1, 0, false, 6, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 0, false, 2, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 0, false, 6, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 2, false, 6, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 5, false, 6, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 0, false, 2, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 0, false, 4, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 0, false, 6, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 2, false, 6, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 5, false, 6, false, false, false, 2>": "check_conv_rp",
    "wgrad_1x1_kernel<2, 1, 6>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 2, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 2, 6>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 3, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 3, 6>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 1, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 3, 2>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 3, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 3, 6>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 4, 2>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 4, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 4, 6>": "check_conv_rp",
    "wgrad_1x1w_kernel<3, 2, 2>": "check_conv_rp",
    "wgrad_1x1w_kernel<3, 2, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<3, 2, 6>": "check_conv_rp",
    "wgrad_1x1w_kernel<4, 2, 2>": "check_conv_rp",
    "wgrad_1x1w_kernel<4, 2, 4>": "check_conv_rp",
    "wgrad_1x1w_kernel<4, 2, 6>": "check_conv_rp",
    "conv_tileM_kernel<9, 1, 0, 0, false, true>": "check_conv_up2",
    "conv_tile_kernel<9, 1, 0, false, 0, false, false, true, 2>": "check_conv_up2",
    "conv_tile_kernel<9, 2, 0, false, 0, false, false, true, 2>": "check_conv_up2",
    "conv_tile_kernel<9, 3, 0, false, 0, false, false, true, 2>": "check_conv_up2",
    "wgrad3_kernel<1, 1, 0, true>": "check_conv_up2",
    "wgrad3_kernel<2, 2, 0, true>": "check_conv_up2",
    "wgrad3_kernel<2, 2, 0, false>": "check_conv_wgrad",
    "wgrad_1x1w_kernel<1, 1, 0>": "check_conv_wgrad",
    "wgrad_1x1w_kernel<2, 1, 0>": "check_conv_wgrad",
    "wgrad_1x1w_kernel<2, 2, 0>": "check_conv_wgrad",
    "wgrad_1x1w_kernel<2, 4, 0>": "check_conv_wgrad",
    "wgrad_lds_kernel<9, 1, 1, 0>": "check_conv_wgrad",
    "wgrad_lds_kernel<9, 2, 2, 0>": "check_conv_wgrad",
    "wgrad_reduce_batch_kernel": "check_conv_wgrad",
    "dw_fwd_kernel<float, false>": "check_dw",
    "conv_tileM_kernel<1, 1, 0, 2, true, false>": "check_fused_sources_modes",
    "conv_tileM_kernel<1, 2, 0, 2, true, false>": "check_fused_sources_modes",
    "conv_tile_kernel<1, 1, 6, false, 2, false, false, false, 2>": "check_fused_sources_modes",
    "conv_tile_kernel<1, 2, 0, false, 2, false, true, false, 2>": "check_fused_sources_modes",
    "conv_tile_kernel<1, 2, 6, false, 2, false, false, false, 2>": "check_fused_sources_modes",
    "conv_tile_kernel<1, 3, 0, false, 2, false, true, false, 2>": "check_fused_sources_modes",
    "conv_tile_kernel<1, 3, 6, false, 2, false, false, false, 2>": "check_fused_sources_modes",
    "wgrad_1x1_kernel<1, 1, 2>": "check_fused_sources_modes",
    "wgrad_1x1_kernel<2, 2, 2>": "check_fused_sources_modes",
    "wgrad_1x1w_kernel<1, 2, 2>": "check_fused_sources_modes",
    "wgrad_1x1w_kernel<2, 1, 2>": "check_fused_sources_modes",
    "wgrad_1x1w_kernel<3, 1, 2>": "check_fused_sources_modes",
    "gattn_bwd_kv_mfma_kernel<float>": "check_gattn",
    "gattn_bwd_q_mfma_kernel<float>": "check_gattn",
    "gattn_fwd_mfma_kernel<float>": "check_gattn",
    "copy2d_kernel": "check_layout_utils",
    "fill_kernel": "check_layout_utils",
    "nchw_to_nhwc_kernel<float>": "check_layout_utils",
    "nhwc_to_nchw_kernel<float>": "check_layout_utils",
    "ln_bwd_kernel<32, float>": "check_ln",
    "ln_bwd_kernel<64, float>": "check_ln",
    "conv_tileM_kernel<1, 1, 0, 0, true, false>": "check_ln_linear",
    "conv_tileM_kernel<1, 2, 0, 0, true, false>": "check_ln_linear",
    "conv_tile_kernel<1, 1, 6, false, 0, false, false, false, 2>": "check_ln_linear",
    "conv_tile_kernel<1, 2, 0, false, 0, false, true, false, 2>": "check_ln_linear",
    "conv_tile_kernel<1, 2, 6, false, 0, false, false, false, 2>": "check_ln_linear",
    "conv_tile_kernel<1, 3, 0, false, 0, false, true, false, 2>": "check_ln_linear",
    "conv_tile_kernel<1, 3, 6, false, 0, false, false, false, 2>": "check_ln_linear",
    "wgrad_1x1w_kernel<1, 2, 0>": "check_ln_linear",
    "wgrad_1x1w_kernel<2, 3, 0>": "check_ln_linear",
    "wgrad_1x1w_kernel<3, 1, 0>": "check_ln_linear",
    "wgrad_1x1w_kernel<3, 2, 0>": "check_ln_linear",
    "wgrad_1x1w_kernel<4, 2, 0>": "check_ln_linear",
    "na_bwd_fused_kernel<1, 3, float>": "check_na",
    "na_bwd_fused_kernel<2, 6, float>": "check_na",
    "na_bwd_kv_kernel<4, float>": "check_na",
    "na_bwd_kv_kernel<8, float>": "check_na",
    "na_bwd_q_kernel<4, float>": "check_na",
    "na_bwd_q_kernel<8, float>": "check_na",
    "na_fwd_kernel<1, float>": "check_na",
    "na_fwd_kernel<2, float>": "check_na",
    "na_fwd_kernel<4, float>": "check_na",
    "na_fwd_kernel<8, float>": "check_na",
    "avgpool_bwd_kernel<float>": "check_resample",
    "avgpool_fwd_wave_kernel<float>": "check_resample",
    "up2_bwd_kernel<float>": "check_resample",
    "up2_fwd_kernel<float>": "check_resample",
    "se_fwd_kernel": "check_se",
    "dw_bwd_kernel<float, 0, false, true, 2>": "check_zpath",
    "dw_bwd_kernel<float, 0, true, true, 2>": "check_zpath",
    "dw_fwd_kernel<float, true>": "check_zpath",
    "dw_stats0_kernel<float, true>": "check_zpath",
    "dw_stats1_kernel<float, true>": "check_zpath",
    "reparam_fold_kernel": "check_zpath",
    "reparam_wfin_kernel": "check_zpath",
    "segloss_bwd_kernel<2>": "tests/test_multiclass_kernels_gpu.py::test_two_class_loss_vs_f64_owns_the_step_kernels",
    "segloss_finish_kernel": "tests/test_multiclass_kernels_gpu.py::test_two_class_loss_vs_f64_owns_the_step_kernels",
    "segloss_sums_kernel<2>": "tests/test_multiclass_kernels_gpu.py::test_two_class_loss_vs_f64_owns_the_step_kernels",
    "adamw_kernel": "tests/test_optim_kernels_gpu.py::test_plain_adamw_step_vs_f64_owns_the_step_kernel",
}

# ---- the wider envelope (tests/test_kernel_census_envelope_gpu.py): wide variants, na_kernel_size 5 / 7, "bf16-mma", other class counts
_WIDE = "tests/test_wide_kernels_gpu.py::"
OWNED.update({
    # general neighbourhood attention, any head dim: <lanes per head, vector width, register array> (csrc/na_gen.hip LMN_NG_SELECT);
    # both storages against oracle/natten_ref.py in float64
    "na_any_%s_kernel<%s, %s>" % (k, a, t): _WIDE + "test_na_general_head_dims_vs_oracle_f64"
    for k in ("fwd", "bwd_q", "bwd_kv")
    for a in ("1, 1, 8", "1, 2, 8", "1, 4, 16", "1, 1, 32", "2, 1, 16", "2, 2, 16", "2, 4, 16")
    for t in ("float", "__bf16")
})
OWNED.update({
    "gattn_bwd_kv_kernel<128, float>": _WIDE + "test_gattn_wide_head_dim_vs_f64",
    "gattn_bwd_kv_kernel<64, float>": _WIDE + "test_gattn_wide_head_dim_vs_f64",
    "gattn_bwd_q_kernel<128, float>": _WIDE + "test_gattn_wide_head_dim_vs_f64",
    "gattn_bwd_q_kernel<64, float>": _WIDE + "test_gattn_wide_head_dim_vs_f64",
    "gattn_fwd_kernel<128, float>": _WIDE + "test_gattn_wide_head_dim_vs_f64",
    "gattn_fwd_kernel<64, float>": _WIDE + "test_gattn_wide_head_dim_vs_f64",
    "ln_bwd_wide_kernel<float>": _WIDE + "test_layernorm_wide_rows_vs_f64",
    "ln_fwd_wide_kernel<float>": _WIDE + "test_layernorm_wide_rows_vs_f64",
    "gattn_bwd_kv_kernel<128, __bf16>": "check_wide_bf16_rows",
    "gattn_bwd_kv_kernel<64, __bf16>": "check_wide_bf16_rows",
    "gattn_bwd_q_kernel<128, __bf16>": "check_wide_bf16_rows",
    "gattn_bwd_q_kernel<64, __bf16>": "check_wide_bf16_rows",
    "gattn_fwd_kernel<128, __bf16>": "check_wide_bf16_rows",
    "gattn_fwd_kernel<64, __bf16>": "check_wide_bf16_rows",
    "ln_bwd_wide_kernel<__bf16>": "check_wide_bf16_rows",
    "ln_fwd_wide_kernel<__bf16>": "check_wide_bf16_rows",
    "na_bwd_kv_kernel<16, float>": "check_na_hd16",
    "na_bwd_q_kernel<16, float>": "check_na_hd16",
    "na_fwd_kernel<16, float>": "check_na_hd16",
})
OWNED.update({"na_%s_gen_kernel<%d, float>" % (k, hd): "check_na" for k in ("fwd", "bwd_q", "bwd_kv") for hd in (1, 2, 4, 8, 16)})
OWNED.update({"na_%s_gen_kernel<%d, __bf16>" % (k, hd): "check_wide_bf16_rows" for k in ("fwd", "bwd_q", "bwd_kv") for hd in (1, 2, 4, 8, 16)})
# the rest of the envelope's list: other template arguments of the conv, weight-gradient, depthwise and row kernels ("bf16-mma": operand
# type 1 / 5; wide variants: other tile shapes; deploy-mode bf16).  Each owner holds a case at the channel counts that select the instance
OWNED.update({
    "dw_bwd_kernel<__bf16, 0, false, false, 2>": "check_bf16_storage_rows",
    "dw_fwd_kernel<__bf16, false>": "check_bf16_storage_rows",
    "dw_stats0_kernel<__bf16, false>": "check_bf16_storage_rows",
    "dw_stats1_kernel<__bf16, false>": "check_bf16_storage_rows",
    "conv_tileM_kernel<1, 1, 3, 4, false, false>": "check_bn_bwd_rp_wide",
    "conv_tileM_kernel<1, 1, 3, 6, false, false>": "check_bn_bwd_rp_wide",
    "conv_tileM_kernel<1, 1, 4, 4, false, false>": "check_bn_bwd_rp_wide",
    "conv_tileM_kernel<1, 1, 4, 6, false, false>": "check_bn_bwd_rp_wide",
    "conv_tileM_kernel<9, 1, 0, 1, false, false>": "check_conv3_storage",
    "conv_tileM_kernel<9, 1, 2, 2, false, false>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 0, 1, false, false>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 0, 1, false, true>": "check_conv3_storage",
    "conv_tileM_kernel<9, 2, 2, 1, false, false>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, false, 0, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, false, 1, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, false, 1, true, false, true, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 0, true, 1, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 1, 2, false, 1, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, false, 1, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, false, 1, false, false, true, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, false, 1, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 0, true, 1, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 2, 2, false, 1, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, false, 1, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, false, 1, false, false, true, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, false, 2, true, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 0, true, 1, false, false, false, 2>": "check_conv3_storage",
    "conv_tile_kernel<9, 3, 2, false, 1, false, false, false, 2>": "check_conv3_storage",
    "wgrad3_kernel<1, 1, 1, false>": "check_conv3_storage",
    "wgrad3_kernel<1, 1, 1, true>": "check_conv3_storage",
    "wgrad3_kernel<2, 2, 1, false>": "check_conv3_storage",
    "wgrad3_kernel<2, 2, 1, true>": "check_conv3_storage",
    "wgrad_lds_kernel<9, 1, 1, 1>": "check_conv3_storage",
    "wgrad_lds_kernel<9, 2, 2, 1>": "check_conv3_storage",
    "wgrad_1x1w_kernel<1, 1, 1>": "check_conv_bf16",
    "wgrad_1x1w_kernel<2, 2, 1>": "check_conv_bf16",
    "conv_tileM_kernel<1, 1, 1, 1, false, false>": "check_conv_bn_epilogues",
    "conv_tileM_kernel<1, 2, 1, 1, false, false>": "check_conv_bn_epilogues",
    "conv_tile_kernel<1, 2, 1, false, 1, false, false, false, 2>": "check_conv_bn_epilogues",
    "conv_tile_kernel<1, 3, 1, false, 1, false, false, false, 2>": "check_conv_bn_epilogues",
    "conv_tileM_kernel<1, 1, 0, 1, true, false>": "check_conv_mma_forms",
    "conv_tileM_kernel<1, 2, 0, 1, true, false>": "check_conv_mma_forms",
    "conv_tile_kernel<1, 1, 6, false, 1, false, false, false, 2>": "check_conv_mma_forms",
    "conv_tile_kernel<1, 2, 0, false, 1, false, true, false, 2>": "check_conv_mma_forms",
    "conv_tile_kernel<1, 2, 6, false, 1, false, false, false, 2>": "check_conv_mma_forms",
    "conv_tile_kernel<1, 3, 0, false, 1, false, true, false, 2>": "check_conv_mma_forms",
    "conv_tile_kernel<1, 3, 6, false, 1, false, false, false, 2>": "check_conv_mma_forms",
    "wgrad_1x1w_kernel<3, 1, 1>": "check_conv_mma_forms",
    "conv_tileM_kernel<1, 1, 0, 2, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 0, 6, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 2, 0, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 2, 2, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 2, 5, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 1, 5, 5, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 0, 1, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 0, 5, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 2, 5, false, false>": "check_conv_rp",
    "conv_tileM_kernel<1, 2, 5, 5, false, false>": "check_conv_rp",
    "conv_tile_kernel<1, 1, 0, false, 1, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 1, 0, false, 5, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 0, false, 1, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 0, false, 5, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 2, false, 5, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 2, 5, false, 5, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 0, false, 1, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 0, false, 5, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 2, false, 5, false, false, false, 2>": "check_conv_rp",
    "conv_tile_kernel<1, 3, 5, false, 5, false, false, false, 2>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 2, 1>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 2, 5>": "check_conv_rp",
    "wgrad_1x1w_kernel<1, 3, 5>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 1, 1>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 1, 5>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 3, 1>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 3, 5>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 4, 1>": "check_conv_rp",
    "wgrad_1x1w_kernel<2, 4, 5>": "check_conv_rp",
    "wgrad_1x1w_kernel<3, 2, 1>": "check_conv_rp",
    "wgrad_1x1w_kernel<3, 2, 5>": "check_conv_rp",
    "wgrad_1x1w_kernel<4, 2, 1>": "check_conv_rp",
    "wgrad_1x1w_kernel<4, 2, 5>": "check_conv_rp",
    "dw_bwd_kernel<float, 0, false, false, 2>": "check_dw",
    "dw_merge_kernel": "check_dw",
    "dw_stats0_kernel<float, false>": "check_dw",
    "dw_stats1_kernel<float, false>": "check_dw",
    "conv_tileM_kernel<9, 1, 0, 2, false, true>": "check_fused_sources_modes",
    "up2_fwd_kernel<__bf16>": "check_fused_sources_modes",
    "wgrad_1x1_kernel<3, 1, 2>": "check_fused_sources_modes",
    "ln_bwd_kernel<16, float>": "check_ln",
    "avgpool_fwd_kernel<__bf16>": "check_rows_envelope",
    "avgpool_fwd_kernel<float>": "check_rows_envelope",
    "bnact_fwd_kernel<__bf16>": "check_rows_envelope",
    "ln_bwd_kernel<16, __bf16>": "check_rows_envelope",
    "se_bwd_params_kernel": "check_se",
    "wgrad_1x1_kernel<1, 3, 2>": "check_wgrad_1x1_envelope",
    "wgrad_1x1_kernel<3, 1, 6>": "check_wgrad_1x1_envelope",
    "wgrad_1x1w_kernel<1, 3, 0>": "check_wgrad_1x1_envelope",
    "wgrad_1x1w_kernel<1, 4, 4>": "check_wgrad_1x1_envelope",
    "wgrad_1x1w_kernel<1, 4, 6>": "check_wgrad_1x1_envelope",
    "wgrad_1x1w_kernel<3, 1, 4>": "check_wgrad_1x1_envelope",
    "wgrad_1x1w_kernel<4, 1, 0>": "check_wgrad_1x1_envelope",
    "segloss_bwd_gen_kernel": "tests/test_multiclass_kernels_gpu.py::test_general_c_loss_vs_f64",
    "segloss_sums_gen_kernel": "tests/test_multiclass_kernels_gpu.py::test_general_c_loss_vs_f64",
})
