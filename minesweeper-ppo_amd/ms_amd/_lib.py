"""ctypes binding of libmsenv.so: the one table of the whole C ABI (the seven headers under
include/), bound once by load(). tests/test_abi_signatures.py checks every entry, the struct
mirrors and the constants below against the headers. The four additions of
include/msposterior_grouped.h sit in a table of their own, SIGNATURES_GROUPED, which load() binds
too and tests/test_posterior_grouped_host.py checks against that header. Likewise the additions
of include/msexpert.h and include/msbc.h: SIGNATURES_EXPERT and SIGNATURES_BC, and the struct
mirror McBcLossArgs, checked by tests/test_expert_host.py; and those of include/mssym.h:
SIGNATURES_SYM, checked by tests/test_symmetry_host.py; and the one of include/msdagger.h:
SIGNATURES_DAGGER, checked by tests/test_dagger_host.py; and the three of include/mslookahead.h:
SIGNATURES_LOOKAHEAD, checked by tests/test_lookahead_host.py.

torch is imported first so that the HIP runtime torch ships is the one the
library binds to (both carry SONAME libamdhip64.so.7; the loader reuses the
already-mapped one). A second runtime in the process would make torch's
streams and pointers invalid for our kernels, so load() verifies that exactly
one libamdhip64 is mapped. There is no CPU fallback: if the library is
missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MSENV_LIB may point at libmsenv_diag.so (tools/diag_step.py); default is the product build
LIB_PATH = os.environ.get("MSENV_LIB") or os.path.join(PKG_DIR, "libmsenv.so")
ABI_VERSION = 3  # MSENV_ABI_VERSION

MS_OUTCOME_NONE, MS_OUTCOME_WIN, MS_OUTCOME_LOSS = 0, 1, 2
MS_TAPE_UNIFORM, MS_TAPE_SAFE_BIASED = 0, 1
MS_LATE_SHARED, MS_LATE_KEYED = 0, 1


class MsEnvError(RuntimeError):
    """Raised when a C ABI call returns a nonzero status."""


class MsCfg(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("mine_count", ctypes.c_int32),
                ("guarantee_safe_neighborhood", ctypes.c_int32), ("win_reward", ctypes.c_double),
                ("loss_reward", ctypes.c_double), ("step_penalty", ctypes.c_double)]


_vp, _i64, _u64, _i32, _f32 = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32,
                               ctypes.c_float)


class McFwdLayer(ctypes.Structure):  # mc_fwd_layer (mscnn.h)
    _fields_ = [(n, _vp) for n in ("w", "bias", "gamma", "beta", "dmask", "out", "ysave", "stats", "relu_mask")]


class McBwdLayer(ctypes.Structure):  # mc_bwd_layer (mscnn.h)
    _fields_ = [(n, _vp) for n in ("ysave", "stats", "gamma", "relu_mask", "dmask", "wT", "dy")]


class McPpoLossArgs(ctypes.Structure):  # mc_ppo_loss_args (msppo.h)
    _fields_ = [(n, _vp) for n in ("logits", "action_mask", "actions", "old_logp", "advantages", "values", "returns",
                                   "vpred", "mine", "labels", "valid", "counts")] + \
        [("vpred_dtype", _i32), ("mine_round", _i32)] + \
        [(n, _f32) for n in ("clip_eps", "clip_eps_v", "vf_coef", "ent_coef", "aux_mine_weight",
                             "aux_mine_calib_weight", "mask_fill", "world")] + \
        [("M", _i64), ("A", _i32)]


class McBcLossArgs(ctypes.Structure):  # mc_bc_loss_args (msbc.h)
    _fields_ = [(n, _vp) for n in ("logits", "action_mask", "best", "weight", "mine", "labels", "valid", "counts")] + \
        [(n, _f32) for n in ("mask_fill", "ent_coef", "aux_mine_weight", "aux_mine_calib_weight", "world")] + \
        [("M", _i64), ("A", _i32)]


_lib = None

# name -> argtypes (restype int unless listed in _RESTYPES)
SIGNATURES = {
    "ms_last_error": [],
    "ms_abi_version": [],
    "ms_create": [ctypes.POINTER(MsCfg), _i64, _u64, _i64, _i64, ctypes.POINTER(_vp)],
    "ms_destroy": [_vp],
    "ms_reset": [_vp, _vp, _vp, _vp],
    "ms_step": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ms_step_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ms_step_codes": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ms_labels": [_vp, _vp, _vp, _vp],
    "ms_snapshot": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ms_rng_state": [_vp, _vp, _vp],
    "ms_tape_actions": [_vp, _u64, _i32, _vp, _vp],
    "ms_run_tape": [_vp, _u64, _i32, _i32, _i32] + [_vp] * 10,
    "ms_gae": [_vp, _vp, _vp, _vp, _i32, _i64, _f32, _f32, _vp, _vp, _vp],
    "ms_sample_masked": [_vp, _vp, _i64, _i32, _i64, _u64, _u64, _vp, _vp, _vp],
    "ms_dropout_masks": [_vp, _i64, _i32, _i32, _u64, _u64, _f32, _vp, _vp],
    "ms_set_late_start": [_vp, ctypes.c_double, _i32, _i32, _i32, _i32, _u64],
    "ms_set_late_start_mode": [_vp, _i32],
    "ms_late_rng_state": [_vp, _vp],
    # msenv_debug.h
    "ms_set_debug_flags": [_vp, ctypes.c_uint32],
    "ms_set_diag": [_vp, _vp],
    "ms_set_timing_events": [_vp, _vp, _vp],
    "ms_event_create": [ctypes.POINTER(_vp)],
    "ms_event_elapsed_ms": [_vp, _vp, ctypes.POINTER(ctypes.c_float)],
    "ms_event_destroy": [_vp],
    # mssolve.h: ten output pointers each (status .. comp_size)
    "ms_avoid": [_vp, _vp, _vp] + [_vp] * 10 + [_vp],
    "ms_avoid_states": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 10 + [_vp],
    "ms_avoid_host": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32] + [_vp] * 10,
    "ms_avoid_set_budget": [_vp, _i32],
    # msposterior.h: four output pointers each (status, prob, configs, max_nodes)
    "ms_posterior": [_vp, _vp] + [_vp] * 4 + [_vp],
    "ms_posterior_states": [_vp, _vp, _i32, _vp, _i64, _i32, _i32, _i32] + [_vp] * 4 + [_vp],
    "ms_posterior_host": [_vp, _vp, _i32, _vp, _i64, _i32, _i32, _i64] + [_vp] * 4,
    "ms_posterior_set_budget": [_vp, _i32],
    # handle, budget, labels, valid, source, max_nodes, stream
    "ms_posterior_labels": [_vp, _i32, _vp, _vp, _vp, _vp, _vp],
    # mscnn.h
    "mc_obs_encode": [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp],
    "mc_codes_to_nhwc": [_vp, _vp, _i64, _i32, _i32, _i32, _vp],
    "mc_conv_gn_fwd": [_vp] * 11 + [_i32] * 4 + [_f32, _i32, _vp],
    "mc_conv_gn_bwd": [_vp] * 16 + [_i64] + [_i32] * 5 + [_vp],
    "mc_conv_gn_bwd_workspace": [_i32] * 4,
    "mc_conv_wgrad": [_vp] * 4 + [_i64] + [_i32] * 5 + [_vp],
    "mc_conv_wgrad_gn": [_vp] * 8 + [_i64] + [_i32] * 4 + [_vp],
    "mc_trunk_fwd_workspace": [_i32] * 3,
    "mc_trunk_fwd": [_vp, ctypes.POINTER(McFwdLayer), _i32, _vp, _i64] + [_i32] * 3 + [_f32, _i32, _vp],
    "mc_trunk_fwd_pooled": [_vp, ctypes.POINTER(McFwdLayer), _i32, _vp, _i64, _vp] + [_i32] * 3 + [_f32, _i32, _vp],
    "mc_trunk_bwd_workspace": [_i32] * 4,
    "mc_trunk_bwd": [_vp, ctypes.POINTER(McBwdLayer), _i32, _vp, _vp, _i64] + [_i32] * 4 + [_vp],
    "mc_heads_fwd": [_vp] * 7 + [_i64, _i32, _vp],
    "mc_heads_bwd": [_vp] * 8 + [_i32] + [_vp] * 5 + [_i64, _i64, _i32, _vp],
    "mc_heads_bwd_workspace": [_i64],
    "mc_last_error": [],
    # msppo.h
    "mc_ppo_loss_workspace": [_i64],
    "mc_ppo_loss_fwd": [ctypes.POINTER(McPpoLossArgs), _vp, _vp, _i64, _vp],
    "mc_ppo_loss_bwd": [ctypes.POINTER(McPpoLossArgs), _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    # msenv_debug.h: kernel variants, and the MC_DIAG stamp hooks (DIAG_ONLY)
    "mc_set_variant": [_i32, _i32],
    "mc_set_fwd_diag": [_vp],
    "mc_set_trunk_diag": [_vp, _vp],
    "mc_set_trunk_dflags": [ctypes.c_int],
    "mc_set_heads_diag": [_vp],
}
# include/msposterior_grouped.h (tests/test_posterior_grouped_host.py checks this table against it):
# the counterparts' parameter lists
SIGNATURES_GROUPED = {
    "ms_posterior_grouped": SIGNATURES["ms_posterior"],
    "ms_posterior_states_grouped": SIGNATURES["ms_posterior_states"],
    "ms_posterior_host_grouped": SIGNATURES["ms_posterior_host"],
    "ms_posterior_labels_grouped": SIGNATURES["ms_posterior_labels"],
}
# include/msexpert.h: status, prob, hidden, n, A, then five output pointers (best .. labels)
SIGNATURES_EXPERT = {
    "ms_expert_targets": [_vp, _vp, _vp, _i64, _i32] + [_vp] * 5 + [_vp],
    "ms_expert_targets_host": [_vp, _vp, _vp, _i64, _i32] + [_vp] * 5,
}
# include/msbc.h
SIGNATURES_BC = {
    "mc_bc_loss_workspace": [_i64],
    "mc_bc_loss_fwd": [ctypes.POINTER(McBcLossArgs), _vp, _vp, _i64, _vp],
    "mc_bc_loss_bwd": [ctypes.POINTER(McBcLossArgs), _vp, _vp, _i64, _vp, _vp, _vp],
}
# include/mssym.h
SIGNATURES_SYM = {
    "ms_sym_cell_map_host": [_i32, _i32, _i32, _vp],
    # rows, g, n, H, W, B_src, five source planes, five output planes, status, stream
    "ms_sym_gather": [_vp, _vp, _i64, _i32, _i32, _i64] + [_vp] * 5 + [_vp] * 5 + [_vp, _vp],
    "ms_sym_expand": [_vp, _i64, _i32, _i32, _i32, _vp, _vp],
    "ms_sym_mean": [_vp, _i64, _i32, _i32, _i32, _vp, _vp],
}
# include/msdagger.h: logits, mask, best, expert_action, kind, n, A, row_begin, seed, counter, beta,
# explore, mode, then four output pointers (action .. agree), stream
SIGNATURES_DAGGER = {
    "ms_dagger_act": [_vp] * 5 + [_i64, _i32, _i64, _u64, _u64, _f32, _f32, _i32] + [_vp] * 4 + [_vp],
}
# include/mslookahead.h
_f64 = ctypes.c_double
SIGNATURES_LOOKAHEAD = {
    # status, prob, revealed, number, n, H, W, K, margin, cap, then six output pointers (slot .. live2), stream
    "ms_lookahead_expand": [_vp] * 4 + [_i64, _i32, _i32, _i32, _f64, _i64] + [_vp] * 6 + [_vp],
    # slot, cand, prob, configs, status2, prob2, configs2, revealed2, mine_count, n, H, W, K, cap, then four
    # output pointers (action .. changed), stream
    "ms_lookahead_score": [_vp] * 8 + [_i32, _i64, _i32, _i32, _i32, _i64] + [_vp] * 4 + [_vp],
    # status, prob, configs, revealed, number, mine_count, n, H, W, K, margin, cap, budget, grouped, then seven
    # output pointers (slot, count, cand, action, score, n_scored, changed)
    "ms_lookahead_host": [_vp] * 5 + [_i32, _i64, _i32, _i32, _i32, _f64, _i64, _i64, _i32] + [_vp] * 7,
}
MS_LOOKAHEAD_MAX_K, MS_LOOKAHEAD_OUTCOMES, MS_LOOKAHEAD_SCORED_RTOL = 16, 9, 1e-9
MS_DAGGER_GREEDY, MS_DAGGER_SAMPLE = 0, 1
MS_DAGGER_SRC_UNIFORM, MS_DAGGER_SRC_EXPERT, MS_DAGGER_SRC_LEARNER = 0, 1, 2
MS_DAGGER_MAX_CELLS = 3968
MS_DAGGER_C_LEARNER = 0xA0761D6478BD642F
MS_DAGGER_C_BETA = 0xE7037ED1A0B428DB
MS_DAGGER_C_EXPLORE = 0x8EBC6AF09C88C6E3
# the four per-row outputs of ms_dagger_act, in argument order
DAGGER_OUTPUTS = (("action", "int64"), ("source", "uint8"), ("learner_action", "int64"), ("agree", "uint8"))
# the five planes of ms_sym_gather (ExpertBuffer.FIELDS), in argument order: name, dtype, per-cell
SYM_PLANES = (("codes", "uint8", True), ("mask", "uint8", True), ("best", "uint8", True),
              ("labels", "float32", True), ("kind", "uint8", False))
MS_EXPERT_NONE, MS_EXPERT_SAFE, MS_EXPERT_GUESS = 0, 1, 2
# the five per-board outputs of the ms_expert_targets* entry points, in argument order
EXPERT_OUTPUTS = (("best", "uint8", True), ("action", "int64", False), ("kind", "uint8", False),
                  ("n_best", "int32", False), ("labels", "float32", True))
POSTERIOR_METHODS = ("enumerate", "grouped")
MS_POSTERIOR_MAX_GROUPS = 128
# declared under #ifdef MC_DIAG: libmsenv_diag.so exports them, the product build does not
DIAG_ONLY = frozenset(("mc_set_fwd_diag", "mc_set_trunk_diag", "mc_set_trunk_dflags", "mc_set_heads_diag"))
MS_AVOID_SKIPPED, MS_AVOID_DECIDED, MS_AVOID_UNDECIDED = 0, 1, 2
MS_AVOID_DEFAULT_BUDGET = 1 << 18
MS_AVOID_MAX_VARS, MS_AVOID_MAX_CELLS = 128, 512
# the ten per-env outputs of the ms_avoid* entry points, in argument order: name, dtype, per-cell
AVOID_OUTPUTS = (("status", "uint8", False), ("avoidable", "uint8", False), ("n_safe", "int32", False),
                 ("chosen_safe", "uint8", False), ("chosen_comp", "int32", False), ("n_comp", "int32", False),
                 ("n_frontier", "int32", False), ("safe_mask", "uint8", True), ("max_nodes", "int32", False),
                 ("comp_size", "int32", True))
MS_POSTERIOR_DEFAULT_BUDGET = 1 << 16
# `source` of ms_posterior_labels: before the first click, the exact posterior, the mine mask
MS_LABELS_NONE, MS_LABELS_POSTERIOR, MS_LABELS_HARD = 0, 1, 2
# the four per-env outputs of the ms_posterior* entry points, in argument order
POSTERIOR_OUTPUTS = (("status", "uint8", False), ("prob", "float64", True), ("configs", "float64", False),
                     ("max_nodes", "int32", False))
MS_DBG_FORCE_SERIAL_PLACEMENT = 1
MS_DBG_FORCE_CHAIN_PLACEMENT = 2
MS_DBG_ONE_BOARD_PER_WAVE = 4  # ms_step without the lane-packed small-board kernel
MS_DBG_TWO_BOARDS_PER_WAVE = 8  # the lane-packed kernel with 32-lane groups
MS_DBG_FORCE_PACKED = 16  # 16x16: the lane-packed kernel below its env-count threshold too
MC_DTYPE_BF16, MC_DTYPE_F16 = 0, 1
MC_TRUNK_MAX_LAYERS = 16
MC_VAR_FWD, MC_VAR_BWD, MC_VAR_WGRAD, MC_VAR_TRUNK_FWD = 0, 1, 2, 3  # mc_set_variant kernels
_RESTYPES = {"ms_last_error": ctypes.c_char_p, "ms_abi_version": ctypes.c_int32, "mc_last_error": ctypes.c_char_p,
             **{n: _i64 for n in ("mc_conv_gn_bwd_workspace", "mc_trunk_fwd_workspace", "mc_trunk_bwd_workspace",
                                  "mc_heads_bwd_workspace", "mc_ppo_loss_workspace", "mc_bc_loss_workspace")},
             **{n: None for n in DIAG_ONLY}}


def _hip_runtimes_mapped() -> set[str]:
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    paths.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    return paths


def load():
    """Load libmsenv.so (once) and declare every C ABI signature."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MsEnvError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
                         " (or `make -C minesweeper-ppo_amd`)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in {**SIGNATURES, **SIGNATURES_GROUPED, **SIGNATURES_EXPERT, **SIGNATURES_BC,
                           **SIGNATURES_SYM, **SIGNATURES_DAGGER, **SIGNATURES_LOOKAHEAD}.items():
        if name in DIAG_ONLY and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    if lib.ms_abi_version() != ABI_VERSION:
        raise MsEnvError(f"libmsenv ABI {lib.ms_abi_version()} != expected {ABI_VERSION}")
    runtimes = _hip_runtimes_mapped()
    if len(runtimes) > 1:
        raise MsEnvError(f"more than one HIP runtime mapped in this process: {sorted(runtimes)}")
    _lib = lib
    return lib


def posterior_entry(name: str, method: str):
    """The entry point ``name`` of msposterior.h / msposterior_labels.h (method "enumerate") or its
    msposterior_grouped.h counterpart ("grouped")."""
    if method not in POSTERIOR_METHODS:
        raise ValueError(f"method: expected one of {POSTERIOR_METHODS}, got {method!r}")
    return getattr(load(), name if method == "enumerate" else name + "_grouped")


def check(rc: int) -> None:
    if rc != 0:
        raise MsEnvError(load().ms_last_error().decode(errors="replace"))


def check_mc(rc: int) -> None:
    if rc != 0:
        raise MsEnvError(load().mc_last_error().decode(errors="replace"))


def ptr(t) -> int | None:
    """data_ptr of a tensor (None passes NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream
