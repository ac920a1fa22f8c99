"""ctypes binding of libhftlob.so (the HIP/gfx950 library behind include/hftlob.h).

There is deliberately no CPU fallback: if the library is missing, or a call
is made without a GPU, this module raises.  The CPU restatement under
``oracle/`` is test infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os

from .layout import EnvCfg, LobCfg, StepOut


class LaunchInfo(C.Structure):
    """hftlob_launch_info (include/hftlob.h): the kernel instantiation a config launches."""
    _fields_ = [("slot_sets", C.c_int32), ("nfix", C.c_int32), ("random_cancel", C.c_int32),
                ("rows_alias", C.c_int32), ("lds_bytes", C.c_int32), ("tick_magic", C.c_uint32),
                ("key_batch", C.c_int32)]

class AdamTensor(C.Structure):
    """hftlob_adam_tensor (include/hftlob.h): one parameter tensor of hftlob_adam_clip."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_void_p),
                ("n", C.c_longlong)]


class GruFwdGroup(C.Structure):
    """hftlob_gru_fwd_group (include/hftlob.h): one group of hftlob_gru_scan_fwd_grouped."""
    _fields_ = [("B", C.c_int)] + [(k, C.c_void_p) for k in ("gi", "h0", "done", "w_hh", "b_hh", "hseq", "gates")]


class GruBwdGroup(C.Structure):
    """hftlob_gru_bwd_group (include/hftlob.h): one group of hftlob_gru_scan_bwd_grouped."""
    _fields_ = [("B", C.c_int)] + [(k, C.c_void_p) for k in ("d_hseq", "hseq", "gates", "h0", "done", "w_hh", "d_gi",
                                                             "d_gh_n", "d_h0")]


class PolicyWeights(C.Structure):
    """hftlob_policy_weights (include/hftlob.h): device pointers of one ActorCriticRNN's parameters."""
    _fields_ = [(n, C.c_void_p) for n in ("w_embed", "b_embed", "w_ih", "b_ih", "w_hh", "b_hh", "w_c1", "b_c1",
                                          "w_c2", "b_c2", "w_a1", "b_a1", "w_a2", "b_a2")]


class PolicyGroup(C.Structure):
    """hftlob_policy_group (include/hftlob.h): one group of hftlob_policy_step_grouped."""
    _fields_ = ([("B", C.c_int), ("D", C.c_int), ("K", C.c_int), ("nvec", C.c_int * 4), ("w", PolicyWeights)]
                + [(k, C.c_void_p) for k in ("obs", "done", "h_in", "h_out", "keys", "action", "log_prob", "value",
                                             "logits")])


LIB_PATH = os.environ.get("HFTLOB_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhftlob.so")
ABI_VERSION = 8
EVAL_WORDS = 106  # HFTLOB_EVAL_WORDS: doubles per agent in hftlob_env_rollout_eval's stats (the table is in hftlob.h)
EPISODE_WORDS = 26  # HFTLOB_EPISODE_WORDS: doubles per (env, agent, completed episode) in the episodes buffers
DIAG_WORDS = 86  # HFTLOB_DIAG_WORDS: doubles of hftlob_rollout_diag's result (the table is in hftlob.h)
DIAG_MAX_HEADS, DIAG_MAX_ACTIONS = 4, 16  # HFTLOB_DIAG_MAX_HEADS, HFTLOB_DIAG_MAX_ACTIONS
DIAG_STRIPE_ROWS, DIAG_MAX_STRIPES = 1024, 256  # HFTLOB_DIAG_STRIPE_ROWS, HFTLOB_DIAG_MAX_STRIPES: the stripe rule
WORLD_TALLY_WORDS = 28  # HFTLOB_WORLD_TALLY_WORDS: doubles per env in hftlob_world_tally's wstats
EXPORTS = ("hftlob_version", "hftlob_last_error", "hftlob_book_process", "hftlob_book_depth",
           "hftlob_book_process_depth", "hftlob_env_reset",
           "hftlob_env_step", "hftlob_env_step_sampled", "hftlob_env_rollout_sampled", "hftlob_rollout_prepare",
           "hftlob_env_rollout_actions", "hftlob_env_rollout_eval", "hftlob_eval_tally",
           "hftlob_draw_actions", "hftlob_env_rollout_eval_drawn",
           "hftlob_env_rollout_eval_episodes", "hftlob_env_rollout_eval_drawn_episodes", "hftlob_eval_tally_episodes",
           "hftlob_env_lds_bytes", "hftlob_env_launch_info", "hftlob_env_baked_id", "hftlob_set_baked",
           "hftlob_sample_actions", "hftlob_split_keys", "hftlob_gru_scan_fwd", "hftlob_gru_scan_bwd",
           "hftlob_gru_scan_fwd_grouped", "hftlob_gru_scan_bwd_grouped",
           "hftlob_policy_step", "hftlob_policy_step_multi", "hftlob_policy_step_grouped", "hftlob_gae", "hftlob_ppo_loss",
           "hftlob_adam_clip", "hftlob_xty", "hftlob_xty_workspace", "hftlob_xty_wide", "hftlob_xty_wide_workspace",
           "hftlob_rollout_diag", "hftlob_rollout_diag_workspace", "hftlob_world_tally")

_lib = None


class HftlobError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hftlob error {code}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.hftlob_version.restype = i32
    L.hftlob_last_error.restype = C.c_char_p
    L.hftlob_book_process.argtypes = [C.POINTER(LobCfg), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hftlob_book_process.restype = i32
    L.hftlob_book_depth.argtypes = [C.POINTER(LobCfg), i32, i32, vp, vp, vp, vp]
    L.hftlob_book_depth.restype = i32
    L.hftlob_book_process_depth.argtypes = [C.POINTER(LobCfg), i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.hftlob_book_process_depth.restype = i32
    L.hftlob_env_reset.argtypes = [C.POINTER(EnvCfg), i32, vp, vp, vp, vp, C.POINTER(StepOut), vp]
    L.hftlob_env_reset.restype = i32
    L.hftlob_env_step.argtypes = [C.POINTER(EnvCfg), i32, vp, vp, vp, vp, vp, C.POINTER(StepOut), vp]
    L.hftlob_env_step.restype = i32
    L.hftlob_env_step_sampled.argtypes = [C.POINTER(EnvCfg), i32, vp, vp, vp, vp, vp, vp, C.POINTER(StepOut), vp]
    L.hftlob_env_step_sampled.restype = i32
    L.hftlob_env_rollout_sampled.argtypes = [C.POINTER(EnvCfg), i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp,
                                             C.POINTER(StepOut), i32, i32, vp]
    L.hftlob_env_rollout_sampled.restype = i32
    L.hftlob_env_rollout_actions.argtypes = [C.POINTER(EnvCfg), i32, i32, vp, vp, vp, vp, vp, C.POINTER(StepOut), i32, vp]
    L.hftlob_env_rollout_actions.restype = i32
    L.hftlob_env_rollout_eval.argtypes = [C.POINTER(EnvCfg), i32, i32, vp, vp, i32, vp, vp, vp, vp, C.POINTER(StepOut), vp]
    L.hftlob_env_rollout_eval.restype = i32
    L.hftlob_eval_tally.argtypes = [i32, i32, i32, i32, vp, vp, vp, C.POINTER(C.c_uint32), vp, vp]
    L.hftlob_eval_tally.restype = i32
    L.hftlob_draw_actions.argtypes = [i32, i32, C.c_uint32, vp, vp, vp]
    L.hftlob_draw_actions.restype = i32
    L.hftlob_env_rollout_eval_drawn.argtypes = [C.POINTER(EnvCfg), i32, i32, vp, vp, C.POINTER(C.c_uint32), vp, vp, vp, vp,
                                                vp, C.POINTER(StepOut), vp]
    L.hftlob_env_rollout_eval_drawn.restype = i32
    # the three with per-episode records: the sibling's arguments, then `episodes, ep_cap` before the stream
    L.hftlob_env_rollout_eval_episodes.argtypes = L.hftlob_env_rollout_eval.argtypes[:-1] + [vp, i32, vp]
    L.hftlob_env_rollout_eval_episodes.restype = i32
    L.hftlob_eval_tally_episodes.argtypes = L.hftlob_eval_tally.argtypes[:-1] + [vp, i32, vp]
    L.hftlob_eval_tally_episodes.restype = i32
    L.hftlob_env_rollout_eval_drawn_episodes.argtypes = L.hftlob_env_rollout_eval_drawn.argtypes[:-1] + [vp, i32, vp]
    L.hftlob_env_rollout_eval_drawn_episodes.restype = i32
    L.hftlob_rollout_prepare.argtypes = [i32, vp]
    L.hftlob_rollout_prepare.restype = i32
    L.hftlob_env_lds_bytes.argtypes = [C.POINTER(EnvCfg)]
    L.hftlob_env_lds_bytes.restype = i32
    L.hftlob_env_launch_info.argtypes = [C.POINTER(EnvCfg), C.POINTER(LaunchInfo)]
    L.hftlob_env_launch_info.restype = i32
    L.hftlob_env_baked_id.argtypes = [C.POINTER(EnvCfg)]
    L.hftlob_env_baked_id.restype = i32
    L.hftlob_set_baked.argtypes = [i32]
    L.hftlob_set_baked.restype = i32
    L.hftlob_sample_actions.argtypes =[C.POINTER(EnvCfg), i32, vp, vp, vp]
    L.hftlob_sample_actions.restype = i32
    L.hftlob_split_keys.argtypes = [i32, i32, i32, vp, vp, vp]
    L.hftlob_split_keys.restype = i32
    L.hftlob_gru_scan_fwd.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hftlob_gru_scan_fwd.restype = i32
    L.hftlob_gru_scan_bwd.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hftlob_gru_scan_bwd.restype = i32
    L.hftlob_gru_scan_fwd_grouped.argtypes = [i32, i32, i32, C.POINTER(GruFwdGroup), vp]
    L.hftlob_gru_scan_fwd_grouped.restype = i32
    L.hftlob_gru_scan_bwd_grouped.argtypes = [i32, i32, i32, C.POINTER(GruBwdGroup), vp]
    L.hftlob_gru_scan_bwd_grouped.restype = i32
    L.hftlob_policy_step.argtypes = [i32, i32, i32, i32, i32, C.POINTER(PolicyWeights), vp, vp, vp, vp, i32, vp,
                                     vp, vp, vp, vp, vp]
    L.hftlob_policy_step.restype = i32
    L.hftlob_policy_step_multi.argtypes = [i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(PolicyWeights), vp, vp,
                                           vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hftlob_policy_step_multi.restype = i32
    L.hftlob_policy_step_grouped.argtypes = [i32, i32, i32, C.POINTER(PolicyGroup), i32, vp]
    L.hftlob_policy_step_grouped.restype = i32
    L.hftlob_gae.argtypes = [i32, i32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]
    L.hftlob_gae.restype = i32
    L.hftlob_ppo_loss.argtypes = [i32, i32, C.POINTER(i32), vp, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double,
                                  C.c_double, vp, vp, vp, vp, vp]
    L.hftlob_ppo_loss.restype = i32
    L.hftlob_adam_clip.argtypes = [i32, C.POINTER(AdamTensor), vp, C.c_double, C.c_double, C.c_float, C.c_float, vp,
                                   vp, vp]
    L.hftlob_adam_clip.restype = i32
    L.hftlob_xty.argtypes = [C.c_longlong, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.hftlob_xty.restype = i32
    L.hftlob_xty_workspace.argtypes = [C.c_longlong, i32, i32]
    L.hftlob_xty_workspace.restype = C.c_longlong
    L.hftlob_xty_wide.argtypes = [C.c_longlong, i32, vp, i32, C.c_longlong, vp, i32, C.c_longlong, vp, vp, C.c_longlong,
                                  vp, vp, vp, vp, vp]
    L.hftlob_xty_wide.restype = i32
    L.hftlob_xty_wide_workspace.argtypes = [C.c_longlong, i32, i32]
    L.hftlob_xty_wide_workspace.restype = C.c_longlong
    L.hftlob_rollout_diag.argtypes = [C.c_longlong, i32, C.POINTER(i32), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hftlob_rollout_diag.restype = i32
    L.hftlob_rollout_diag_workspace.argtypes = [C.c_longlong]
    L.hftlob_rollout_diag_workspace.restype = C.c_longlong
    L.hftlob_world_tally.argtypes = [i32, i32, i32, vp, C.c_uint32, vp, vp]
    L.hftlob_world_tally.restype = i32
    if L.hftlob_version() != ABI_VERSION:
        raise RuntimeError(f"libhftlob ABI {L.hftlob_version()} != {ABI_VERSION}")
    _lib = L
    return L


def set_baked(on: bool) -> bool:
    """hftlob_set_baked: the process-wide switch of the baked-config kernels (default on; off = every
    launch takes the general kernels, for A/B runs and tests).  Returns the previous setting."""
    return bool(lib().hftlob_set_baked(int(bool(on))))


def check(rc: int) -> None:
    if rc != 0:
        raise HftlobError(rc, lib().hftlob_last_error().decode())


def ptr(t) -> int:
    """Device pointer of a CUDA (HIP) tensor; refuses host tensors loudly."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("hftlob kernels need device (HIP) tensors; got a CPU tensor")
    if not t.is_contiguous():
        raise RuntimeError("hftlob kernels need contiguous tensors")
    return t.data_ptr()


def stream_ptr(stream=None, device=None) -> int:
    """hipStream_t of `stream`, else of torch's current stream on `device` (default: the
    current device)."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return s.cuda_stream
