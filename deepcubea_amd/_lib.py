"""ctypes binding of libdca_hip.so (the C ABI in include/dca.h).

There is NO CPU fallback: if the shared library is missing, or no HIP device is present when a
compute entry point is called, this module raises.  PyTorch-ROCm is used only for device memory,
streams and (elsewhere) the heuristic network.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
from typing import Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdca_hip.so")

ENV_CUBE3, ENV_NPUZZLE, ENV_LIGHTSOUT, ENV_CUBE4 = 0, 1, 2, 3
DT_F32, DT_F16, DT_BF16, DT_F16_PLANES, DT_E4M3, DT_F64 = 0, 1, 2, 4, 5, 6  # (3 is unused)
E4M3 = torch.float8_e4m3fn  # OCP e4m3: the fp8 format of gfx950's matrix pipes
SEM_PY, SEM_CPP = 0, 1
HEUR_MOD97, HEUR_KNUTH3, HEUR_HASHU01, HEUR_ZERO, HEUR_MANHATTAN = 0, 1, 2, 3, 4

_TORCH_DT = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}

# Every entry point the two headers declare, in their order: name -> "return parameters", one letter per C type.  This table is
# the one place that knows how wide a C parameter is: lib() turns it into restype / argtypes, so callers pass plain Python values
# and a wrong width or argument count raises ctypes.ArgumentError / TypeError (tests check it against the headers).
#   parameters  p any pointer (c_void_p: None, an int, byref(...), a ctypes array)   i int   l int64_t   u uint64_t   d double
#   returns     i int   l int64_t   v void   s const char*   b const uint8_t* (a host table)
_CTYPE = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64, "u": C.c_uint64, "d": C.c_double,
          "v": None, "s": C.c_char_p, "b": C.POINTER(C.c_uint8)}
_SIGNATURES = {
    # include/dca.h: the product ABI
    "dca_abi_version": "i",
    "dca_last_error": "s",
    "dca_cube3_perm_table": "b",
    "dca_npuzzle_swap_table": "i ip",
    "dca_cube3_next_state": "i plipp",
    "dca_cube3_prev_state": "i plipp",
    "dca_npuzzle_next_state": "i pliipp",
    "dca_npuzzle_prev_state": "i pliipp",
    "dca_lightsout_next_state": "i pliipp",
    "dca_cube3_expand_fused": "i plpppippp",
    "dca_npuzzle_expand_fused": "i plippippp",
    "dca_lightsout_expand_fused": "i plippippp",
    "dca_cube4_perm_table": "b",
    "dca_cube4_next_state": "i plipp",
    "dca_cube4_prev_state": "i plipp",
    "dca_cube4_expand_fused": "i plpppp",
    "dca_is_solved": "i iiplpp",
    "dca_hash64": "i plipp",
    "dca_nnet_input": "i iiplpp",
    "dca_onehot": "i pliipip",
    "dca_heuristic_builtin": "i iplipp",
    "dca_generate_states": "i iiliiulpppip",
    "dca_bellman_backup": "i ppliippp",
    "dca_hcache_bytes": "l il",
    "dca_hcache_clear": "i pilp",
    "dca_hcache_lookup": "i pilpllpppp",
    "dca_hcache_finish": "i pillpppp",
    "dca_pdb_bytes": "l ii",
    "dca_pdb_build": "i ipippp",
    "dca_pdb_eval": "i ipllippppp",
    "dca_pdb_eval_reflected": "i ipllippppp",
    "dca_cube3_pdb_bytes": "l ii",
    "dca_cube3_pdb_cubies": "i ip",
    "dca_cube3_pdb_index": "i ipipip",
    "dca_cube3_pdb_build": "i ipippp",
    "dca_cube3_pdb_eval": "i plliipppppp",
    "dca_cube3_pdb_eval_sym": "i plliippppipp",
    "dca_cube3_pdb_eval_dual": "i plliippppipp",
    "dca_lightsout_exact_matrix": "i ip",
    "dca_lightsout_exact_eval": "i ipllpp",
    "dca_lightsout_exact_solve": "i ipllpp",
    "dca_idastar_npuzzle": "i ipippplpppipppipp",
    "dca_idastar_npuzzle_reflected": "i ipippplpppipppipp",
    "dca_idastar_npuzzle_batch": "i ipiipppilpppipppipp",
    "dca_idastar_cube3": "i pipppplpppipppipp",
    "dca_idastar_cube3_sym": "i pippppilpppipppipp",
    "dca_idastar_cube3_dual": "i pippppilpppipppipp",
    "dca_idastar_cube3_batch": "i piippppiiplpppipppipp",
    "dca_engine_create": "i piidilii",
    "dca_engine_create_multi": "i piidiliii",
    "dca_engine_num_instances": "i p",
    "dca_engine_destroy": "v p",
    "dca_engine_reset": "i ppp",
    "dca_engine_reset_instance": "i pipp",
    "dca_engine_root_commit": "i ppp",
    "dca_engine_root_commit_instance": "i pipp",
    "dca_engine_root_nnet_in": "i pp",
    "dca_engine_root_nnet_in_instance": "i pip",
    "dca_engine_pop_expand": "i ppppp",
    "dca_engine_commit": "i ppp",
    "dca_engine_enable_packed": "i pil",
    "dca_engine_pop_expand_packed": "i pppppp",
    "dca_engine_commit_packed": "i ppp",
    "dca_engine_packed_state": "i ppp",
    "dca_engine_run_builtin": "i piiip",
    "dca_engine_status": "i ppp",
    "dca_engine_status_instance": "i pipp",
    "dca_engine_set_weight_instance": "i pid",
    "dca_engine_set_weights": "i ppi",
    "dca_engine_park_instance": "i pip",
    "dca_engine_last_popped": "i pppp",
    "dca_engine_reset_many": "i ppip",
    "dca_engine_root_commit_many": "i ppip",
    "dca_engine_set_weights_dev": "i ppip",
    "dca_engine_info": "i ppp",
    "dca_engine_last_children": "i pppp",
    "dca_engine_solution": "i ppippp",
    "dca_engine_solution_instance": "i pipippp",
    "dca_bn_workspace_bytes": "l l",
    "dca_bn_train_forward": "i pppplldippppplp",
    "dca_bn_train_backward": "i ppppppllippppplp",
    "dca_l1_supported": "i ii",
    "dca_l1_kpad": "l ii",
    "dca_l1_onehot_gemm": "i pliipilpipipp",
    "dca_l1_supported8": "i ii",
    "dca_l1_kpad8": "l ii",
    "dca_l1_onehot_gemm8": "i pliiplppipp",
    "dca_l1_embed_supported": "i ii",
    "dca_l1_embed": "i pliiplpipipp",
    "dca_l1_embed_wgrad_slice_rows": "l ii",
    "dca_l1_embed_wgrad_workspace_bytes": "l liil",
    "dca_l1_embed_wgrad": "i pliipllplpplp",
    "dca_act_split": "i ppppdillpppp",
    "dca_f16x3_gemm": "i pplilppilpdppippplpp",
    "dca_gemm16": "i plilpilippiplp",
    "dca_gemm8": "i plilpilpppiplpldp",
    "dca_gemm8_mx": "i pplillpilpppiplplplp",
    "dca_l1_onehot_gemm_mx": "i pliiplpipplp",
    "dca_quant_e4m3": "i pillldplp",
    "dca_split_planes": "i plllpplpp",
    "dca_absmax_bits": "i plllpp",
    "dca_split_planes_scaled": "i plllpppllp",
    "dca_split_rows_scaled": "i plllppllppp",
    "dca_fill_inv_pow2": "i plpp",
    "dca_f16_gemm": "i plilpilpdpplp",
    "dca_cast_planes_scaled": "i plllppllp",
    "dca_cast_rows_scaled": "i plllpllppp",
    "dca_wgrad_splits": "i lii",
    "dca_wgrad_workspace_bytes": "l lii",
    "dca_wgrad_f16": "i pplpplliippiplplp",
    "dca_head_gemv": "i pililppipp",
    "dca_head_gemv64": "i plilppipp",
    "dca_gemm64": "i plilpilppiplp",
    "dca_l1_embed64": "i pliiplpipp",
    # include/dca_debug.h: test / tuning / profiling hooks
    "dca_engine_plan_chunk": "i lipp",
    "dca_engine_known_duplicate": "i iiliii",
    "dca_engine_profile_builtin": "i piiippp",
    "dca_engine_set_tiers": "i pll",
    "dca_engine_debug": "i ppp",
    "dca_debug_tune": "i ii",
    "dca_idastar_host": "i iipipppplpppipppip",
    "dca_idastar_host_reflected": "i ipippplpppipppip",
    "dca_idastar_host_batch": "i ipiipppilpppipppip",
    "dca_pdb_eval_host": "i ipllipppip",
    "dca_idastar_host_sym": "i pippppilpppipppip",
    "dca_cube3_pdb_eval_sym_host": "i plliippppip",
    "dca_idastar_host_dual": "i pippppilpppipppip",
    "dca_idastar_host_cube3_batch": "i piippppiiplpppipppip",
    "dca_cube3_pdb_eval_dual_host": "i plliippppip",
    "dca_cube3_inverse_locs": "i pip",
    "dca_cube3_sym_tables": "i pp",
    "dca_cube3_sym_images": "i ipiipppp",
    "dca_idastar_set_prefix": "i i",
    "dca_debug_write_ceiling": "i pllp",
    "dca_f16x3_gemm_variant": "i i",
    "dca_gemm16_variant": "i i",
}
ABI_SYMBOLS = list(_SIGNATURES)


class DcaError(RuntimeError):
    pass


class DcaStatus(C.Structure):
    _fields_ = [("done", C.c_int32), ("failed", C.c_int32), ("iterations", C.c_int64),
                ("nodes_generated", C.c_int64), ("nodes_expanded", C.c_int64), ("open_size", C.c_int64),
                ("closed_size", C.c_int64), ("pool_size", C.c_int64), ("best_cost", C.c_double)]


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libdca_hip.so; raise loudly if it was never built (python __graft_entry__.py builds it)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DcaError("HIP extension missing: %s — build it with `make -C deepcubea_amd/csrc` "
                           "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        for name, sig in _SIGNATURES.items():
            fn = getattr(_lib, name)  # AttributeError here = stale build of libdca_hip.so
            ret, _, params = sig.partition(" ")
            fn.restype, fn.argtypes = _CTYPE[ret], [_CTYPE[c] for c in params]
        if _lib.dca_abi_version() != 6:
            raise DcaError("libdca_hip.so ABI version mismatch")
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise DcaError("%s failed (rc=%d): %s" % (what or "dca call", rc, lib().dca_last_error().decode()))


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise DcaError("no HIP device visible: the deepcubea_amd hot path runs on an MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device address of a contiguous tensor, as the plain integer a pointer parameter takes; None -> NULL."""
    assert t is None or (t.is_cuda and t.is_contiguous()), "device-resident contiguous tensor required"
    return None if t is None else t.data_ptr()


def _raw(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device address of a tensor that the callee walks with an explicit row stride (views welcome); None -> NULL."""
    assert t is None or t.is_cuda
    return None if t is None else t.data_ptr()


def env_ids(env_name: str):
    """utils/env_utils.py:6-28 registry names -> (env id, dim, state_dim, num_moves, onehot_depth)."""
    import math
    import re
    name = env_name.lower()
    if name == "cube3":
        return ENV_CUBE3, 0, 54, 12, 6
    if name == "cube4":  # environment kernels only (no network / search driver: the reference's harness has none either)
        return ENV_CUBE4, 0, 96, 24, 6
    m = re.search(r"puzzle(\d+)", name)
    if m:
        dim = int(math.sqrt(int(m.group(1)) + 1))
        if 3 <= dim <= 7:
            return ENV_NPUZZLE, dim, dim * dim, 4, dim * dim
    m = re.search(r"lightsout(\d+)", name)
    if m and int(m.group(1)) == 7:
        return ENV_LIGHTSOUT, 7, 49, 49, 6
    raise ValueError("No known environment %s" % env_name)


def env_geometry(env: int, dim: int):
    """(state_dim, num_moves, onehot_depth) of an (env id, dim) pair."""
    if env == ENV_CUBE3:
        return 54, 12, 6
    if env == ENV_CUBE4:
        return 96, 24, 6
    if env == ENV_LIGHTSOUT:
        return dim * dim, dim * dim, 6
    return dim * dim, 4, dim * dim


# ------------------------------------------------------------------------------ tables (host)
def cube3_perm_table() -> np.ndarray:
    return np.ctypeslib.as_array(lib().dca_cube3_perm_table(), (12, 54)).copy()


def cube4_perm_table() -> np.ndarray:
    return np.ctypeslib.as_array(lib().dca_cube4_perm_table(), (24, 96)).copy()


def npuzzle_swap_table(dim: int) -> np.ndarray:
    out = np.zeros((dim * dim, 4), np.uint8)
    check(lib().dca_npuzzle_swap_table(dim, out.ctypes.data_as(C.c_void_p)), "dca_npuzzle_swap_table")
    return out


def engine_known_duplicate(env: int, dim: int, g_parent: int, move_parent: int, action: int, blank: int = 0) -> bool:
    """Does the engine's expansion skip the CLOSED probe for this child (include/dca_debug.h)?  Host only."""
    rc = lib().dca_engine_known_duplicate(env, dim, g_parent, move_parent, action, blank)
    check(min(rc, 0), "dca_engine_known_duplicate")
    return rc == 1


# ------------------------------------------------------------------------------ device ops
def _u8(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.uint8 and t.is_cuda
    return t.contiguous()


def next_state(env: int, dim: int, states: torch.Tensor, action: int, prev: bool = False) -> torch.Tensor:
    states = _u8(states)
    out = torch.empty_like(states)
    n = states.shape[0]
    L = lib()
    if env == ENV_CUBE3:
        fn = L.dca_cube3_prev_state if prev else L.dca_cube3_next_state
        check(fn(ptr(states), n, action, ptr(out), stream_ptr()), "dca_cube3_next_state")
    elif env == ENV_CUBE4:
        fn = L.dca_cube4_prev_state if prev else L.dca_cube4_next_state
        check(fn(ptr(states), n, action, ptr(out), stream_ptr()), "dca_cube4_next_state")
    elif env == ENV_LIGHTSOUT:  # every move is its own inverse (lights_out.py:52-53)
        check(L.dca_lightsout_next_state(ptr(states), n, dim, action, ptr(out), stream_ptr()), "dca_lightsout_next_state")
    else:
        fn = L.dca_npuzzle_prev_state if prev else L.dca_npuzzle_next_state
        check(fn(ptr(states), n, dim, action, ptr(out), stream_ptr()), "dca_npuzzle_next_state")
    return out


def expand_fused(env: int, dim: int, parents: torch.Tensor, *, children: bool = True, nnet_in: bool = False,
                 onehot_dtype: Optional[torch.dtype] = None, solved: bool = True, hashes: bool = True,
                 out: Optional[dict] = None) -> dict:
    """One launch of the fused expansion.  Returns a dict of the requested device tensors.
    `out` may hold preallocated tensors (keys: children, nnet_in, onehot, solved, hash)."""
    parents = _u8(parents)
    n, D = parents.shape
    _, A, depth = env_geometry(env, dim)
    dev = parents.device
    out = dict(out) if out else {}
    if children and "children" not in out:
        out["children"] = torch.empty((n, A, D), dtype=torch.uint8, device=dev)
    if nnet_in and env == ENV_CUBE3 and "nnet_in" not in out:
        out["nnet_in"] = torch.empty((n * A, D), dtype=torch.uint8, device=dev)
    if onehot_dtype is not None and "onehot" not in out:
        out["onehot"] = torch.empty((n * A, D * depth), dtype=onehot_dtype, device=dev)
    if solved and "solved" not in out:
        out["solved"] = torch.empty((n * A,), dtype=torch.uint8, device=dev)
    if hashes and "hash" not in out:
        out["hash"] = torch.empty((n * A,), dtype=torch.int64, device=dev)  # bit pattern of the u64 hash
    oh = out.get("onehot")
    ohdt = _TORCH_DT[oh.dtype] if oh is not None else DT_F32
    L = lib()
    if env == ENV_CUBE4:
        assert oh is None and not nnet_in, "cube4 has no network input in the reference (environment kernels only)"
        check(L.dca_cube4_expand_fused(ptr(parents), n, ptr(out.get("children")), ptr(out.get("solved")), ptr(out.get("hash")),
                                       stream_ptr()), "dca_cube4_expand_fused")
    elif env == ENV_CUBE3:
        check(L.dca_cube3_expand_fused(ptr(parents), n, ptr(out.get("children")), ptr(out.get("nnet_in")), ptr(oh), ohdt,
                                       ptr(out.get("solved")), ptr(out.get("hash")), stream_ptr()), "dca_cube3_expand_fused")
    else:
        fn = L.dca_lightsout_expand_fused if env == ENV_LIGHTSOUT else L.dca_npuzzle_expand_fused
        check(fn(ptr(parents), n, dim, ptr(out.get("children")), ptr(oh), ohdt, ptr(out.get("solved")), ptr(out.get("hash")),
                 stream_ptr()), "dca_npuzzle/lightsout_expand_fused")
        if nnet_in and out.get("children") is not None:
            out["nnet_in"] = out["children"].view(n * A, D)  # n_puzzle.py:84-89: the tiles themselves
    return out


def is_solved(env: int, dim: int, states: torch.Tensor) -> torch.Tensor:
    states = _u8(states)
    out = torch.empty((states.shape[0],), dtype=torch.uint8, device=states.device)
    check(lib().dca_is_solved(env, dim, ptr(states), states.shape[0], ptr(out), stream_ptr()), "dca_is_solved")
    return out


def hash64(states: torch.Tensor) -> torch.Tensor:
    states = _u8(states)
    out = torch.empty((states.shape[0],), dtype=torch.int64, device=states.device)
    check(lib().dca_hash64(ptr(states), states.shape[0], states.shape[1], ptr(out), stream_ptr()), "dca_hash64")
    return out


def nnet_input(env: int, dim: int, states: torch.Tensor) -> torch.Tensor:
    states = _u8(states)
    out = torch.empty_like(states)
    check(lib().dca_nnet_input(env, dim, ptr(states), states.shape[0], ptr(out), stream_ptr()), "dca_nnet_input")
    return out


def onehot(idx: torch.Tensor, depth: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    idx = _u8(idx)
    n, D = idx.shape
    out = torch.empty((n, D * depth), dtype=dtype, device=idx.device)
    check(lib().dca_onehot(ptr(idx), n, D, depth, ptr(out), _TORCH_DT[dtype], stream_ptr()), "dca_onehot")
    return out


def heuristic_builtin(heur_id: int, states: torch.Tensor) -> torch.Tensor:
    states = _u8(states)
    out = torch.empty((states.shape[0],), dtype=torch.float32, device=states.device)
    check(lib().dca_heuristic_builtin(heur_id, ptr(states), states.shape[0], states.shape[1], ptr(out), stream_ptr()),
          "dca_heuristic_builtin")
    return out


def generate_states(env: int, dim: int, n: int, back_lo: int, back_hi: int, seed: int, index0: int = 0,
                    want_moves: bool = False):
    """Device random reverse walks from the goal -> (states [n,D] u8, num_back [n] i32, moves [n,back_hi] i8|None)."""
    dev = require_gpu()
    D = env_geometry(env, dim)[0]
    states = torch.empty((n, D), dtype=torch.uint8, device=dev)
    nb = torch.empty((n,), dtype=torch.int32, device=dev)
    mv = torch.full((n, max(back_hi, 1)), -1, dtype=torch.int8, device=dev) if want_moves else None
    check(lib().dca_generate_states(env, dim, n, back_lo, back_hi, seed & (2**64 - 1), index0, ptr(states), ptr(nb), ptr(mv),
                                    max(back_hi, 1), stream_ptr()), "dca_generate_states")
    return states, nb, mv


def bellman_backup(h_children: torch.Tensor, solved_parent: Optional[torch.Tensor], num_moves: int,
                   clip_zero: bool = True):
    """-> (ctg_backup f32 [n], argmin i32 [n])  (search_utils.py:16-32, gbfs.py:108)."""
    h = h_children.to(torch.float32).contiguous()
    n = h.numel() // num_moves
    ctg = torch.empty((n,), dtype=torch.float32, device=h.device)
    am = torch.empty((n,), dtype=torch.int32, device=h.device)
    check(lib().dca_bellman_backup(ptr(h), ptr(solved_parent), n, num_moves, clip_zero, ptr(ctg), ptr(am), stream_ptr()),
          "dca_bellman_backup")
    return ctg, am


# ------------------------------------------------------------------------------ heuristic cache (update step)
HCACHE_HIT, HCACHE_EVAL_STORE, HCACHE_DUP, HCACHE_EVAL_ONLY = 0, 1, 2, 3


def hcache_bytes(row_bytes: int, slots: int) -> int:
    """Bytes of a heuristic-cache table: a pure function of its arguments (include/dca.h)."""
    b = lib().dca_hcache_bytes(row_bytes, slots)
    check(min(b, 0), "dca_hcache_bytes")
    return b


class HeuristicCache:
    """Owns the device table of dca_hcache_* (include/dca.h "heuristic cache"): rows uint8 [n, row_bytes] -> float32 values,
    exact for a heuristic that is a function of the row alone.  lookup() / finish() are the two halves around the caller's
    evaluation of the EVAL_STORE and EVAL_ONLY rows."""

    def __init__(self, row_bytes: int, slots: int, device: Optional[torch.device] = None):
        row_bytes, slots = int(row_bytes), int(slots)
        if not 1 <= row_bytes <= 64:
            raise ValueError("HeuristicCache: row_bytes must be 1..64, not %d" % row_bytes)
        if slots < 2 or slots > (1 << 30) or slots & (slots - 1):
            raise ValueError("HeuristicCache: slots must be a power of two in 2..2^30, not %d" % slots)
        self.row_bytes, self.slots = row_bytes, slots
        self.nbytes = hcache_bytes(row_bytes, slots)
        dev = device if device is not None else require_gpu()
        self.table = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.clear()

    def clear(self) -> None:
        check(lib().dca_hcache_clear(ptr(self.table), self.row_bytes, self.slots, stream_ptr()), "dca_hcache_clear")

    def used(self) -> int:
        """Slots in use (synchronises)."""
        return int(self.table[:4].view(torch.int32).item())

    def _rows(self, rows: torch.Tensor):
        if rows.dtype != torch.uint8 or not rows.is_cuda or rows.dim() != 2:
            raise ValueError("HeuristicCache: rows must be a uint8 device tensor [n, row_bytes]")
        n, rb = rows.shape
        if rb != self.row_bytes:
            raise ValueError("HeuristicCache: rows are %d bytes wide, the table was built for %d" % (rb, self.row_bytes))
        if n > 0 and rows.stride(1) != 1:
            rows = rows.contiguous()
        ld = rows.stride(0) if n > 1 else max(rows.stride(0), rb)
        if ld < rb:
            rows, ld = rows.contiguous(), rb
        return rows, n, ld

    def lookup(self, rows: torch.Tensor, h: Optional[torch.Tensor] = None, slot: Optional[torch.Tensor] = None,
               status: Optional[torch.Tensor] = None):
        """-> (h f32 [n], slot i32 [n], status u8 [n]); h is written for HIT rows only.  rows may be a strided view (row stride
        >= row_bytes, unit byte stride)."""
        rows, n, ld = self._rows(rows)
        dev = rows.device
        h = torch.empty(n, dtype=torch.float32, device=dev) if h is None else h
        slot = torch.empty(n, dtype=torch.int32, device=dev) if slot is None else slot
        status = torch.empty(n, dtype=torch.uint8, device=dev) if status is None else status
        assert h.dtype == torch.float32 and slot.dtype == torch.int32 and status.dtype == torch.uint8
        assert h.numel() >= n and slot.numel() >= n and status.numel() >= n
        check(lib().dca_hcache_lookup(ptr(self.table), self.row_bytes, self.slots, _raw(rows), n, ld, ptr(h), ptr(slot), ptr(status),
                                      stream_ptr()), "dca_hcache_lookup")
        return h, slot, status

    def finish(self, h: torch.Tensor, slot: torch.Tensor, status: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
        n = int(status.numel() if n is None else n)
        check(lib().dca_hcache_finish(ptr(self.table), self.row_bytes, self.slots, n, ptr(slot), ptr(status), ptr(h), stream_ptr()),
              "dca_hcache_finish")
        return h


# ------------------------------------------------------------------------------ pattern databases (sliding puzzles)
PDB_MAX_PATTERNS = 24
PDB_NO_STATE, PDB_UNREACHABLE = 0xFF, 0xFE  # table bytes: two digits equal / a state the goal cannot be reached from


def _pdb_rows(states: torch.Tensor, width: int, who: str):
    """The rows a pattern-database eval walks -> (states with unit byte stride, n, row stride ld)."""
    if states.dtype != torch.uint8 or not states.is_cuda or states.dim() != 2:
        raise ValueError("%s: states must be a uint8 device tensor [n, >= %d]" % (who, width))
    n = states.shape[0]
    if n > 0 and states.stride(1) != 1:
        states = states.contiguous()
    ld = states.stride(0) if n > 1 else max(states.stride(0), states.shape[1])
    if ld < states.shape[1]:
        states, ld = states.contiguous(), states.shape[1]
    if states.shape[1] < width:
        ld = states.shape[1]  # too narrow a row: the library refuses ld < width
    return states, n, ld


def _byte_list(values) -> np.ndarray:
    """Small non-negative integers as the uint8 array an entry point reads; ValueError (not a wrapped value) outside a byte."""
    a = np.ascontiguousarray(list(values), dtype=np.int64)
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("values outside 0..255: %s" % (a.tolist(),))
    return a.astype(np.uint8)


def _pdb_build(symbol: str, bytes_fn, family: int, ids, table: Optional[torch.Tensor]):
    """One pattern's build through `symbol`(family, ids, k, table, sweeps, stream) -> (table, sweeps)."""
    ids = _byte_list(ids)
    nbytes = bytes_fn(family, len(ids))
    if table is None:
        table = torch.empty(nbytes, dtype=torch.uint8, device=require_gpu())
    assert table.dtype == torch.uint8 and table.numel() == nbytes
    sweeps = C.c_int(0)
    check(getattr(lib(), symbol)(family, ids.ctypes.data_as(C.c_void_p), len(ids), ptr(table), C.byref(sweeps), stream_ptr()), symbol)
    return table, int(sweeps.value)


@functools.lru_cache(maxsize=64)
def _pdb_set(groups, families, size_of):
    """What an eval marshals from its pattern set, kept per set (the engine's closure evaluates one set every iteration, and the
    library only reads these arrays) -> (pointers to families i32, ids u8, ks i32; each pattern's table bytes; the arrays, kept
    alive).  groups: the patterns' id tuples; families: per pattern the dim or the kind; size_of(family, k): the table's bytes by
    arithmetic, no library call — None outside the library's limits, where the library words the refusal."""
    arrays = (np.ascontiguousarray(families, dtype=np.int32), _byte_list([i for g in groups for i in g]),
              np.ascontiguousarray([len(g) for g in groups], dtype=np.int32))
    return (tuple(a.ctypes.data_as(C.c_void_p) for a in arrays), tuple(size_of(f, len(g)) for f, g in zip(families, groups)), arrays)


def _pdb_eval(who: str, symbol: str, states: torch.Tensor, width: int, groups, families, size_of, tables, out: Optional[torch.Tensor],
              call):
    """What the evals share; call(states, n, ld, num_patterns, families, ids, ks, tables, out, stream) makes the family's call."""
    states, n, ld = _pdb_rows(states, width, who)
    pointers, sizes, _ = _pdb_set(tuple(tuple(g) for g in groups), tuple(families), size_of)
    if len(tables) != len(groups):
        raise ValueError("%s: %d tables for %d patterns" % (who, len(tables), len(groups)))
    for size, t in zip(sizes, tables):  # the library cannot see a table's size: a short one would be read past its end
        if size is not None and (t.dtype != torch.uint8 or t.numel() != size):
            raise ValueError("%s: a table of %d elements for a pattern that needs %d bytes" % (who, t.numel(), size))
    ptrs = (C.c_void_p * max(len(tables), 1))(*[ptr(t) for t in tables])
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=states.device)
    assert out.dtype == torch.float32 and out.numel() >= n
    check(call(_raw(states), n, ld, len(groups), *pointers, ptrs, ptr(out), stream_ptr()), symbol)
    return out


def pdb_bytes(dim: int, k: int) -> int:
    """Bytes of one pattern's table, N^(k+1) with N = dim * dim: a pure function (include/dca.h); DcaError outside its limits."""
    b = lib().dca_pdb_bytes(dim, k)
    check(min(b, 0), "dca_pdb_bytes")
    return b


def _pdb_table_bytes(dim: int, k: int) -> Optional[int]:
    return (dim * dim) ** (k + 1) if 3 <= dim <= 7 and 1 <= k <= dim * dim - 1 else None


def pdb_build(dim: int, tiles, table: Optional[torch.Tensor] = None):
    """Fill (or allocate and fill) the device table of the pattern `tiles` -> (table u8 [N^(k+1)], sweeps).  Synchronises."""
    return _pdb_build("dca_pdb_build", pdb_bytes, dim, tiles, table)


def pdb_eval(dim: int, states: torch.Tensor, partition, tables, out: Optional[torch.Tensor] = None, reflect: bool = False) -> torch.Tensor:
    """Sum of the patterns' table bytes per row -> f32 [n].  states: uint8 device rows [n, >= dim * dim] with unit byte stride
    (a strided view is fine); ANY bytes are in bounds (include/dca.h, the any-bytes rule).  reflect: the larger of that sum and
    the sum at the row's mirror image (include/dca.h, "Reflected look-up")."""
    symbol = "dca_pdb_eval_reflected" if reflect else "dca_pdb_eval"
    return _pdb_eval("pdb_eval", symbol, states, dim * dim, partition, (dim,) * len(partition), _pdb_table_bytes, tables, out,
                     lambda s, n, ld, m, dims, *rest: getattr(lib(), symbol)(dim, s, n, ld, m, *rest))


def pdb_eval_host(dim: int, rows, partition, tables, reflect: bool = False) -> np.ndarray:
    """pdb_eval on the CPU (include/dca_debug.h: the kernels' own row value in a plain loop) -> float32 [n].  rows: a uint8 host
    array [n, >= dim * dim]; tables: one uint8 host array per pattern.  No device needed."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2:
        raise ValueError("pdb_eval_host: rows must be a uint8 host array [n, >= %d]" % (dim * dim))
    rows = np.ascontiguousarray(rows)
    _table_sizes("pdb_eval_host", [_pdb_table_bytes(dim, len(g)) for g in partition], tables, True)
    (_, ids, ks), ptrs, _keep = _idastar_set(partition, (dim,) * len(partition), tables, True)
    out = np.zeros(len(rows), np.float32)
    check(lib().dca_pdb_eval_host(dim, rows.ctypes.data_as(C.c_void_p), len(rows), rows.shape[1], len(partition), ids, ks, ptrs,
                                  int(bool(reflect)), out.ctypes.data_as(C.c_void_p)), "dca_pdb_eval_host")
    return out


# ------------------------------------------------------------------------------ pattern databases (cube3)
CUBE3_CORNERS, CUBE3_EDGES = 0, 1
ROWS_STATE, ROWS_NNET = 0, 1  # what a row's 54 bytes are: sticker ids 0..53 / colour bytes 0..5 (the network input)
CUBE3_PDB_SLOTS = {CUBE3_CORNERS: (8, 3), CUBE3_EDGES: (12, 2)}  # kind -> (slots n, orientations o)


def cube3_pdb_bytes(kind: int, k: int) -> int:
    """Bytes of one pattern's table, P(n, k) * o^k: a pure function (include/dca.h); DcaError outside its limits."""
    b = lib().dca_cube3_pdb_bytes(kind, k)
    check(min(b, 0), "dca_cube3_pdb_bytes")
    return b


def _cube3_table_bytes(kind: int, k: int) -> Optional[int]:
    if kind not in CUBE3_PDB_SLOTS or not 1 <= k <= 8:
        return None
    n, o = CUBE3_PDB_SLOTS[kind]
    return math.perm(n, k) * o ** k


def cube3_pdb_cubies(kind: int) -> np.ndarray:
    """The cubie lists as the library numbers them -> uint8 [n, o] sticker positions."""
    if kind not in CUBE3_PDB_SLOTS:
        raise ValueError("kind is CUBE3_CORNERS (0) or CUBE3_EDGES (1), not %r" % (kind,))
    n, o = CUBE3_PDB_SLOTS[kind]
    out = np.zeros(n * o, np.uint8)
    check(lib().dca_cube3_pdb_cubies(kind, out.ctypes.data_as(C.c_void_p)), "dca_cube3_pdb_cubies")
    return out.reshape(n, o)


def cube3_pdb_index(kind: int, cubies, rows: np.ndarray, row_kind: int) -> np.ndarray:
    """Table index of host rows [m, 54] (or one row [54]) by the code the kernels run -> int64 [m].  No device needed."""
    cubies = _byte_list(cubies)
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 54)
    out = np.zeros(len(rows), np.int64)
    fn, one = lib().dca_cube3_pdb_index, C.c_int64(0)
    cp = cubies.ctypes.data_as(C.c_void_p)
    for i in range(len(rows)):
        check(fn(kind, cp, len(cubies), rows[i].ctypes.data_as(C.c_void_p), row_kind, C.byref(one)), "dca_cube3_pdb_index")
        out[i] = one.value
    return out


def cube3_pdb_build(kind: int, cubies, table: Optional[torch.Tensor] = None):
    """Fill (or allocate and fill) the device table of one pattern -> (table u8 [P(n,k) * o^k], sweeps).  Synchronises."""
    return _pdb_build("dca_cube3_pdb_build", cube3_pdb_bytes, kind, cubies, table)


def cube3_pdb_eval(states: torch.Tensor, row_kind: int, patterns, tables, out: Optional[torch.Tensor] = None, sym: int = 0,
                   dual: bool = False) -> torch.Tensor:
    """Max of the patterns' table bytes per row -> f32 [n].  patterns: [(kind, cubies), ...]; states: uint8 device rows
    [n, >= 54] with unit byte stride (a strided view is fine); ANY bytes are in bounds (include/dca.h, the any-bytes rule).
    sym = N in 1..48: the max over the first N images of every pattern as well (include/dca.h, "Symmetric look-ups"); 0: plain.
    dual: the larger of that value at the row and at its inverse (include/dca.h, "Dual look-ups"); without sym, of the plain value."""
    groups, kinds = [g for _, g in patterns], [kind for kind, _ in patterns]
    infix, images = _cube3_mode(sym, dual)
    symbol = "dca_cube3_pdb_eval" + infix
    return _pdb_eval("cube3_pdb_eval", symbol, states, 54, groups, kinds, _cube3_table_bytes, tables, out,
                     lambda s, n, ld, m, k, c, ks, t, *rest: getattr(lib(), symbol)(s, n, ld, row_kind, m, k, c, ks, t, *images, *rest))


CUBE3_SYMS, CUBE3_SYM_MAX_LOOKUPS = 48, 64  # include/dca.h


def _cube3_mode(sym: int, dual: bool):
    """A cube3 look-up mode's entry points -> (their symbols' infix, the max_images argument they take behind `tables`): plain,
    the first `sym` images of every pattern, or the dual look-ups (on the patterns alone without sym)."""
    if dual:
        return "_dual", (int(sym or 1),)
    return ("_sym", (int(sym),)) if sym else ("", ())


def cube3_pdb_eval_host(rows, row_kind: int, patterns, tables, sym: int = 1, dual: bool = False) -> np.ndarray:
    """cube3_pdb_eval(sym=..., dual=...) on the CPU (include/dca_debug.h: the kernel's own row value in a plain loop) -> float32 [n].
    rows: a uint8 host array [n, >= 54]; tables: one uint8 host array per pattern.  sym = 1 is the plain value.  No device needed."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2:
        raise ValueError("cube3_pdb_eval_host: rows must be a uint8 host array [n, >= 54]")
    rows = np.ascontiguousarray(rows)
    _table_sizes("cube3_pdb_eval_host", [_cube3_table_bytes(kind, len(g)) for kind, g in patterns], tables, True)
    (kinds, ids, ks), ptrs, _keep = _idastar_set([g for _, g in patterns], [kind for kind, _ in patterns], tables, True)
    out = np.zeros(len(rows), np.float32)
    infix, _ = _cube3_mode(sym or 1, dual)  # (no plain host eval: sym = 1 is that value, and the library words sym = 0's refusal)
    symbol = "dca_cube3_pdb_eval%s_host" % infix
    check(getattr(lib(), symbol)(rows.ctypes.data_as(C.c_void_p), len(rows), rows.shape[1], row_kind, len(patterns), kinds, ids,
                                 ks, ptrs, int(sym), out.ctypes.data_as(C.c_void_p)), symbol)
    return out


def cube3_inverse_locs(rows, row_kind: int) -> np.ndarray:
    """The location words of the inverse of each row by the inversion rule (include/dca.h, "Dual look-ups"; the replacing form) ->
    uint64 [n, 2]: the corner word and the edge word, 5 bits a cubie.  rows: uint8 host [n, >= 54], any bytes.  No device needed."""
    rows = np.ascontiguousarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] < 54:
        raise ValueError("cube3_inverse_locs: rows must be a uint8 host array [n, >= 54]")
    out = np.zeros((len(rows), 2), np.uint64)
    for i in range(len(rows)):
        check(lib().dca_cube3_inverse_locs(rows[i].ctypes.data_as(C.c_void_p), row_kind, out[i].ctypes.data_as(C.c_void_p)), "dca_cube3_inverse_locs")
    return out


def cube3_sym_tables():
    """The 48 symmetries as the library derives them, in include/dca.h's order -> (sticker permutations uint8 [48, 54], position
    -> position; move maps uint8 [48, 12]).  No device needed."""
    sticker, move = np.zeros((CUBE3_SYMS, 54), np.uint8), np.zeros((CUBE3_SYMS, 12), np.uint8)
    check(lib().dca_cube3_sym_tables(sticker.ctypes.data_as(C.c_void_p), move.ctypes.data_as(C.c_void_p)), "dca_cube3_sym_tables")
    return sticker, move


def cube3_sym_images(kind: int, cubies, max_images: int = CUBE3_SYMS):
    """The first min(max_images, distinct) images of one pattern -> (the symmetry standing for each uint8 [m], their source cubies
    uint8 [m, k], their location maps uint8 [m, k, 24]).  No device needed."""
    cubies = _byte_list(cubies)
    k, count = len(cubies), C.c_int(0)
    syms, src, maps = np.zeros(CUBE3_SYMS, np.uint8), np.zeros((CUBE3_SYMS, 8), np.uint8), np.zeros((CUBE3_SYMS, 8, 24), np.uint8)
    check(lib().dca_cube3_sym_images(kind, cubies.ctypes.data_as(C.c_void_p), k, int(max_images), C.byref(count),
                                     *(a.ctypes.data_as(C.c_void_p) for a in (syms, src, maps))), "dca_cube3_sym_images")
    m = count.value
    return syms[:m].copy(), src[:m, :k].copy(), maps[:m, :k].copy()


# ------------------------------------------------------------------------------ exact LightsOut heuristic (lightsout7)
LIGHTSOUT_EXACT_DIM = 7  # the one board size the library instantiates (its press matrix is invertible over GF(2))


def lightsout_exact_matrix() -> np.ndarray:
    """A^-1 over GF(2) as the kernels use it -> uint64 [49]: row a, bit i for cell i (include/dca.h).  No device needed."""
    out = np.zeros(LIGHTSOUT_EXACT_DIM ** 2, np.uint64)
    check(lib().dca_lightsout_exact_matrix(LIGHTSOUT_EXACT_DIM, out.ctypes.data_as(C.c_void_p)), "dca_lightsout_exact_matrix")
    return out


def _lightsout_exact(who: str, symbol: str, states: torch.Tensor, out: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    states, n, ld = _pdb_rows(states, LIGHTSOUT_EXACT_DIM ** 2, who)
    if out is None:
        out = torch.empty(n, dtype=dtype, device=states.device)
    assert out.dtype == dtype and out.is_cuda and out.numel() >= n
    check(getattr(lib(), symbol)(LIGHTSOUT_EXACT_DIM, _raw(states), n, ld, ptr(out), stream_ptr()), symbol)
    return out


def lightsout_exact_eval(states: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The exact distance popcount(A^-1 row) per row -> f32 [n].  states: uint8 device rows [n, >= 49] with unit byte stride (a
    strided view is fine); a cell is bit 0 of its byte, so ANY bytes are in bounds (include/dca.h, the bit-0 rule)."""
    return _lightsout_exact("lightsout_exact_eval", "dca_lightsout_exact_eval", states, out, torch.float32)


def lightsout_exact_solve(states: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The optimal solution per row as a 64-bit mask -> int64 [n]: bit a set iff cell a is pressed.  states as for the eval."""
    return _lightsout_exact("lightsout_exact_solve", "dca_lightsout_exact_solve", states, out, torch.int64)


# ------------------------------------------------------------------------------ IDA* on the pattern databases
IDASTAR_SOLVED, IDASTAR_BUDGET, IDASTAR_UNSOLVABLE, IDASTAR_BOUNDED = 0, 1, 2, 3
IDASTAR_STATUS = {IDASTAR_SOLVED: "solved", IDASTAR_BUDGET: "budget exhausted", IDASTAR_UNSOLVABLE: "unsolvable",
                  IDASTAR_BOUNDED: "bounded"}  # bounded: no solution within the root's max_length (the bounded batches alone)
IDASTAR_POLL_NODES, IDASTAR_MAX_LANES, IDASTAR_MAX_MOVES = 512, 1 << 19, 254  # include/dca.h
IDASTAR_OVERSHOOT = IDASTAR_MAX_LANES * IDASTAR_POLL_NODES  # total_nodes <= max_nodes + this, whatever the launch
IDASTAR_MAX_PREFIX = {ENV_NPUZZLE: 15, ENV_CUBE3: 6}  # moves a work item's prefix has at the most
IDASTAR_MAX_PUZZLE_PATTERNS = 8
IDASTAR_MAX_REFLECT_PATTERNS = 4  # a running index and a reflected one per pattern share the 8 a lane keeps
IDASTAR_MAX_BATCH = 1024  # DCA_IDASTAR_MAX_BATCH: roots of one dca_idastar_npuzzle_batch or dca_idastar_cube3_batch call


def _idastar(symbol: str, call, root, width: int, max_nodes: int) -> dict:
    """What the three searches share: the root's bytes, the output buffers, and the result as a dict shaped like the engine's
    (solved, moves, path_cost, nodes_generated) plus status, thresholds and nodes_per_threshold.  call(root, max_nodes, *outputs)
    makes the entry point's call."""
    root = np.ascontiguousarray(root, dtype=np.uint8).reshape(-1)
    if root.size != width:
        raise ValueError("%s: a root of %d bytes, not %d" % (symbol, root.size, width))
    cap = IDASTAR_MAX_MOVES + 2
    status, length, count, total = C.c_int(-1), C.c_int(0), C.c_int(0), C.c_int64(0)
    moves, thresholds, per = np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int64)

    def as_p(a):
        return a.ctypes.data_as(C.c_void_p)
    check(call(as_p(root), int(max_nodes), C.byref(status), C.byref(length), as_p(moves), cap, C.byref(count), as_p(thresholds),
               as_p(per), cap, C.byref(total)), symbol)
    n = min(count.value, cap)
    solved = status.value == IDASTAR_SOLVED
    return {"solved": solved, "status": IDASTAR_STATUS[status.value], "moves": [int(m) for m in moves[:length.value]] if solved else [],
            "path_cost": float(length.value) if solved else float("inf"), "nodes_generated": int(total.value),
            "thresholds": [int(t) for t in thresholds[:n]], "nodes_per_threshold": [int(c) for c in per[:n]]}


def _idastar_batch(symbol: str, call, roots, width: int, max_nodes: int) -> list:
    """_idastar for a batch: the roots' bytes [n, width], the output arrays, and one dict per root.  call(roots, n, max_nodes,
    *outputs) makes the entry point's call."""
    roots = np.ascontiguousarray(roots, dtype=np.uint8)
    if roots.ndim != 2 or roots.shape[1] != width:
        raise ValueError("%s: roots of shape %s, not [n, %d]" % (symbol, tuple(roots.shape), width))
    n, cap = len(roots), IDASTAR_MAX_MOVES + 2
    status, length, count = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    total, moves = np.zeros(n, np.int64), np.zeros((n, cap), np.uint8)
    thresholds, per = np.zeros((n, cap), np.int32), np.zeros((n, cap), np.int64)

    def as_p(a):
        return a.ctypes.data_as(C.c_void_p)
    check(call(as_p(roots), n, int(max_nodes), as_p(status), as_p(length), as_p(moves), cap, as_p(count), as_p(thresholds), as_p(per), cap,
               as_p(total)), symbol)
    out = []
    for r in range(n):
        k, solved = min(int(count[r]), cap), int(status[r]) == IDASTAR_SOLVED
        out.append({"solved": solved, "status": IDASTAR_STATUS[int(status[r])],
                    "moves": [int(m) for m in moves[r, :length[r]]] if solved else [],
                    "path_cost": float(length[r]) if solved else float("inf"), "nodes_generated": int(total[r]),
                    "thresholds": [int(t) for t in thresholds[r, :k]], "nodes_per_threshold": [int(c) for c in per[r, :k]]})
    return out


def _no_size(family: int, k: int) -> None:
    return None


def _idastar_set(groups, families, tables, host: bool):
    """The pattern set's marshalled arrays (as the evals build them) and the HOST array of table pointers."""
    pointers, _, keep = _pdb_set(tuple(tuple(g) for g in groups), tuple(families), _no_size)
    if len(tables) != len(groups):
        raise ValueError("%d tables for %d patterns" % (len(tables), len(groups)))
    if host:
        keep = (keep, [np.ascontiguousarray(t, dtype=np.uint8).reshape(-1) for t in tables])
        addresses = [t.ctypes.data for t in keep[1]]
    else:
        addresses = [ptr(t) for t in tables]
    return pointers, (C.c_void_p * max(len(tables), 1))(*addresses), keep


def _table_sizes(who: str, sizes, tables, host: bool) -> None:
    """The library sees a table as an address: a short one would be read past its end, and a host address handed to the kernel
    (or a device address to the host search) is a fault.  So uint8 device tensors for the device searches, uint8 host arrays for
    the host search, each of its pattern's size where that is defined (the library refuses the pattern otherwise)."""
    for i, (size, t) in enumerate(zip(sizes, tables)):
        if host:
            if isinstance(t, torch.Tensor) or np.asarray(t).dtype != np.uint8:
                raise ValueError("%s: table %d is not a uint8 host array" % (who, i))
            n = int(np.asarray(t).size)
        else:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError("%s: table %d is not a contiguous uint8 device tensor" % (who, i))
            n = int(t.numel())
        if size is not None and n != size:
            raise ValueError("%s: a table of %d elements for a pattern that needs %d bytes" % (who, n, size))


def idastar_npuzzle(dim: int, root, partition, tables, max_nodes: int, reflect: bool = False) -> dict:
    """Optimal solution of one sliding-puzzle root by IDA* on the device tables of `partition` (include/dca.h "IDA*") -> dict.
    Synchronises once per threshold.  reflect: h is the reflected value; at most IDASTAR_MAX_REFLECT_PATTERNS patterns."""
    _table_sizes("idastar_npuzzle", [_pdb_table_bytes(dim, len(g)) for g in partition], tables, False)
    (_, ids, ks), ptrs, _keep = _idastar_set(partition, (dim,) * len(partition), tables, False)
    symbol = "dca_idastar_npuzzle_reflected" if reflect else "dca_idastar_npuzzle"
    return _idastar(symbol, lambda r, n, *out: getattr(lib(), symbol)(dim, r, len(partition), ids, ks, ptrs, n, *out, stream_ptr()),
                    root, max(dim, 0) ** 2, max_nodes)


def idastar_npuzzle_batch(dim: int, roots, partition, tables, max_nodes: int, reflect: bool = False) -> list:
    """A batch of sliding-puzzle roots [n, dim * dim], n in 1..IDASTAR_MAX_BATCH, searched in rounds of one launch each
    (include/dca.h "batch") -> one dict per root, each what idastar_npuzzle gives for that root alone; max_nodes is per root.
    Synchronises once per round.  A bad root refuses the whole batch: DcaError, "roots[i]: ..."."""
    _table_sizes("idastar_npuzzle_batch", [_pdb_table_bytes(dim, len(g)) for g in partition], tables, False)
    (_, ids, ks), ptrs, _keep = _idastar_set(partition, (dim,) * len(partition), tables, False)
    return _idastar_batch("dca_idastar_npuzzle_batch", lambda r, n, m, *out: lib().dca_idastar_npuzzle_batch(
        dim, r, n, len(partition), ids, ks, ptrs, int(bool(reflect)), m, *out, stream_ptr()), roots, max(dim, 0) ** 2, max_nodes)


def idastar_host_batch(dim: int, roots, partition, tables, max_nodes: int, reflect: bool = False) -> list:
    """idastar_npuzzle_batch run on the CPU from HOST tables (include/dca_debug.h): no device needed."""
    _table_sizes("idastar_host_batch", [_pdb_table_bytes(dim, len(g)) for g in partition], tables, True)
    (_, ids, ks), ptrs, _keep = _idastar_set(partition, (dim,) * len(partition), tables, True)
    return _idastar_batch("dca_idastar_host_batch", lambda r, n, m, *out: lib().dca_idastar_host_batch(
        dim, r, n, len(partition), ids, ks, ptrs, int(bool(reflect)), m, *out), roots, max(dim, 0) ** 2, max_nodes)


def idastar_cube3(root, patterns, tables, max_nodes: int, sym: int = 0, dual: bool = False) -> dict:
    """Optimal solution of one cube3 root (54 sticker ids) by IDA* on the device tables of `patterns` [(kind, cubies), ...].
    sym = N in 1..48: h is the max over the first N images of every pattern (include/dca.h, "Symmetric look-ups"); 0: plain.
    dual: h is the larger of that value at the state and at its inverse (include/dca.h, "Dual look-ups")."""
    _table_sizes("idastar_cube3", [_cube3_table_bytes(kind, len(g)) for kind, g in patterns], tables, False)
    (kinds, ids, ks), ptrs, _keep = _idastar_set([g for _, g in patterns], [kind for kind, _ in patterns], tables, False)
    infix, images = _cube3_mode(sym, dual)
    symbol = "dca_idastar_cube3" + infix
    return _idastar(symbol, lambda r, n, *out: getattr(lib(), symbol)(r, len(patterns), kinds, ids, ks, ptrs, *images, n, *out, stream_ptr()),
                    root, 54, max_nodes)


def _max_length(max_length, n: int):
    """A bounded batch's max_length argument -> (the int32 array kept alive or None, its pointer or None)."""
    if max_length is None:
        return None, None
    bound = np.ascontiguousarray(np.broadcast_to(np.asarray(max_length, dtype=np.int32), (n,)))
    return bound, bound.ctypes.data_as(C.c_void_p)


def _idastar_cube3_batch(symbol: str, host: bool, roots, patterns, tables, max_length, max_nodes: int, sym: int, dual: bool) -> list:
    _table_sizes(symbol, [_cube3_table_bytes(kind, len(g)) for kind, g in patterns], tables, host)
    (kinds, ids, ks), ptrs, _keep = _idastar_set([g for _, g in patterns], [kind for kind, _ in patterns], tables, host)
    images = _cube3_mode(sym, dual)[1] or (0,)
    _bound, bound = _max_length(max_length, len(roots))
    stream = () if host else (stream_ptr(),)
    return _idastar_batch(symbol, lambda r, n, m, *out: getattr(lib(), symbol)(
        r, n, len(patterns), kinds, ids, ks, ptrs, *images, int(bool(dual)), bound, m, *out, *stream), roots, 54, max_nodes)


def idastar_cube3_batch(roots, patterns, tables, max_nodes: int, max_length=None, sym: int = 0, dual: bool = False) -> list:
    """A bounded batch of cube3 roots [n, 54], n in 1..IDASTAR_MAX_BATCH, searched in rounds of one launch each (include/dca.h
    "Bounded batches") -> one dict per root, each what idastar_cube3 gives for that root alone, except that a root with no
    solution of at most max_length[r] moves (an int for all roots, one per root, or None: no bound) ends with status "bounded".
    For shallow roots; max_nodes is per root.  A bad root refuses the whole batch: DcaError, "roots[i]: ..."."""
    return _idastar_cube3_batch("dca_idastar_cube3_batch", False, roots, patterns, tables, max_length, max_nodes, sym, dual)


def idastar_host_cube3_batch(roots, patterns, tables, max_nodes: int, max_length=None, sym: int = 0, dual: bool = False) -> list:
    """idastar_cube3_batch run on the CPU from HOST tables (include/dca_debug.h): no device needed."""
    return _idastar_cube3_batch("dca_idastar_host_cube3_batch", True, roots, patterns, tables, max_length, max_nodes, sym, dual)


def idastar_host(env: int, dim: int, root, patterns, tables, max_nodes: int, reflect: bool = False, sym: int = 0,
                 dual: bool = False) -> dict:
    """The same search run sequentially on the CPU from HOST tables (include/dca_debug.h): no device needed.  patterns: the
    partition (puzzles) or [(kind, cubies), ...] (cube3); tables: one uint8 array per pattern.  reflect: the reflected search,
    sliding puzzles only.  sym = N: the search on the symmetric look-ups, dual: on the dual look-ups, cube3 only."""
    if reflect and env != ENV_NPUZZLE:
        raise ValueError("idastar_host: the reflected look-up is defined for the sliding puzzles only")
    if sym and env != ENV_CUBE3:
        raise ValueError("idastar_host: the symmetric look-ups are defined for cube3 only")
    if dual and env != ENV_CUBE3:
        raise ValueError("idastar_host: the dual look-ups are defined for cube3 only")
    if env == ENV_CUBE3:
        groups, families = [g for _, g in patterns], [kind for kind, _ in patterns]
        sizes, width = [_cube3_table_bytes(kind, len(g)) for kind, g in patterns], 54
    else:
        groups, families = list(patterns), [dim] * len(patterns)
        sizes, width = [_pdb_table_bytes(dim, len(g)) for g in patterns], max(dim, 0) ** 2
    _table_sizes("idastar_host", sizes, tables, True)
    (kinds, ids, ks), ptrs, _keep = _idastar_set(groups, families, tables, True)
    infix, images = _cube3_mode(sym, dual)
    if infix:
        symbol = "dca_idastar_host" + infix
        return _idastar(symbol, lambda r, n, *out: getattr(lib(), symbol)(r, len(groups), kinds, ids, ks, ptrs, *images, n, *out),
                        root, width, max_nodes)
    if reflect:
        return _idastar("dca_idastar_host_reflected", lambda r, n, *out: lib().dca_idastar_host_reflected(dim, r, len(groups), ids, ks, ptrs,
                                                                                                          n, *out), root, width, max_nodes)
    return _idastar("dca_idastar_host", lambda r, n, *out: lib().dca_idastar_host(env, dim, r, len(groups), kinds, ids, ks, ptrs, n, *out),
                    root, width, max_nodes)


def idastar_set_prefix(depth: int) -> None:
    """Test hook: the prefix depth of every work item (-1 = chosen from the previous iteration's node count)."""
    check(lib().dca_idastar_set_prefix(depth), "dca_idastar_set_prefix")


# ------------------------------------------------------------------------------ training step
class _BnTrainFn(torch.autograd.Function):
    """BatchNorm1d (training statistics) [+ skip] [+ ReLU] through dca_bn_train_forward / backward."""

    @staticmethod
    def forward(ctx, x, skip, gamma, beta, eps, relu, stats_out):
        x = x.contiguous()
        n, c = x.shape
        ws = torch.empty(lib().dca_bn_workspace_bytes(c), dtype=torch.uint8, device=x.device)
        y = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        var_u = torch.empty_like(mean)
        sk = skip.contiguous() if skip is not None else None
        check(lib().dca_bn_train_forward(ptr(x), ptr(sk), ptr(gamma.contiguous()), ptr(beta.contiguous()), n, c, eps, relu, ptr(y),
                                         ptr(mean), ptr(invstd), ptr(var_u), ptr(ws), ws.numel(), stream_ptr()), "dca_bn_train_forward")
        stats_out.append((mean, var_u))
        ctx.save_for_backward(x, y, mean, invstd, gamma)
        ctx.relu, ctx.has_skip = bool(relu), skip is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, invstd, gamma = ctx.saved_tensors
        n, c = x.shape
        dy = dy.contiguous()
        ws = torch.empty(lib().dca_bn_workspace_bytes(c), dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(x)
        dskip = torch.empty_like(x) if ctx.has_skip else None
        dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
        dbeta = torch.empty_like(dgamma)
        check(lib().dca_bn_train_backward(ptr(dy), ptr(x), ptr(y), ptr(mean), ptr(invstd), ptr(gamma.contiguous()), n, c, ctx.relu,
                                          ptr(dx), ptr(dskip), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream_ptr()),
              "dca_bn_train_backward")
        return dx, dskip, dgamma, dbeta, None, None, None


def bn_train(x: torch.Tensor, bn: "torch.nn.BatchNorm1d", relu: bool, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Training-mode `relu?(bn(x) (+ skip))` on the device, updating bn.running_mean / running_var /
    num_batches_tracked exactly like nn.BatchNorm1d (momentum average, unbiased variance)."""
    if x.shape[0] == 1:  # one sample has no batch variance: nn.BatchNorm1d refuses it in training mode, with these words
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (torch.Size(x.shape),))
    stats = []
    y = _BnTrainFn.apply(x, skip, bn.weight, bn.bias, float(bn.eps), bool(relu), stats)
    if bn.track_running_stats and bn.running_mean is not None:
        mean, var_u = stats[0]
        with torch.no_grad():
            bn.num_batches_tracked += 1
            mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1.0 - mom).add_(mean, alpha=mom)
            bn.running_var.mul_(1.0 - mom).add_(var_u, alpha=mom)
    return y


# ------------------------------------------------------------------------------ training step: dense layers
def _pad64(k: int) -> int:
    return (k + 63) // 64 * 64


def _rows_cols_ld(x: torch.Tensor, m, n, ld):
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    return (int(x.shape[0]) if m is None else int(m), int(x.shape[1]) if n is None else int(n),
            int(x.stride(0)) if ld is None else int(ld))


def absmax_bits(x: torch.Tensor, m: Optional[int] = None, n: Optional[int] = None, ld: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max |x| of an fp32 matrix as float bits in a device int32 word (dca_absmax_bits; the word is zeroed by the call).
    x: rows of unit column stride — a column slice of a wider matrix is fine; m / n / ld (row stride in elements) default to
    x's own shape and stride."""
    m, n, ld = _rows_cols_ld(x, m, n, ld)
    if out is None:
        out = torch.empty(1, dtype=torch.int32, device=x.device)
    check(lib().dca_absmax_bits(_raw(x), m, n, ld, _raw(out), stream_ptr()), "dca_absmax_bits")
    return out


def _plane_ptrs(out: torch.Tensor):
    """Device addresses of the planes of a contiguous fp16 [planes, rows, ld] tensor (no view per plane: this runs per launch)."""
    base = _raw(out)
    return [base + p * out.shape[1] * out.shape[2] * 2 for p in range(out.shape[0])]


def _planes_scaled(planes: int, x, amax, n_pad, ldo, out, m, n, ld) -> torch.Tensor:
    """split_planes_scaled (planes = 2) and cast_planes_scaled (1): the defaults, the [planes, m, ldo] buffer, the call."""
    m, n, ld = _rows_cols_ld(x, m, n, ld)
    n_pad = n if n_pad is None else int(n_pad)
    ldo = n_pad if ldo is None else int(ldo)
    if out is None:
        out = torch.empty((planes, m, ldo), dtype=torch.float16, device=x.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape) == (planes, m, ldo)
    name = "dca_split_planes_scaled" if planes == 2 else "dca_cast_planes_scaled"
    check(getattr(lib(), name)(_raw(x), m, n, ld, _raw(amax), *_plane_ptrs(out), ldo, n_pad, stream_ptr()), name)
    return out


def _rows_scaled(planes: int, w, other_amax, k_pad, ldo, out, col_scale, n, k, ld):
    """split_rows_scaled (planes = 2) and cast_rows_scaled (1): the defaults, the [planes, n, ldo] buffer, col_scale, the call."""
    n, k, ld = _rows_cols_ld(w, n, k, ld)
    k_pad = k if k_pad is None else int(k_pad)
    ldo = k_pad if ldo is None else int(ldo)
    if out is None:
        out = torch.empty((planes, n, ldo), dtype=torch.float16, device=w.device)
    if col_scale is None:
        col_scale = torch.empty(n, dtype=torch.float32, device=w.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape) == (planes, n, ldo)
    assert col_scale.dtype == torch.float32 and col_scale.is_contiguous() and col_scale.numel() >= n
    name = "dca_split_rows_scaled" if planes == 2 else "dca_cast_rows_scaled"
    check(getattr(lib(), name)(_raw(w), n, k, ld, *_plane_ptrs(out), ldo, k_pad, _raw(col_scale), _raw(other_amax), stream_ptr()), name)
    return out, col_scale


def split_planes_scaled(x: torch.Tensor, amax: Optional[torch.Tensor] = None, n_pad: Optional[int] = None,
                        ldo: Optional[int] = None, out: Optional[torch.Tensor] = None, m: Optional[int] = None,
                        n: Optional[int] = None, ld: Optional[int] = None) -> torch.Tensor:
    """fp32 [m, n] (row stride ld) * 2^e -> its fp16 planes out[0] (high) / out[1] (low), [2, m, ldo] (dca_split_planes_scaled):
    2^e takes the |max| whose bits `amax` holds into [2^14, 2^15) (amax None: unscaled); columns n..n_pad are written as zeros,
    columns n_pad..ldo are not touched.  n_pad defaults to n, ldo to n_pad; `out` may be a buffer of the caller's."""
    return _planes_scaled(2, x, amax, n_pad, ldo, out, m, n, ld)


def split_rows_scaled(w: torch.Tensor, other_amax: Optional[torch.Tensor] = None, k_pad: Optional[int] = None,
                      ldo: Optional[int] = None, out: Optional[torch.Tensor] = None, col_scale: Optional[torch.Tensor] = None,
                      n: Optional[int] = None, k: Optional[int] = None, ld: Optional[int] = None):
    """Per row of w [n, k] fp32 (row stride ld): the row's own power-of-two scale 2^e (its |max| into [2^14, 2^15)), the fp16
    planes of row * 2^e in out [2, n, ldo] (columns k..k_pad zero, k_pad..ldo untouched) and col_scale[row] = 1 / (2^e * the scale
    of the OTHER operand, whose |max| bits `other_amax` holds; None: 1) (dca_split_rows_scaled).  -> (out, col_scale)."""
    return _rows_scaled(2, w, other_amax, k_pad, ldo, out, col_scale, n, k, ld)


def fill_inv_pow2(amax: torch.Tensor, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[0..n) = the reciprocal of the power-of-two scale split_planes_scaled derives from `amax` (dca_fill_inv_pow2)."""
    if out is None:
        out = torch.empty(int(n), dtype=torch.float32, device=amax.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    check(lib().dca_fill_inv_pow2(_raw(out), n, _raw(amax), stream_ptr()), "dca_fill_inv_pow2")
    return out


def cast_planes_scaled(x: torch.Tensor, amax: Optional[torch.Tensor] = None, n_pad: Optional[int] = None,
                       ldo: Optional[int] = None, out: Optional[torch.Tensor] = None, m: Optional[int] = None,
                       n: Optional[int] = None, ld: Optional[int] = None) -> torch.Tensor:
    """The HIGH plane alone of split_planes_scaled, bit for bit, as a [1, m, ldo] fp16 tensor (dca_cast_planes_scaled): what the
    one-product kernels read (f16_gemm; wgrad_f16 with products = 1 takes the tensor as it is).  Same arguments and padding."""
    return _planes_scaled(1, x, amax, n_pad, ldo, out, m, n, ld)


def cast_rows_scaled(w: torch.Tensor, other_amax: Optional[torch.Tensor] = None, k_pad: Optional[int] = None,
                     ldo: Optional[int] = None, out: Optional[torch.Tensor] = None, col_scale: Optional[torch.Tensor] = None,
                     n: Optional[int] = None, k: Optional[int] = None, ld: Optional[int] = None):
    """The HIGH plane alone of split_rows_scaled, bit for bit, as a [1, n, ldo] fp16 tensor, and the same col_scale
    (dca_cast_rows_scaled).  -> (out, col_scale)."""
    return _rows_scaled(1, w, other_amax, k_pad, ldo, out, col_scale, n, k, ld)


def f16_gemm(a_h: torch.Tensor, w_h: torch.Tensor, col_scale: Optional[torch.Tensor], alpha: float,
             bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(a_h . w_h^T) * alpha * col_scale + bias -> fp32 [m, n] on the one-product kernel dca_f16_gemm: 11-bit operands, fp32
    accumulation, NOT a parity mode.  a_h [m, k] / w_h [n, k] fp16 of unit column stride (row views of wider matrices welcome),
    k % 64 == 0; `out`: an fp32 [m, n] view of unit column stride to write into (its other columns are not touched)."""
    for t in (a_h, w_h):
        assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
    m, k = a_h.shape
    n = w_h.shape[0]
    assert w_h.shape[1] == k
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a_h.device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (m, n) and out.stride(1) == 1
    check(lib().dca_f16_gemm(_raw(a_h), m, k, a_h.stride(0) if m > 1 else k, _raw(w_h), n, w_h.stride(0) if n > 1 else k,
                             ptr(col_scale), alpha, ptr(bias), _raw(out), out.stride(0) if m > 1 else (n + 3) // 4 * 4, stream_ptr()),
          "dca_f16_gemm")
    return out


def _train_gemm(planes: torch.Tensor, amax: Optional[torch.Tensor], w: torch.Tensor, bias: Optional[torch.Tensor], gemm: str) -> torch.Tensor:
    """a . w^T (+ bias) -> fp32 [m, n] on planes of `a` that exist already ([1 or 2, m, pad64(k)], scaled by `amax`; None: unscaled):
    the rows of w [n, k] prepared on the spot, then the GEMM.  gemm "f16x3": split_rows_scaled + dca_f16x3_gemm on both planes;
    "f16": cast_rows_scaled + dca_f16_gemm on plane 0.  Every forward and input-gradient GEMM of linear_train is one call of this."""
    bias = None if bias is None else bias.contiguous()
    if gemm == "f16x3":
        wp, cs = split_rows_scaled(w, amax, k_pad=planes.shape[2])
        return f16x3_gemm(planes, wp[0], wp[1], cs, 1.0, bias, None, False, False, True)[1]
    wh, cs = cast_rows_scaled(w, amax, k_pad=planes.shape[2])
    return f16_gemm(planes[0], wh[0], cs, 1.0, bias)


def linear_f16x3(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], scale_a: bool,
                 amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [m, k] fp32 . w [n, k]^T (+ bias) -> [m, n] fp32 through dca_f16x3_gemm (fp32-accurate on the f16 matrix pipes),
    operands prepared on the spot: rows of w scaled by their own power of two (split_rows_scaled), `a` by one power of two
    for the whole tensor when scale_a (absmax_bits + split_planes_scaled; the forward's activations and the backward's
    gradients both take it).  k, n % 4 == 0; K is zero-padded to a multiple of 64 inside the planes (the kernels write the
    pad: the planes come from torch.empty)."""
    assert a.is_cuda and a.dtype == torch.float32 and w.dtype == torch.float32 and a.dim() == 2 and w.dim() == 2
    a, w = a.contiguous(), w.contiguous()
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and k % 4 == 0 and n % 4 == 0
    kp = _pad64(k)
    if scale_a and amax is None:  # (the backward pass takes max|dy| once for both of its GEMMs)
        amax = absmax_bits(a)
    if not scale_a:
        amax = None
    return _train_gemm(split_planes_scaled(a, amax, n_pad=kp), amax, w, bias, "f16x3")


WGRAD_MODES = ("library", "f16x3", "f16")  # how the training step computes nn.Linear's weight gradient (linear_train)
TRAIN_GEMM_MODES = ("f16x3", "f16")  # how the training step runs nn.Linear's forward and input-gradient GEMMs (linear_train)


def wgrad_splits(m: int, n: int, k: int) -> int:
    """Slices dca_wgrad_f16 cuts m batch rows into for an [n, k] weight gradient: a function of the three sizes alone."""
    s = lib().dca_wgrad_splits(m, n, k)
    check(min(s, 0), "dca_wgrad_splits")
    return s


def wgrad_workspace_bytes(m: int, n: int, k: int) -> int:
    """Bytes of fp32 workspace dca_wgrad_f16 needs: 0 with one slice, else slices * n * k * 4."""
    b = lib().dca_wgrad_workspace_bytes(m, n, k)
    check(min(b, 0), "dca_wgrad_workspace_bytes")
    return b


def wgrad_f16(dy_planes: torch.Tensor, x_planes: torch.Tensor, n: int, k: int, amax_dy: Optional[torch.Tensor],
              amax_x: Optional[torch.Tensor], products: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW [n, k] fp32 = dy^T . x from the fp16 planes of dy [2, m, ld_dy] and x [2, m, ld_x] (split_planes_scaled's, widths
    zero-padded to a multiple of 64; amax_dy / amax_x: the words they were scaled by, None = unscaled) on dca_wgrad_f16.
    products = 3: fp32-accurate (dyh.xh + dyh.xl + dyl.xh); products = 1: the high planes alone (non-parity; a [1, m, ld] tensor
    will do).  `out`: an fp32 [n, k] view of unit column stride to write into (its other columns are not touched)."""
    for t in (dy_planes, x_planes):
        assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 3 and t.is_contiguous()
    m = int(dy_planes.shape[1])
    assert x_planes.shape[1] == m
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=dy_planes.device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, k) and out.stride(1) == 1
    need = wgrad_workspace_bytes(m, n, k)
    ws = torch.empty(need, dtype=torch.uint8, device=out.device) if need else None
    dy_l, x_l = (t[1] if (t.shape[0] > 1 and products != 1) else None for t in (dy_planes, x_planes))
    check(lib().dca_wgrad_f16(_raw(dy_planes[0]), _raw(dy_l), dy_planes.shape[2], _raw(x_planes[0]), _raw(x_l), x_planes.shape[2], m, n,
                              k, _raw(amax_dy), _raw(amax_x), products, _raw(out), out.stride(0) if n > 1 else k, ptr(ws), need,
                              stream_ptr()), "dca_wgrad_f16")
    return out


class _LinearTrainFn(torch.autograd.Function):
    """nn.Linear for the training step (reference nnet_utils.py:53-118 runs it as the library's fp32 GEMMs), in every mode of
    gemm (TRAIN_GEMM_MODES) x wgrad (WGRAD_MODES).  Three facts make the table:

      * planes made of an activation or gradient tensor: 2 (split_planes_scaled) if gemm or wgrad is "f16x3", else 1
        (cast_planes_scaled: half the bytes).  One power-of-two scale per tensor from its own magnitude (absmax_bits: one extra
        pass; without it a value beyond 65504 turns into inf in its fp16 plane and the loss into NaN without a word).
      * weight rows and the GEMM of y = x . W^T + b and dx = dy . W (_train_gemm; 2/3 of the layer's flops): "f16x3" =
        split_rows_scaled + dca_f16x3_gemm, fp32-accurate at ~3x the library's fp32 rate; "f16" = cast_rows_scaled + dca_f16_gemm
        on plane 0 — 11-bit operands, one product instead of three, NOT a parity mode.
      * kept for the backward pass: (x, weight) for wgrad "library" — dW = dy^T . x is the library's fp32 GEMM, as the reference —
        else (planes of x, their amax word, weight): dW on dca_wgrad_f16 from those and the planes of dy, which the backward
        makes once for both gradients, with three products ("f16x3", fp32-accurate) or the high planes alone ("f16").  The
        kernel contracts over the BATCH dimension reading the row-major planes with the transposing LDS read."""

    @staticmethod
    def forward(ctx, x, weight, bias, wgrad, gemm):
        ctx.has_bias = bias is not None
        ctx.wgrad, ctx.gemm = wgrad, gemm
        ctx.planes = split_planes_scaled if "f16x3" in (gemm, wgrad) else cast_planes_scaled
        xc = x.contiguous()
        amax_x = absmax_bits(xc)
        xp = ctx.planes(xc, amax_x, n_pad=_pad64(x.shape[1]))
        if wgrad == "library":
            ctx.save_for_backward(x, weight)
        else:
            ctx.save_for_backward(xp, amax_x, weight)
        return _train_gemm(xp, amax_x, weight.contiguous(), bias, gemm)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        weight = ctx.saved_tensors[-1]
        n, k = weight.shape
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        if need_dx or (need_dw and ctx.wgrad != "library"):  # (fc1 has no input gradient: its planes of dy serve dW alone)
            amax = absmax_bits(dy)
            dyp = ctx.planes(dy, amax, n_pad=_pad64(n))
            if need_dx:
                dx = _train_gemm(dyp, amax, weight.t().contiguous(), None, ctx.gemm)
        if need_dw:
            if ctx.wgrad == "library":
                dw = dy.t().mm(ctx.saved_tensors[0])
            else:
                xp, amax_x = ctx.saved_tensors[0], ctx.saved_tensors[1]
                dw = wgrad_f16(dyp, xp, n, k, amax, amax_x, 3 if ctx.wgrad == "f16x3" else 1)
        db = dy.sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None, None


def linear_train(x: torch.Tensor, lin: "torch.nn.Linear", wgrad: str = "library", gemm: str = "f16x3") -> torch.Tensor:
    """`lin(x)` inside the training step.  The f16x3 path needs the GPU, fp32, 4-element-aligned widths and enough rows to
    fill a tile; anything else (the 1-wide output layer, the host) is F.linear.  wgrad (WGRAD_MODES): where the f16x3 path
    computes the weight gradient; the layers that go to F.linear are the same in every mode.  gemm (TRAIN_GEMM_MODES): "f16x3"
    (default) = forward and input gradient fp32-accurate on dca_f16x3_gemm; "f16" = the same layers on dca_f16_gemm, the high
    planes alone — 11-bit operands, NOT a parity mode."""
    if wgrad not in WGRAD_MODES:
        raise ValueError("wgrad must be one of %s, not %r" % ("/".join(WGRAD_MODES), wgrad))
    if gemm not in TRAIN_GEMM_MODES:
        raise ValueError("gemm must be one of %s, not %r" % ("/".join(TRAIN_GEMM_MODES), gemm))
    if (x.is_cuda and x.dtype == torch.float32 and lin.weight.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 256
            and lin.in_features % 4 == 0 and lin.out_features % 4 == 0 and lin.in_features >= 64 and TRAIN_F16X3):
        return _LinearTrainFn.apply(x, lin.weight, lin.bias, wgrad, gemm)
    return torch.nn.functional.linear(x, lin.weight, lin.bias)


TRAIN_F16X3 = os.environ.get("DCA_TRAIN_GEMM", "f16x3") != "library"  # A/B switches (bench.py --workload train, tools/train_grad_check.py)
# initial GEMM mode of new models (ResnetModel.set_train_gemm): exactly "f16" selects the non-parity one-product mode
TRAIN_GEMM = "f16" if os.environ.get("DCA_TRAIN_GEMM") == "f16" else "f16x3"
TRAIN_WGRAD = os.environ.get("DCA_TRAIN_WGRAD", "library")  # initial weight-gradient mode of new models (ResnetModel.set_wgrad)
if TRAIN_WGRAD not in WGRAD_MODES:
    raise ValueError("DCA_TRAIN_WGRAD must be one of %s, not %r" % ("/".join(WGRAD_MODES), TRAIN_WGRAD))

# ------------------------------------------------------------------------------ heuristic network, layer 1
def l1_supported(state_dim: int, depth: int) -> bool:
    return bool(lib().dca_l1_supported(state_dim, depth))


def l1_kpad(state_dim: int, depth: int) -> int:
    return lib().dca_l1_kpad(state_dim, depth)


def _l1_out(x: torch.Tensor, n_pad: int, out_dtype, split):
    """Output tensor and DCA_DT_* code of a layer-1 forward on the rows x: the two fp16 planes [2, m, n_pad] for split="planes",
    else [m, n_pad] in out_dtype (e4m3: the caller has folded the activation scale into the weights and bias)."""
    m = x.shape[0]
    if split == "planes":
        return torch.empty((2, m, n_pad), dtype=torch.float16, device=x.device), DT_F16_PLANES
    if out_dtype == E4M3:
        return torch.empty((m, n_pad), dtype=E4M3, device=x.device), DT_E4M3
    return torch.empty((m, n_pad), dtype=out_dtype, device=x.device), _TORCH_DT[out_dtype]


def l1_onehot_gemm(states_nnet: torch.Tensor, depth: int, w_tiles: torch.Tensor, planes: int, bias: torch.Tensor,
                   relu: bool, out_dtype, split=False, overflow: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu?(onehot(states_nnet) @ W1^T + b1) from the uint8 rows, [m, n_pad] in out_dtype (dca_l1_onehot_gemm);
    split="planes": dca_f16x3_gemm's operand [2, m, n_pad] fp16 of the next layer instead (high halves, low halves;
    DCA_DT_F16_PLANES)."""
    if split not in (False, "planes"):
        raise ValueError("l1_onehot_gemm: split is False or 'planes', not %r" % (split,))
    x = _u8(states_nnet)
    m, d = x.shape
    n_pad = bias.numel()
    out, code = _l1_out(x, n_pad, out_dtype, split)  # (e4m3: planes == 1)
    check(lib().dca_l1_onehot_gemm(ptr(x), m, d, depth, ptr(w_tiles), planes, n_pad, ptr(bias), relu, ptr(out), code, ptr(overflow),
                                   stream_ptr()), "dca_l1_onehot_gemm")
    return out


def l1_supported8(state_dim: int, depth: int) -> bool:
    return bool(lib().dca_l1_supported8(state_dim, depth))


def l1_kpad8(state_dim: int, depth: int) -> int:
    return lib().dca_l1_kpad8(state_dim, depth)


def l1_onehot_gemm8(states_nnet: torch.Tensor, depth: int, w_tiles8: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor,
                    relu: bool) -> torch.Tensor:
    """Layer 1 of the fp8 mode on the f8f6f4 pipe (dca_l1_onehot_gemm8): e4m3(sat(relu?((onehot(s) . w8^T) * scale + bias))),
    [m, n_pad] e4m3, from the uint8 rows; w_tiles8 from pytorch_models.l1_weight_tiles8."""
    x = _u8(states_nnet)
    m, d = x.shape
    n_pad = bias.numel()
    assert scale.dtype == torch.float32 and bias.dtype == torch.float32 and scale.numel() == n_pad and n_pad % 128 == 0
    out = torch.empty((m, n_pad), dtype=E4M3, device=x.device)
    check(lib().dca_l1_onehot_gemm8(ptr(x), m, d, depth, ptr(w_tiles8), n_pad, ptr(scale), ptr(bias), relu, ptr(out), stream_ptr()),
          "dca_l1_onehot_gemm8")
    return out


def l1_embed_supported(state_dim: int, depth: int) -> bool:
    return bool(lib().dca_l1_embed_supported(state_dim, depth))


def l1_embed(states_nnet: torch.Tensor, depth: int, w_t: torch.Tensor, bias: torch.Tensor, relu: bool, out_dtype=torch.float32,
             split=False, overflow: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Layer 1 as an embedding sum (dca_l1_embed): relu?(b1 + sum_pos w_t[pos * depth + s[pos]]) in exact fp32 arithmetic from
    the uint8 rows; w_t = W1^T fp32 [state_dim * depth, n_pad].  [m, n_pad] in out_dtype (fp32 / bf16 / e4m3 saturating), or split="planes":
    dca_f16x3_gemm's operand [2, m, n_pad] fp16."""
    x = _u8(states_nnet)
    if x.data_ptr() % 16:  # a row slice of a larger matrix: the kernel streams the rows in 16-byte pieces
        x = x.clone()
    m, d = x.shape
    n_pad = bias.numel()
    assert w_t.dtype == torch.float32 and bias.dtype == torch.float32 and w_t.is_contiguous() and tuple(w_t.shape) == (d * depth, n_pad)
    assert split == "planes" or out_dtype == E4M3 or (not split and out_dtype in (torch.float32, torch.bfloat16))
    out, code = _l1_out(x, n_pad, out_dtype, split)
    if m == 0:
        return out
    check(lib().dca_l1_embed(ptr(x), m, d, depth, ptr(w_t), n_pad, ptr(bias), relu, ptr(out), code, ptr(overflow), stream_ptr()),
          "dca_l1_embed")
    return out


def l1_embed_wgrad_slice_rows(state_dim: int, depth: int) -> int:
    """Rows per slice of dca_l1_embed_wgrad's summation order (a property of the geometry; 0: one slice)."""
    s = lib().dca_l1_embed_wgrad_slice_rows(state_dim, depth)
    check(min(s, 0), "dca_l1_embed_wgrad_slice_rows")
    return s


def l1_embed_wgrad(states_nnet: torch.Tensor, dy: torch.Tensor, depth: int, want_bias: bool = True):
    """Weight gradient of layer 1 from the uint8 rows (dca_l1_embed_wgrad): dW[j, pos * depth + v] = the sum of dy[r, j] over
    the rows with s[r, pos] == v, db[j] = the sum of dy[:, j] — fp32, in the fixed order include/dca.h states (bit-identical from
    launch to launch).  dy: fp32 [m, n] of unit column stride (a column slice of a wider matrix is fine), n % 4 == 0.
    -> (dW [n, state_dim * depth] in nn.Linear's layout, db [n] or None)."""
    x = _u8(states_nnet)
    assert dy.is_cuda and dy.dtype == torch.float32 and dy.dim() == 2 and dy.shape[0] == x.shape[0]
    if dy.stride(1) != 1 or dy.stride(0) % 4 or dy.stride(0) < dy.shape[1] or dy.data_ptr() % 16:
        dy = dy.contiguous()
    m, d = x.shape
    n = int(dy.shape[1])
    dw = torch.empty((n, d * depth), dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device) if want_bias else None
    if m == 0 or n == 0:  # (an empty tensor has no address to hand over)
        return dw.zero_(), (None if db is None else db.zero_())
    need = lib().dca_l1_embed_wgrad_workspace_bytes(m, d, depth, n)
    check(min(need, 0), "dca_l1_embed_wgrad_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    check(lib().dca_l1_embed_wgrad(ptr(x), m, d, depth, _raw(dy), dy.stride(0) if m > 1 else n, n, ptr(dw), d * depth, ptr(db), ptr(ws),
                                   need, stream_ptr()), "dca_l1_embed_wgrad")
    return dw, db


class _L1EmbedTrainFn(torch.autograd.Function):
    """fc1 of the training step straight from the uint8 rows (reference: utils/pytorch_models.py:49-60 on the one-hot matrix,
    differentiated by utils/nnet_utils.py:53-118): forward = the embedding sum dca_l1_embed (exact fp32, positions ascending),
    backward = its scatter dca_l1_embed_wgrad.  The one-hot matrix never exists; the states get no gradient."""

    @staticmethod
    def forward(ctx, states, depth, weight, bias):
        n, k = weight.shape
        n_pad = _pad64(n)
        # the forward kernel stages W^T [K, n_pad] (n_pad % 64 == 0): one padded transposing copy per step
        w_t = torch.empty((k, n_pad), dtype=torch.float32, device=weight.device)
        w_t[:, :n].copy_(weight.detach().t())
        w_t[:, n:].zero_()
        b = torch.zeros(n_pad, dtype=torch.float32, device=weight.device)
        if bias is not None:
            b[:n].copy_(bias.detach())
        y = l1_embed(states, depth, w_t, b, relu=False)
        ctx.save_for_backward(states)
        ctx.depth, ctx.has_bias = int(depth), bias is not None
        return y if n_pad == n else y[:, :n].contiguous()  # (bn_train wants a contiguous matrix)

    @staticmethod
    def backward(ctx, dy):
        (states,) = ctx.saved_tensors
        want_w, want_b = ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3]
        dw = db = None
        if want_w:
            dw, db = l1_embed_wgrad(states, dy, ctx.depth, want_bias=want_b)
        elif want_b:  # a frozen weight: no scatter, the bias gradient alone is a column sum
            db = dy.sum(0)
        return None, None, dw, db


def l1_embed_train(states_nnet: torch.Tensor, lin: "torch.nn.Linear", depth: int) -> torch.Tensor:
    """`lin(one_hot(states))` inside the training step without the one-hot matrix: uint8 [m, state_dim] -> fp32 [m, out_features]
    (contiguous), differentiable in lin.weight and lin.bias.  A missing kernel is an error: the geometry must be one
    dca_l1_embed_supported names and out_features % 4 == 0."""
    x = _u8(states_nnet)
    if not l1_embed_supported(x.shape[1], depth) or lin.in_features != x.shape[1] * depth or lin.out_features % 4:
        raise DcaError("l1_embed_train: no kernel for state_dim %d, depth %d, %d -> %d units" %
                       (x.shape[1], depth, lin.in_features, lin.out_features))
    assert lin.weight.is_cuda and lin.weight.dtype == torch.float32
    return _L1EmbedTrainFn.apply(x, int(depth), lin.weight, lin.bias)


def act_split(y: torch.Tensor, bias: Optional[torch.Tensor], skip: Optional[torch.Tensor], alpha, relu: bool,
              want_x: bool, want_a3="planes", overflow: Optional[torch.Tensor] = None):
    """v = relu?(y*alpha + bias (+ skip)) -> (a3, v fp32 or None).  want_a3="planes": a3 = dca_f16x3_gemm's operand [2,m,n] fp16
    (high halves, low halves); False: None."""
    if want_a3 not in (False, "planes"):
        raise ValueError("act_split: want_a3 is 'planes' or False, not %r" % (want_a3,))
    assert y.dtype == torch.float32 and y.is_contiguous() and (want_x or want_a3)
    m, n = y.shape
    a3 = torch.empty((2, m, n), dtype=torch.float16, device=y.device) if want_a3 else None
    x_out = torch.empty_like(y) if want_x else None
    col_scale = alpha if isinstance(alpha, torch.Tensor) else None  # per-output-unit scale vector or one scalar
    check(lib().dca_act_split(ptr(y), ptr(bias), ptr(skip), ptr(col_scale), 1.0 if col_scale is not None else alpha, relu, m, n,
                              ptr(x_out), ptr(a3), ptr(overflow), stream_ptr()), "dca_act_split")
    return a3, x_out


def split_planes(x: torch.Tensor, overflow: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [m, n] -> its fp16 planes [2, m, n] (x = planes[0] + planes[1] to 22 bits): the operand of f16x3_gemm."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] % 4 == 0
    m, n = x.shape
    out = torch.empty((2, m, n), dtype=torch.float16, device=x.device)
    check(lib().dca_split_planes(ptr(x), m, n, n, ptr(out[0]), ptr(out[1]), n, ptr(overflow), stream_ptr()), "dca_split_planes")
    return out


def f16x3_gemm(a_planes: torch.Tensor, w_h: torch.Tensor, w_l: torch.Tensor, col_scale: Optional[torch.Tensor], alpha: float,
               bias: Optional[torch.Tensor], skip: Optional[torch.Tensor], relu: bool, want_planes: bool, want_x: bool,
               overflow: Optional[torch.Tensor] = None):
    """One dense layer of the cost-to-go network as the hand-written fp32-accurate MFMA kernel (dca_f16x3_gemm):
    v = relu?((a . w^T) * alpha * col_scale + bias (+ skip)).  a_planes [2, m, k] fp16, w_h / w_l [n, k] fp16.
    -> (planes of v [2, m, n] fp16 or None, v fp32 [m, n] or None)."""
    assert a_planes.dtype == torch.float16 and a_planes.dim() == 3 and a_planes.is_contiguous()
    assert w_h.dtype == torch.float16 and w_h.is_contiguous() and w_l.is_contiguous() and w_h.shape == w_l.shape
    _, m, k = a_planes.shape
    n = w_h.shape[0]
    assert w_h.shape[1] == k and (want_planes or want_x)
    planes = torch.empty((2, m, n), dtype=torch.float16, device=a_planes.device) if want_planes else None
    x_out = torch.empty((m, n), dtype=torch.float32, device=a_planes.device) if want_x else None
    check(lib().dca_f16x3_gemm(ptr(a_planes[0]), ptr(a_planes[1]), m, k, k, ptr(w_h), ptr(w_l), n, k, ptr(col_scale), alpha, ptr(bias),
                               ptr(skip), relu, ptr(planes[0]) if want_planes else None, ptr(planes[1]) if want_planes else None,
                               ptr(x_out), n, ptr(overflow), stream_ptr()), "dca_f16x3_gemm")
    return planes, x_out


def gemm16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], skip: Optional[torch.Tensor], relu: bool,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One dense layer in the non-parity 16-bit modes (dca_gemm16): relu?(a . w^T + bias (+ skip)), a [m, k] / w [n, k] /
    skip [m, n] bf16 or fp16, bias fp32, fp32 accumulation, result in the operands' type.  `out` may be `skip` (in place)."""
    assert a.dtype in (torch.bfloat16, torch.float16) and w.dtype == a.dtype and a.is_contiguous() and w.is_contiguous()
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and (bias is None or (bias.dtype == torch.float32 and bias.numel() == n))
    assert skip is None or (skip.dtype == a.dtype and skip.shape == (m, n) and skip.is_contiguous())
    if out is None:
        out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    assert out.dtype == a.dtype and out.shape == (m, n) and out.is_contiguous() and out.data_ptr() != a.data_ptr()
    check(lib().dca_gemm16(ptr(a), m, k, k, ptr(w), n, k, _TORCH_DT[a.dtype], ptr(bias), ptr(skip), relu, ptr(out), n, stream_ptr()),
          "dca_gemm16")
    return out


def gemm8(a: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor], skip: Optional[torch.Tensor],
          relu: bool, want16: bool, out8_scale: Optional[float], out16: Optional[torch.Tensor] = None):
    """One dense layer in the fp8 mode (dca_gemm8): v = relu?((a . w^T) * scale + bias (+ skip)), a [m, k] / w [n, k] e4m3, scale /
    bias [n] fp32, skip [m, n] bf16.  Returns (bf16 v or None, e4m3(sat(v * out8_scale)) or None); `out16` may be `skip`."""
    assert a.dtype == E4M3 and w.dtype == E4M3 and a.is_contiguous() and w.is_contiguous()
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and scale.dtype == torch.float32 and scale.numel() == n
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == n)
    assert skip is None or (skip.dtype == torch.bfloat16 and skip.shape == (m, n) and skip.is_contiguous())
    if want16 and out16 is None:
        out16 = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    assert out16 is None or (out16.dtype == torch.bfloat16 and out16.shape == (m, n) and out16.is_contiguous())
    out8 = torch.empty((m, n), dtype=E4M3, device=a.device) if out8_scale is not None else None
    check(lib().dca_gemm8(ptr(a), m, k, k, ptr(w), n, k, ptr(scale), ptr(bias), ptr(skip), relu, ptr(out16), n, ptr(out8), n,
                          out8_scale if out8_scale is not None else 1.0, stream_ptr()), "dca_gemm8")
    return out16, out8


def gemm8_mx(a: torch.Tensor, a_scale: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor],
             skip: Optional[torch.Tensor], relu: bool, want16: bool, want8: bool, out16: Optional[torch.Tensor] = None):
    """One dense layer in the block-scaled fp8 mode (dca_gemm8_mx): a [m, k] e4m3 with a_scale [m, k/64] E8M0 bytes, w [n, k] e4m3 with
    w_scale [n] fp32.  -> (bf16 v or None, e4m3 v blocks or None, their E8M0 scales [m, n/64] or None); `out16` may be `skip`."""
    assert a.dtype == E4M3 and w.dtype == E4M3 and a.is_contiguous() and w.is_contiguous()
    m, k = a.shape
    n = w.shape[0]
    assert a_scale.dtype == torch.uint8 and a_scale.shape == (m, k // 64) and a_scale.is_contiguous()
    assert w.shape[1] == k and w_scale.dtype == torch.float32 and w_scale.numel() == n
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == n)
    assert skip is None or (skip.dtype == torch.bfloat16 and skip.shape == (m, n) and skip.is_contiguous())
    if want16 and out16 is None:
        out16 = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    out8 = torch.empty((m, n), dtype=E4M3, device=a.device) if want8 else None
    out_sc = torch.empty((m, n // 64), dtype=torch.uint8, device=a.device) if want8 else None
    check(lib().dca_gemm8_mx(ptr(a), ptr(a_scale), m, k, k, k // 64, ptr(w), n, k, ptr(w_scale), ptr(bias), ptr(skip), relu, ptr(out16),
                             n, ptr(out8), n, ptr(out_sc), n // 64, stream_ptr()), "dca_gemm8_mx")
    return out16, out8, out_sc


def l1_onehot_gemm_mx(states_nnet: torch.Tensor, depth: int, w_tiles: torch.Tensor, bias: torch.Tensor, relu: bool):
    """Layer 1 (one bf16 weight plane) leaving as e4m3 + one E8M0 block scale per row and 64 units (dca_l1_onehot_gemm_mx)
    -> (e4m3 [m, n_pad], uint8 [m, n_pad / 64])."""
    x = _u8(states_nnet)
    m, d = x.shape
    n_pad = bias.numel()
    out = torch.empty((m, n_pad), dtype=E4M3, device=x.device)
    sc = torch.empty((m, n_pad // 64), dtype=torch.uint8, device=x.device)
    check(lib().dca_l1_onehot_gemm_mx(ptr(x), m, d, depth, ptr(w_tiles), n_pad, ptr(bias), relu, ptr(out), ptr(sc), n_pad // 64,
                                      stream_ptr()), "dca_l1_onehot_gemm_mx")
    return out, sc


def quant_e4m3(x: torch.Tensor, scale: float) -> torch.Tensor:
    """fp32 / bf16 [m, n] -> e4m3(sat(x * scale)) (dca_quant_e4m3)."""
    assert x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous() and x.dim() == 2 and x.shape[1] % 4 == 0
    m, n = x.shape
    out = torch.empty((m, n), dtype=E4M3, device=x.device)
    check(lib().dca_quant_e4m3(ptr(x), _TORCH_DT[x.dtype], m, n, n, scale, ptr(out), n, stream_ptr()), "dca_quant_e4m3")
    return out


def _row_view(t: torch.Tensor, even: bool) -> bool:
    """A 2-d device view whose rows are contiguous and do not overlap (row stride >= width; even where the kernel loads pairs)."""
    return (t.is_cuda and t.dim() == 2 and (t.shape[1] == 0 or t.stride(1) == 1) and t.stride(0) >= t.shape[1]
            and not (even and t.stride(0) % 2))


def head_gemv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out_dtype: torch.dtype = torch.float32,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Output layer (dca_head_gemv): x [m, k] fp32 / fp16 / bf16 / float64 (rows may be strided), w [n_out, k] fp32, bias [n_out] fp32
    -> [m, n_out] fp32, summed in float64 in a fixed order (a row's bits do not depend on m or on the row's position) and rounded
    once.  out_dtype=torch.float64 (float64 rows only, dca_head_gemv64): the same sum, not rounded.  `out`: a contiguous
    [m, n_out] tensor of out_dtype to write into."""
    dts = {**_TORCH_DT, torch.float64: DT_F64}
    assert x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.dtype in dts
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape[1] == x.shape[1]
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == w.shape[0])
    assert out_dtype == torch.float32 or (out_dtype == torch.float64 and x.dtype == torch.float64)
    m, k = x.shape
    if out is None:
        out = torch.empty((m, w.shape[0]), dtype=out_dtype, device=x.device)
    assert out.dtype == out_dtype and tuple(out.shape) == (m, w.shape[0])
    if m == 0:
        return out
    if out_dtype == torch.float64:
        check(lib().dca_head_gemv64(_raw(x), m, k, x.stride(0), ptr(w), ptr(bias), w.shape[0], ptr(out), stream_ptr()),
              "dca_head_gemv64")
        return out
    check(lib().dca_head_gemv(_raw(x), dts[x.dtype], m, k, x.stride(0), ptr(w), ptr(bias), w.shape[0], ptr(out), stream_ptr()),
          "dca_head_gemv")
    return out


def gemm64(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], skip: Optional[torch.Tensor], relu: bool,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One dense layer of the fp64 mode (dca_gemm64): relu?(a . w^T + bias (+ skip)), a [m, k] / w [n, k] / bias [n] / skip [m, n]
    float64, f64 MFMA, every element summed over k in ascending order.  `out` may be `skip` (in place).  a, w, skip and out may
    be row-strided views (stride(1) == 1, row stride >= width; a's and w's even): their row strides go to the kernel as lda,
    ldw and ldo, and skip must have out's."""
    assert a.dtype == torch.float64 and w.dtype == torch.float64 and _row_view(a, True) and _row_view(w, True)
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and (bias is None or (bias.dtype == torch.float64 and bias.numel() == n and bias.is_contiguous()))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float64, device=a.device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (m, n) and _row_view(out, False) and out.data_ptr() != a.data_ptr()
    assert skip is None or (skip.dtype == torch.float64 and tuple(skip.shape) == (m, n) and _row_view(skip, False)
                            and skip.stride(0) == out.stride(0))  # one ldo for both
    assert skip is None or skip.data_ptr() == out.data_ptr() or skip.data_ptr() != a.data_ptr()
    check(lib().dca_gemm64(_raw(a), m, k, a.stride(0), _raw(w), n, w.stride(0), ptr(bias), _raw(skip), relu, _raw(out), out.stride(0),
                           stream_ptr()), "dca_gemm64")
    return out


def l1_embed64(states_nnet: torch.Tensor, depth: int, w_t: torch.Tensor, bias: torch.Tensor, relu: bool,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Layer 1 of the fp64 mode as an embedding sum (dca_l1_embed64): relu?(b1 + sum_pos w_t[pos * depth + s[pos]]) in float64
    (bias first, positions ascending) from the uint8 rows; w_t = W1^T float64 [state_dim * depth, n_pad] -> [m, n_pad] float64.
    The entry point takes no row strides: a strided view of the states is packed first, `out` (optional) is contiguous."""
    x = _u8(states_nnet)
    m, d = x.shape
    n_pad = bias.numel()
    assert w_t.dtype == torch.float64 and bias.dtype == torch.float64 and w_t.is_contiguous() and bias.is_contiguous()
    assert tuple(w_t.shape) == (d * depth, n_pad)
    if out is None:
        out = torch.empty((m, n_pad), dtype=torch.float64, device=x.device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (m, n_pad)
    if m == 0:
        return out
    check(lib().dca_l1_embed64(ptr(x), m, d, depth, ptr(w_t), n_pad, ptr(bias), relu, ptr(out), stream_ptr()), "dca_l1_embed64")
    return out


def gemm16_variant(v: int) -> None:
    """Test hook: 3 (default) = ping-pong schedule, swapped operand roles, lean tail per layer form; 2 = the same schedule with
    the general tail; 1 = two-stage loop (one drain + barrier per K-step).  Bit-identical results."""
    check(lib().dca_gemm16_variant(v), "dca_gemm16_variant")


def f16x3_gemm_variant(v: int) -> None:
    """Test hook: 3 (default) = LDS-DMA 256x256 kernel on the ping-pong schedule, 2 = the same tile with two whole-K-step
    stages (bit-identical)."""
    check(lib().dca_f16x3_gemm_variant(v), "dca_f16x3_gemm_variant")
