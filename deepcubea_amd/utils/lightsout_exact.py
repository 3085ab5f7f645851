"""The exact heuristic of lightsout7 (include/dca.h "exact LightsOut heuristic", csrc/dca_lightsout_exact.hip): a state is
s = A x over GF(2), A is invertible on the 7 x 7 board, so the distance of any state is popcount(A^-1 s) and its optimal solution
is "press the cells of A^-1 s, in any order".  No table: nothing to build, save or load.

`--model_dir exact:gf2` puts it into the search.  Its values are integers and every state reached by pressing a subset of the
solution's cells has the same f at `--weight 1` (2^h states for distance h): search with a weight below 1, where the
solution is still optimal."""
from __future__ import annotations

from typing import List

import torch

from .. import _lib

SPECS = ("gf2",)


def parse_exact_spec(env_name: str, spec: str) -> str:
    """`--model_dir exact:SPEC` -> SPEC; ValueError, with no device needed, for an environment other than lightsout7 or a
    name other than gf2."""
    name, spec = str(env_name).lower(), str(spec).strip().lower()
    if name != "lightsout7":
        raise ValueError("exact: is defined for lightsout7 only (the board whose press matrix is invertible over GF(2)), not for %r"
                         % (env_name,))
    if spec not in SPECS:
        raise ValueError("unknown exact heuristic %r for %s (have: %s)" % (spec, env_name, ", ".join(SPECS)))
    return spec


class LightsOutExact:
    """popcount(A^-1 s) and A^-1 s for uint8 device rows of lightsout7."""

    _engine_rows = "state"  # the network input of lightsout7 is the cells themselves (lights_out.py:70-75)

    def __init__(self, env_name: str):
        parse_exact_spec(env_name, "gf2")
        self.env_name = str(env_name).lower()
        self.spec = "gf2"

    def heuristic(self, states: torch.Tensor) -> torch.Tensor:
        """-> f32 [n]: the exact distance of every row (uint8 device rows [n, >= 49], strided views welcome)."""
        return _lib.lightsout_exact_eval(states)

    def solve(self, states: torch.Tensor) -> List[List[int]]:
        """-> per row the cells of its optimal solution, ascending (synchronises: the masks come to the host)."""
        masks = _lib.lightsout_exact_solve(states).cpu().tolist()
        return [[a for a in range(49) if (m >> a) & 1] for m in masks]

    def heuristic_fn_dev(self):
        """(uint8 rows on the device, is_onehot=False) -> float32 [m]: the closure form of BwasEngine.step / solve."""
        def fn(states: torch.Tensor, is_onehot: bool = False) -> torch.Tensor:
            if is_onehot:
                raise ValueError("a pattern database reads the uint8 %s rows, not one-hot rows" % self._engine_rows)
            return self.heuristic(states)
        return fn
