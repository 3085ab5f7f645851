"""Pattern databases for cube3 (include/dca.h "pattern databases for cube3", csrc/dca_pdb_cube3.hip): Korf's distance tables
over corner cubies and over subsets of the edge cubies, combined by max — an exact admissible, consistent heuristic.  With
`--env cube3 --model_dir pdb:<spec> --weight 1 --semantics cpp` the engine is an optimal solver (a spec without `+dual`).

A set is a tuple of patterns, a pattern a (kind, cubies) pair; `parse_cube3_pdb_spec` turns a preset name or explicit groups
("c0,c1,c2/e0,e1,e2,e3") into one and refuses what cannot be built, before any device work.  Patterns may share cubies: the
max of admissible tables is admissible.

`<spec>+sym` reads every table again at the state's conjugates under the cube's 48 symmetries, each pattern at all of its distinct
images, and takes the largest value (include/dca.h "Symmetric look-ups"): no table bytes, the same tables.  `<spec>+sym:N` takes
the first N images of each pattern; `+sym:1` is the plain heuristic.

`<spec>+dual` reads every look-up a second time at the INVERSE state and takes the larger value (include/dca.h "Dual look-ups"):
d(s^-1) = d(s), so the value stays admissible — but it is no longer consistent.  It composes with `+sym`: `<spec>+sym:N+dual`."""
from __future__ import annotations

import re
from math import perm
from typing import Dict, List, Tuple

import torch

from .. import _lib
from .pattern_db import _TableSet

Pattern = Tuple[int, Tuple[int, ...]]
PatternSet = Tuple[Pattern, ...]

_C, _E = _lib.CUBE3_CORNERS, _lib.CUBE3_EDGES
_PREFIX = {_C: "c", _E: "e"}
PRESETS: Dict[str, PatternSet] = {
    "corners": ((_C, tuple(range(8))),),
    "korf": ((_C, tuple(range(8))), (_E, tuple(range(0, 6))), (_E, tuple(range(6, 12)))),
    "korf7": ((_C, tuple(range(8))), (_E, tuple(range(0, 7))), (_E, tuple(range(5, 12)))),
}
MAX_K = 8
MAX_TABLE_BYTES = 1 << 34  # one pattern's table (the library's own limit)
SYM_SUFFIX = "+sym"  # a spec that ends in it, or in +sym:N, asks for the symmetric look-ups; the tables are the same
SYM_ALL = _lib.CUBE3_SYMS
DUAL_SUFFIX = "+dual"  # a spec with it asks for the dual look-ups as well; the tables and the look-up list are the same


def split_sym(spec: str) -> Tuple[str, int]:
    """A spec string -> (the spec parse_cube3_pdb_spec takes, N): N = 0 without a suffix, 48 for "+sym", N for "+sym:N" with N in
    1..48.  ValueError for any other use of '+' (a +reflect suffix among them: the parser words that refusal)."""
    spec = str(spec).strip()
    base, plus, suffix = spec.partition("+")
    if not plus:
        return spec, 0
    m = re.fullmatch(r"sym(?::\s*(-?\d+))?", suffix.strip().lower())
    if not m:
        if suffix.strip().lower().startswith("sym"):
            raise ValueError("cube3 pattern database %r: the suffix is %s or %s:N with N in 1..%d, once" % (spec, SYM_SUFFIX, SYM_SUFFIX, SYM_ALL))
        parse_cube3_pdb_spec(spec)  # raises, in the parser's words: cube3 has no other suffix
        raise ValueError("cube3 pattern database %r: the only suffix is %s or %s:N" % (spec, SYM_SUFFIX, SYM_SUFFIX))
    sym = SYM_ALL if m.group(1) is None else int(m.group(1))
    if sym == 0:
        raise ValueError("cube3 pattern database %r: +sym:N takes N in 1..%d images of each pattern, not 0" % (spec, SYM_ALL))
    return base.strip(), check_sym(sym)


def split_suffixes(spec: str) -> Tuple[str, int, bool]:
    """A spec string -> (the spec parse_cube3_pdb_spec takes, N as split_sym gives it, whether +dual was there).  The suffixes
    are +sym[:N] and +dual, in either order, each at most once; what is left without +dual goes through split_sym, which words
    every other refusal."""
    base, *suffixes = str(spec).strip().split("+")
    named = [t.strip().lower() for t in suffixes]
    for t in named:
        if t.startswith(DUAL_SUFFIX[1:]) and t != DUAL_SUFFIX[1:]:
            raise ValueError("cube3 pattern database %r: %s takes no argument and no other spelling" % (spec, DUAL_SUFFIX))
    if named.count(DUAL_SUFFIX[1:]) > 1:
        raise ValueError("cube3 pattern database %r: the suffix %s, once" % (spec, DUAL_SUFFIX))
    dual = DUAL_SUFFIX[1:] in named
    rest = "+".join([base] + [t for t, name in zip(suffixes, named) if name != DUAL_SUFFIX[1:]])
    return split_sym(rest) + (dual,)


def check_sym(sym) -> int:
    sym = int(sym or 0)
    if not 0 <= sym <= SYM_ALL:
        raise ValueError("+sym:N takes N in 1..%d images of each pattern, not %d" % (SYM_ALL, sym))
    return sym


def sym_suffix(sym: int, dual: bool = False) -> str:
    """The canonical suffix: +sym or +sym:N where there is one, then +dual."""
    return ("" if not sym else SYM_SUFFIX if sym == SYM_ALL else "%s:%d" % (SYM_SUFFIX, sym)) + (DUAL_SUFFIX if dual else "")


def sym_lookups(patterns: PatternSet, sym: int) -> int:
    """Look-ups of a pattern set under +sym:N: per pattern min(N, its distinct images), as the library counts them (no device)."""
    return sum(len(_lib.cube3_sym_images(kind, g, sym)[0]) for kind, g in patterns)


def check_sym_lookups(patterns: PatternSet, sym: int) -> None:
    n = sym_lookups(patterns, sym) if sym else 0
    if n > _lib.CUBE3_SYM_MAX_LOOKUPS:
        raise ValueError("cube3 pattern database %s%s: %d look-ups, over the cap of %d: take fewer images of each pattern with %s:N"
                         % (spec_of(patterns), sym_suffix(sym), n, _lib.CUBE3_SYM_MAX_LOOKUPS, SYM_SUFFIX))


def pattern_bytes(kind: int, k: int) -> int:
    n, o = _lib.CUBE3_PDB_SLOTS[kind]
    return perm(n, k) * o ** k


def spec_of(patterns: PatternSet) -> str:
    return "/".join(",".join("%s%d" % (_PREFIX[kind], c) for c in g) for kind, g in patterns)


def check_patterns(patterns) -> PatternSet:
    patterns = tuple((int(kind), tuple(int(c) for c in g)) for kind, g in patterns)
    if not 1 <= len(patterns) <= _lib.PDB_MAX_PATTERNS:
        raise ValueError("a pattern database has 1..%d patterns, not %d" % (_lib.PDB_MAX_PATTERNS, len(patterns)))
    for kind, group in patterns:
        if kind not in _lib.CUBE3_PDB_SLOTS:
            raise ValueError("a pattern's kind is 0 (corners) or 1 (edges), not %r" % (kind,))
        n, _ = _lib.CUBE3_PDB_SLOTS[kind]
        if not 1 <= len(group) <= MAX_K:
            raise ValueError("a pattern has 1..%d cubies, not %d" % (MAX_K, len(group)))
        for c in group:
            if not 0 <= c < n:
                raise ValueError("cubie %s%d is out of range: cube3 has %s0..%s%d" % (_PREFIX[kind], c, _PREFIX[kind], _PREFIX[kind], n - 1))
        if len(set(group)) != len(group):
            raise ValueError("a cubie is named twice in the pattern %s" % spec_of(((kind, group),)))
        if pattern_bytes(kind, len(group)) > MAX_TABLE_BYTES:
            raise ValueError("the pattern %s needs a table of %d bytes: over the cap of 2^34"
                             % (spec_of(((kind, group),)), pattern_bytes(kind, len(group))))
    return patterns


def parse_cube3_pdb_spec(spec: str) -> PatternSet:
    """`spec`: a preset ("corners", "korf", "korf7") or explicit groups such as "c0,c1,c2/e0,e1,e2,e3" (cubies separated by
    commas, patterns by slashes; c = corner 0..7, e = edge 0..11, numbered as dca_cube3_pdb_cubies lists them).  ValueError,
    with no device needed, for: an unknown name (cube3 has no "auto"), bare numbers, corners and edges in one group, a cubie
    twice in one group, more than 8 cubies in a group, a table over the size cap, more than 24 groups."""
    spec = str(spec).strip()
    if "+" in spec:
        raise ValueError("cube3 pattern database %r: a suffix such as +reflect is defined for the sliding puzzles only" % spec)
    if spec.lower() in PRESETS:
        return PRESETS[spec.lower()]
    if not re.fullmatch(r"[ce\d,/\s]+", spec) or not re.search(r"\d", spec):
        raise ValueError("unknown cube3 pattern database %r (presets: %s; or explicit groups such as c0,c1,c2/e0,e1,e2,e3)"
                         % (spec, ", ".join(sorted(PRESETS))))
    patterns = []
    for group in spec.split("/"):
        names = [t.strip() for t in group.split(",")]
        if not all(re.fullmatch(r"[ce]\d+", t) for t in names):
            raise ValueError("pattern group %r: cubies are written c0..c7 / e0..e11, separated by ',', patterns by '/'" % group)
        if len({t[0] for t in names}) != 1:
            raise ValueError("pattern group %r mixes corners and edges: a pattern is of one kind" % group)
        patterns.append((_C if names[0][0] == "c" else _E, tuple(int(t[1:]) for t in names)))
    return check_patterns(patterns)


def table_bytes(patterns: PatternSet) -> List[int]:
    return [pattern_bytes(kind, len(g)) for kind, g in patterns]


class Cube3PatternDatabase(_TableSet):
    """The tables of one cube3 pattern set, combined by max; the engine's closure reads the network-input colour rows."""

    env_name = "cube3"
    _engine_rows = "network-input"

    def __init__(self, patterns, sym: int = 0, dual: bool = False):
        super().__init__()
        sym = check_sym(sym)
        if isinstance(patterns, str):
            patterns, suffix, named = split_suffixes(patterns)
            self.patterns = parse_cube3_pdb_spec(patterns)
            sym = suffix or sym
            dual = bool(dual) or named
        else:
            self.patterns = check_patterns(patterns)
        self.sym = sym  # 0: plain; N: the first N images of each pattern (48: all)
        self.dual = bool(dual)  # every look-up read again at the inverse state
        check_sym_lookups(self.patterns, self.sym)

    @property
    def spec(self) -> str:
        return spec_of(self.patterns) + sym_suffix(self.sym, self.dual)

    def _table_bytes(self) -> List[int]:
        return table_bytes(self.patterns)

    def _build_one(self, i: int):
        return _lib.cube3_pdb_build(*self.patterns[i])

    def heuristic(self, states: torch.Tensor, row_kind: int = _lib.ROWS_STATE) -> torch.Tensor:
        self._ready("build() or load() first")
        return _lib.cube3_pdb_eval(states, row_kind, self.patterns, self.tables, sym=self.sym, dual=self.dual)

    def _engine_heuristic(self, states: torch.Tensor) -> torch.Tensor:
        return self.heuristic(states, _lib.ROWS_NNET)  # BwasEngine.step / solve hand a cube3 closure the rows sticker // 9

    @classmethod
    def _from_header(cls, path: str, env_name: str, spec: str):
        if env_name != cls.env_name:
            raise ValueError("%s holds tables of %s, not of cube3" % (path, env_name))
        return cls(spec)
