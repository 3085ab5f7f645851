"""Additive disjoint pattern databases for the sliding puzzles (include/dca.h "pattern databases", csrc/dca_pdb.hip): an exact
admissible, consistent heuristic — the baseline the DeepCubeA paper measures its learned heuristic against.  With
`--model_dir pdb:<spec> --weight 1 --semantics cpp` the engine is an optimal solver.  `<spec>+reflect` reads the same tables at
the state and at its mirror image in the main diagonal and takes the larger value (Korf & Felner's reflected look-up).

A partition is a tuple of patterns, a pattern a tuple of tiles; `parse_pdb_spec` turns a preset name or explicit groups
("1,2,3,4/5,6,7,8") into one and refuses what cannot be built, before any device work."""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

Partition = Tuple[Tuple[int, ...], ...]

# presets: settings, each covering every tile of its board exactly once (tests check that)
PRESETS: Dict[str, Dict[str, Partition]] = {
    "puzzle8": {"4-4": ((1, 2, 3, 4), (5, 6, 7, 8))},
    "puzzle15": {"5-5-5": ((1, 2, 3, 5, 6), (4, 7, 8, 11, 12), (9, 10, 13, 14, 15)),
                 "6-6-3": ((1, 5, 6, 9, 10, 13), (7, 8, 11, 12, 14, 15), (2, 3, 4))},
    "puzzle24": {"6-6-6-6": ((1, 2, 3, 6, 7, 8), (4, 5, 9, 10, 14, 15), (11, 12, 16, 17, 21, 22), (13, 18, 19, 20, 23, 24))},
}
AUTO = {"puzzle8": "4-4", "puzzle15": "5-5-5", "puzzle24": "6-6-6-6"}  # puzzle35 / puzzle48: explicit groups only
MAX_TABLE_BYTES = 1 << 34  # one pattern's table (the library's own limit)
REFLECT_SUFFIX = "+reflect"  # a spec that ends in it asks for the reflected look-up (include/dca.h); the tables are the same


def split_reflect(spec: str) -> Tuple[str, bool]:
    """A spec string -> (the spec parse_pdb_spec takes, whether it ended in "+reflect").  ValueError for any other use of '+'."""
    spec = str(spec).strip()
    base, plus, suffix = spec.partition("+")
    if not plus:
        return spec, False
    if "+" + suffix.strip().lower() != REFLECT_SUFFIX:
        raise ValueError("pattern database %r: the only suffix is %s, once" % (spec, REFLECT_SUFFIX))
    return base.strip(), True


def puzzle_dim(env_name: str) -> int:
    """Board side of a sliding-puzzle environment name; ValueError for anything else."""
    m = re.fullmatch(r"puzzle(\d+)", str(env_name).lower())
    if not m:
        raise ValueError("pattern databases are defined for the sliding puzzles only, not for %r" % (env_name,))
    env, dim = _lib.env_ids(env_name)[:2]
    assert env == _lib.ENV_NPUZZLE
    return dim


def parse_pdb_spec(env_name: str, spec: str) -> Partition:
    """`spec`: a preset name of this board ("4-4", "5-5-5", "6-6-3", "6-6-6-6"), "auto", or explicit groups such as
    "1,2,3,4/5,6,7,8" (tiles separated by commas, patterns by slashes; tiles may be left out).  ValueError, with no device
    needed, for: an environment that is no sliding puzzle, an unknown preset, tiles outside 1..N-1 or named twice, more than
    24 patterns, a pattern whose table N^(k+1) is over the size cap."""
    dim = puzzle_dim(env_name)
    N = dim * dim
    name = str(env_name).lower()
    spec = str(spec).strip()
    if spec.lower() == "auto":
        if name not in AUTO:
            raise ValueError("pdb:auto has no preset for %s: name the groups, e.g. pdb:1,2,3/4,5,6" % env_name)
        spec = AUTO[name]
    if spec in PRESETS.get(name, {}):
        partition = PRESETS[name][spec]
    elif re.fullmatch(r"[\d,/\s]+", spec) and re.search(r"\d", spec):
        try:
            partition = tuple(tuple(int(t) for t in group.split(",")) for group in spec.split("/"))
        except ValueError:
            raise ValueError("pattern groups %r: tiles are separated by ',' and patterns by '/'" % spec) from None
    else:
        raise ValueError("unknown pattern database %r for %s (presets: %s; or explicit groups such as 1,2,3/4,5,6)"
                         % (spec, env_name, ", ".join(sorted(PRESETS.get(name, {}))) or "none"))
    return check_partition(dim, partition)


def check_partition(dim: int, partition: Sequence[Sequence[int]]) -> Partition:
    N = dim * dim
    partition = tuple(tuple(int(t) for t in g) for g in partition)
    if not 1 <= len(partition) <= _lib.PDB_MAX_PATTERNS:
        raise ValueError("a pattern database has 1..%d patterns, not %d" % (_lib.PDB_MAX_PATTERNS, len(partition)))
    seen = set()
    for group in partition:
        if not group:
            raise ValueError("a pattern needs at least one tile")
        for t in group:
            if not 1 <= t <= N - 1:
                raise ValueError("tile %d is out of range: a %d x %d board has tiles 1..%d" % (t, dim, dim, N - 1))
            if t in seen:
                raise ValueError("tile %d is named twice: the patterns must be disjoint" % t)
            seen.add(t)
        if N ** (len(group) + 1) > MAX_TABLE_BYTES:
            raise ValueError("a %d-tile pattern of a %d x %d board needs a table of %d^%d bytes: over the cap of 2^34"
                             % (len(group), dim, dim, N, len(group) + 1))
    return partition


def table_bytes(dim: int, partition: Partition) -> List[int]:
    return [(dim * dim) ** (len(g) + 1) for g in partition]


class _TableSet:
    """What the pattern databases of every family share (PatternDatabase below, cube3_pdb.Cube3PatternDatabase): the tables of
    one pattern set on the current device.  build() fills them one pattern after another; save() / load() keep them in an .npz;
    heuristic_fn_dev() is the closure BwasEngine.step calls.  A family supplies env_name, spec (the string save() writes),
    _table_bytes(), _build_one(i), _engine_heuristic(rows), _engine_rows and _from_header(path, env_name, spec)."""

    def __init__(self):
        self.tables: List[torch.Tensor] = []
        self.sweeps: List[int] = []

    @property
    def bytes(self) -> int:
        return sum(self._table_bytes())

    def build(self):
        _lib.require_gpu()
        self.tables, self.sweeps = [], []
        for i in range(len(self._table_bytes())):
            table, sweeps = self._build_one(i)
            self.tables.append(table)
            self.sweeps.append(sweeps)
        return self

    def set_tables(self, tables: Sequence[np.ndarray]):
        """Adopt host-made tables (one uint8 array per pattern, of the pattern's table size)."""
        want = self._table_bytes()
        if len(tables) != len(want):
            raise ValueError("%d tables for %d patterns" % (len(tables), len(want)))
        host = [np.ascontiguousarray(t, dtype=np.uint8).reshape(-1) for t in tables]
        for t, b in zip(host, want):
            if t.size != b:
                raise ValueError("a table of %d bytes where the pattern needs %d" % (t.size, b))
        dev = _lib.require_gpu()
        self.tables = [torch.from_numpy(t if t.flags.writeable else t.copy()).to(dev) for t in host]
        self.sweeps = [0] * len(host)
        return self

    def _ready(self, otherwise: str) -> None:
        if len(self.tables) != len(self._table_bytes()):
            raise _lib.DcaError("%s: %s" % (type(self).__name__, otherwise))

    def heuristic_fn_dev(self):
        """(uint8 rows on the device, is_onehot=False) -> float32 [m]: the closure form of BwasEngine.step / solve."""
        def fn(states: torch.Tensor, is_onehot: bool = False) -> torch.Tensor:
            if is_onehot:
                raise ValueError("a pattern database reads the uint8 %s rows, not one-hot rows" % self._engine_rows)
            return self._engine_heuristic(states)
        return fn

    def save(self, path: str, tables: Optional[Sequence[np.ndarray]] = None) -> None:
        """Write the pattern set and the tables to an .npz (`tables`: host arrays to write instead of the device's)."""
        if tables is None:
            self._ready("nothing to save, build() first")
            tables = [t.cpu().numpy() for t in self.tables]
        want = self._table_bytes()
        if [int(np.asarray(t).size) for t in tables] != want:
            raise ValueError("table sizes %s, the pattern set needs %s" % ([int(np.asarray(t).size) for t in tables], want))
        arrays = {"table_%d" % i: np.ascontiguousarray(t, dtype=np.uint8).reshape(-1) for i, t in enumerate(tables)}
        arrays["env_name"] = np.array(self.env_name)
        arrays["partition"] = np.array(self.spec)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load_host(cls, path: str):
        """-> (the database without device tables, [host tables]); needs no device."""
        with np.load(path) as z:
            pdb = cls._from_header(path, str(z["env_name"]), str(z["partition"]))
            tables = [z["table_%d" % i] for i in range(len(pdb._table_bytes()))]
        if [int(t.size) for t in tables] != pdb._table_bytes():
            raise ValueError("%s: table sizes do not match the pattern set" % path)
        return pdb, tables

    @classmethod
    def load(cls, path: str):
        pdb, tables = cls.load_host(path)
        return pdb.set_tables(tables)


class PatternDatabase(_TableSet):
    """The additive tables of one partition of a sliding puzzle (a 6-6-6-6 set, once saved, need not be rebuilt)."""

    _engine_rows = "state"

    def __init__(self, env_name: str, partition, reflect: bool = False):
        super().__init__()
        self.env_name = str(env_name).lower()
        self.dim = puzzle_dim(env_name)
        if isinstance(partition, str):
            partition, suffix = split_reflect(partition)
            self.partition = parse_pdb_spec(env_name, partition)
            reflect = bool(reflect) or suffix
        else:
            self.partition = check_partition(self.dim, partition)
        self.reflect = bool(reflect)

    @property
    def spec(self) -> str:
        return "/".join(",".join(str(t) for t in g) for g in self.partition) + (REFLECT_SUFFIX if self.reflect else "")

    def _table_bytes(self) -> List[int]:
        return table_bytes(self.dim, self.partition)

    def _build_one(self, i: int):
        return _lib.pdb_build(self.dim, self.partition[i])

    def heuristic(self, states: torch.Tensor) -> torch.Tensor:
        self._ready("build() or load() first")
        return _lib.pdb_eval(self.dim, states, self.partition, self.tables, reflect=self.reflect)

    _engine_heuristic = heuristic  # the engine hands the closure the state rows [m, D]

    @classmethod
    def _from_header(cls, path: str, env_name: str, spec: str):
        return cls(env_name, spec)  # (a file of another family: no sliding puzzle, ValueError)
