"""Inputs of the topology tests (checker plumbing, CPU only): index tensors from the host builder (torch_m3gnet.data.neighbors), one per
regime of csrc/m3g_topology.hip, each named for the regime it is there for.

tests/test_topology_cpu.py asserts from the restatement (tests/topology_reference.py) that each regime is reached;
tests/test_gpu_topology.py runs every case through every entry point of the build.  `case(name)` builds a case once and
`reference(name)` restates it once; neither result is ever modified."""
from __future__ import annotations

import functools
import importlib.util
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import topology_reference as tr

kInStage = 512   # longest row the mirror search of the incoming-edge lists stages (k_in_edges_symmetric); longer rows: the sort


@dataclass(frozen=True)
class Case:
    name: str
    regime: str
    N: int
    S: int
    edge_index: np.ndarray           # [2, E] int64
    triplet_edge_index: np.ndarray   # [2, T] int64
    batch: np.ndarray                # [N] int64
    canonical: bool                  # the lists are as this library's builders write them: the canonical entry points are admitted

    @property
    def E(self):
        return self.edge_index.shape[1]

    @property
    def T(self):
        return self.triplet_edge_index.shape[1]

    # ---- which branch of the build the lists take, from the lists alone
    @property
    def triplets_sorted(self):
        t = self.triplet_edge_index
        key = (t[0].astype(np.uint64) << np.uint64(32)) | t[1].astype(np.uint64)
        return bool(np.all(key[1:] >= key[:-1]))

    @property
    def triplets_symmetric(self):
        t = self.triplet_edge_index
        fwd = np.sort((t[0].astype(np.uint64) << np.uint64(32)) | t[1].astype(np.uint64))
        rev = np.sort((t[1].astype(np.uint64) << np.uint64(32)) | t[0].astype(np.uint64))
        return bool(np.array_equal(fwd, rev))   # every (e1, e2) has its (e2, e1), with multiplicity

    @property
    def edges_symmetric(self):
        """Every i -> j has its j -> i, with multiplicity."""
        e = self.edge_index
        fwd = np.sort((e[0].astype(np.uint64) << np.uint64(32)) | e[1].astype(np.uint64))
        rev = np.sort((e[1].astype(np.uint64) << np.uint64(32)) | e[0].astype(np.uint64))
        return bool(np.array_equal(fwd, rev))

    @property
    def longest_row(self):
        return int(np.bincount(self.edge_index[0], minlength=max(self.N, 1)).max()) if self.E else 0

    @property
    def mirrors_apply(self):
        """The incoming-edge lists come from the mirror search (no sort)."""
        return self.E > 0 and self.T > 0 and self.edges_symmetric and self.longest_row <= kInStage

    @property
    def branch(self):
        """The branch of the general build the lists take."""
        if self.T == 0:
            return "no triplets"
        if not self.triplets_sorted:
            return "sorted again" if self.triplets_symmetric else "sorted again, one-sided second sort"
        if not self.triplets_symmetric:
            return "one-sided second sort"
        return "optimistic" if self.mirrors_apply else "in-edge sort fallback"

    @property
    def fast_build_applies(self):
        """m3g_topology_build_canonical takes its six-launch build (m3g_topology_debug_last_path == 1)."""
        return self.canonical and self.N > 0 and self.E > 0 and self.T > 0 and self.mirrors_apply


# ------------------------------------------------------------------ the host builder
def host_lists(lattices, positions, cutoff, tb_cutoff):
    """(N, S, edge_index, triplet_edge_index, batch) of a batch of cells, one structure at a time with the batch offsets."""
    from torch_m3gnet.data.neighbors import neighbor_list, threebody_index

    eis, teis, n0, e0 = [], [], 0, 0
    for lat, pos in zip(lattices, positions):
        ei, _, d = neighbor_list(lat, pos, cutoff)
        tei, _, _ = threebody_index(len(pos), ei, d.astype(np.float32), tb_cutoff)
        eis.append(ei + n0)
        teis.append(tei + e0)
        n0 += len(pos)
        e0 += ei.shape[1]
    batch = np.repeat(np.arange(len(positions)), [len(p) for p in positions]).astype(np.int64)
    return n0, len(positions), np.concatenate(eis, axis=1), np.concatenate(teis, axis=1), batch


def _from_batch(g):
    from torch_m3gnet.data import MaterialGraphKey as K

    return (int(g[K.BATCH].numel()), int(g[K.LATTICE].size(0)), g[K.EDGE_INDEX].numpy().astype(np.int64),
            g[K.TRIPLET_EDGE_INDEX].numpy().astype(np.int64), g[K.BATCH].numpy().astype(np.int64))


def _fcc(nx, ny, nz):
    from torch_m3gnet.data.synthetic import fcc_cu_arrays

    lat, pos, _ = fcc_cu_arrays(nx, ny, nz, a=3.61, jitter=0.02)
    return host_lists([lat], [pos], 5.0, 4.0)


def _uniform(n, box, cutoff, tb_cutoff, seed):
    pos = np.random.default_rng(seed).uniform(0, box, (n, 3))
    return host_lists([np.eye(3) * box], [pos], cutoff, tb_cutoff)


def _random_cells(spec, cutoff, tb_cutoff):
    from torch_m3gnet.data.synthetic import random_cell_arrays

    cells = [random_cell_arrays(*s) for s in spec]
    return host_lists([c[0] for c in cells], [c[1] for c in cells], cutoff, tb_cutoff)


STAGED_WINDOW_CELL = dict(n_atoms=24, box=6.5, seed=1, cutoff=8.0, tb_cutoff=5.2)   # windows of 193..255 rows, T <= 24 E (found by search)


def _staged_window():
    c = STAGED_WINDOW_CELL
    return _random_cells([(c["n_atoms"], c["box"], c["seed"])], c["cutoff"], c["tb_cutoff"])


def _seven_atoms(cutoff, tb_cutoff):
    """The 7-atom cell of tests/test_gpu_graph_build.py: rows of ~150 edges at 5.5 A, ~590 at 9 A."""
    rng = np.random.default_rng(17)
    lat = np.array([[3.3, 0.2, 0.0], [-0.3, 3.4, 0.1], [0.2, -0.1, 3.2]])
    frac = rng.uniform(0, 1, (7, 3))
    return host_lists([lat], [frac @ lat], cutoff, tb_cutoff)


def _idle_atoms():
    """Structures without triplets beside structures with them, and -- in the second structure -- atoms without an active edge at the
    start, in the middle and at the end of a structure whose other atoms have some: three lone atoms of a 24 A cell around two
    clusters of six."""
    from torch_m3gnet.data.synthetic import random_cell_arrays

    sparse = [random_cell_arrays(3, 9.0, 70 + s) for s in range(3)]
    cluster = random_cell_arrays(12, 5.0, 3)[1]
    lone = np.array([[12.0, 12.0, 12.0], [19.0, 6.0, 18.0], [6.0, 19.0, 12.0]])
    pos = np.concatenate([lone[:1], cluster[:6], lone[1:2], cluster[6:], lone[2:]])
    dense = random_cell_arrays(30, 7.5, 80)
    lats = [sparse[0][0], np.eye(3) * 24.0, sparse[1][0], dense[0], sparse[2][0]]
    poss = [sparse[0][1], pos, sparse[1][1], dense[1], sparse[2][1]]
    return host_lists(lats, poss, 5.0, 3.0)


def _empty():
    return host_lists([np.eye(3) * 30.0], [np.array([[1.0, 1.0, 1.0], [15.0, 15.0, 15.0]])], 5.0, 4.0)


def _dimer():
    return host_lists([np.eye(3) * 30.0], [np.array([[1.0, 1.0, 1.0], [3.0, 1.0, 1.0]])], 5.0, 4.0)


def _one_atom():
    return _random_cells([(1, 3.0, 5)], 5.0, 4.0)


# ------------------------------------------------------------------ lists that are not canonical
def _with_triplets(lists, tei):
    N, S, ei, _, batch = lists
    return N, S, ei, np.ascontiguousarray(tei), batch


def _two_cells():
    return _random_cells([(20, 6.5, 7), (20, 6.5, 8)], 5.0, 4.0)


def _shuffled(lists, seed=0):
    tei = lists[3]
    return _with_triplets(lists, tei[:, np.random.default_rng(seed).permutation(tei.shape[1])])


def _one_sided(lists):
    tei = lists[3]
    return _with_triplets(lists, tei[:, tei[0] < tei[1]])


def _thinned(lists, keep=0.5, seed=0):
    tei = lists[3]
    return _with_triplets(lists, tei[:, np.random.default_rng(seed).random(tei.shape[1]) < keep])


def _pair_twice(lists):
    tei = lists[3]
    k = tei.shape[1] // 2
    return _with_triplets(lists, np.concatenate([tei[:, : k + 1], tei[:, k:]], axis=1))   # pair k twice, the list still sorted


def _unsorted_batch(lists, seed=0):
    N, S, ei, tei, batch = lists
    return N, S, ei, tei, batch[np.random.default_rng(seed).permutation(N)]


def _variant(which, key):
    import reverse_term_cases as rc

    return _from_batch({"triplets": rc.triplet_list_variants, "edges": rc.edge_list_variants}[which]()[key])


def _dense_cell():
    import reverse_term_cases as rc

    return _from_batch(rc.dense_batch())


# ------------------------------------------------------------------ random batches
PERTURBATIONS = ("none", "shuffle", "one-sided", "thinned")
N_RANDOM = 20


def _fuzz_module():
    path = Path(__file__).resolve().parent / "checkers" / "fuzz_graph_build.py"
    spec = importlib.util.spec_from_file_location("fuzz_graph_build", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _random_batch(seed):
    """A batch of tests/checkers/fuzz_graph_build.random_cell cells under that checker's cutoffs (draws beyond 200,000 triplets or
    without an edge are drawn again), its triplet list perturbed as the seed says."""
    random_cell = _fuzz_module().random_cell
    rng = np.random.default_rng(1000 + seed)
    while True:
        cutoff = float(rng.uniform(2.5, 9.0))
        tb = float(rng.uniform(0.5, 1.0) * cutoff) if rng.random() < 0.8 else cutoff
        cells = [random_cell(rng) for _ in range(int(rng.integers(1, 7)))]
        if min(abs(np.linalg.det(l)) for l, _ in cells) < 4.0:
            continue
        # (a bound on the triplets before they are formed: neighbours inside the three-body cutoff from the density)
        est = sum(len(p) * (len(p) / abs(np.linalg.det(l)) * 4.19 * tb**3) ** 2 for l, p in cells)
        if est > 400_000:
            continue
        lists = host_lists([l for l, _ in cells], [p for _, p in cells], cutoff, tb)
        if lists[2].shape[1] > 0 and lists[3].shape[1] <= 200_000:
            break
    which = PERTURBATIONS[seed % len(PERTURBATIONS)]
    if which == "shuffle":
        lists = _shuffled(lists, seed)
    elif which == "one-sided":
        lists = _one_sided(lists)
    elif which == "thinned":
        lists = _thinned(lists, 0.5, seed)
    return lists


# name -> (regime, builder, canonical)
CASES = {
    "fcc 1x1x1": ("one window, part-filled", lambda: _fcc(1, 1, 1), True),
    "fcc 2x2x4": ("A an exact multiple of 128: the record after the last window has 128 b == A", lambda: _fcc(2, 2, 4), True),
    "fcc 4x4x4": ("many windows, E and T beyond one scan tile and one sort chunk", lambda: _fcc(4, 4, 4), True),
    "400 atoms in 30 A": ("a window spans more than 64 atoms: not fast, hints word 0", lambda: _uniform(400, 30.0, 5.0, 2.6, 1), True),
    "300 atoms in 24 A": ("a window spans exactly 64 atoms: fast", lambda: _uniform(300, 24.0, 5.0, 3.0, 2), True),
    "150 atoms in 10 A": ("windows above 255 rows: bytes 255, not fast", lambda: _uniform(150, 10.0, 5.5, 5.5, 8), True),
    "24 atoms in 6.5 A": ("windows of 193..255 rows under the short lists (T <= 24 E)", _staged_window, True),
    "idle atoms": ("atoms without an active edge at the start, middle and end of a structure; structures without triplets", _idle_atoms, True),
    "7 atoms, rows of ~150": ("rows of several 64-lane passes", lambda: _seven_atoms(5.5, 4.0), True),
    "7 atoms, rows of ~590": ("rows beyond the mirror search's stage: the in-edge sort fallback", lambda: _seven_atoms(9.0, 3.0), True),
    "no edges": ("E = 0", _empty, True),
    "dimer": ("T = 0 with E > 0", _dimer, True),
    "one atom": ("one atom, self images only", _one_atom, True),
    "triplets shuffled": ("sorted again", lambda: _shuffled(_two_cells()), False),
    "triplets one-sided": ("one-sided second sort", lambda: _variant("triplets", "one_sided"), False),
    "triplets thinned": ("incomplete rows", lambda: _variant("triplets", "thinned"), False),
    "single pair": ("one triplet: one active pair of edges", lambda: _variant("triplets", "single_pair"), False),
    "one pair twice": ("duplicate pairs are kept", lambda: _pair_twice(_two_cells()), False),
    "shuffled and one-sided": ("sorted again, then the one-sided second sort", lambda: _shuffled(_one_sided(_two_cells())), False),
    "asymmetric edge list": ("in-edge sort fallback on a one-sided edge list", lambda: _variant("edges", ("thinned", "asymmetric")), False),
    "multigraph": ("several images of the same neighbour", lambda: _variant("edges", ("multigraph", "symmetric")), False),
    "dense cell": ("~100 partners per centre", _dense_cell, False),
    "unsorted batch": ("flags[3]: struct_ptr unspecified", lambda: _unsorted_batch(_two_cells()), False),
}
for _s in range(N_RANDOM):
    CASES[f"random batch {_s}"] = (f"random cells, triplet list: {PERTURBATIONS[_s % len(PERTURBATIONS)]}",
                                   functools.partial(_random_batch, _s), _s % len(PERTURBATIONS) == 0)
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    regime, builder, canonical = CASES[name]
    N, S, ei, tei, batch = builder()
    for a in (ei, tei, batch):
        a.setflags(write=False)
    return Case(name, regime, int(N), int(S), ei, tei, batch, canonical)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    c = case(name)
    return tr.restate(c.N, c.S, c.edge_index, c.triplet_edge_index, c.batch)


def window_rows(ref: dict) -> np.ndarray:
    """hi - lo of every window that holds rows."""
    w = ref["tb_win"].reshape(-1, 6)
    n = (ref["A"] + tr.kTbRows - 1) // tr.kTbRows
    return (w[:n, 1] - w[:n, 0]).astype(np.int64)


def window_atoms(ref: dict) -> np.ndarray:
    """Centre atoms spanned by every window that holds rows."""
    w = ref["tb_win"].reshape(-1, 6)
    n = (ref["A"] + tr.kTbRows - 1) // tr.kTbRows
    src, act = ref["src"], ref["act_list"]
    return np.array([int(src[act[w[b, 1] - 1]]) - int(src[act[w[b, 0]]]) + 1 for b in range(n)], dtype=np.int64)
