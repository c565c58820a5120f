"""Shared test plumbing: fixtures -> oracle inputs and -> engine (torch_m3gnet) inputs."""
from __future__ import annotations

from collections import Counter
from pathlib import Path

import numpy as np
import torch

from oracle import m3gnet_oracle as orc

GOLDEN = Path(__file__).resolve().parent / "golden"
CASE_MODEL = {"cu32": "model_default_seed0", "tio": "model_default_seed0", "alna": "model_small_seed0", "mix": "model_mix_seed3",
              # round 3: sheared / rotated / left-handed triclinic cell with atoms outside the home cell; the default model FITTED
              # (reference nn code, Adam) to Lennard-Jones energies and forces: |F| ~ 1 eV/A, activations no longer near-linear
              "tri": "model_default_seed0", "cu32fit": "model_fitted_lj", "mixfit": "model_fitted_lj",
              "cu32pair": "model_default_seed0"}   # (doc mode only: a triplet list of one pair)
CASES = [(c, m) for c in CASE_MODEL for m in ("ref", "doc") if c != "cu32pair"]
FITTED_CASES = [(c, m) for c, m in CASES if c.endswith("fit")]


def load_oracle_case(case: str, mode: str, dtype=torch.float32):
    params, cfg, elemental = orc.load_model_npz(GOLDEN / f"{CASE_MODEL[case]}.npz", dtype=dtype)
    graph, expect = orc.load_case_npz(GOLDEN / f"case_{case}_{mode}.npz")
    consts = orc.make_constants(cfg, elemental, dtype=dtype)
    consts.factors = expect["const_factors"].to(dtype)  # captured constant (SURVEY finding 1)
    return params, cfg, consts, graph, expect


def build_engine_model(case: str, mode: str, device="cuda"):
    """torch_m3gnet (the product) model with the fixture's weights and captured constants."""
    from torch_m3gnet.model.build import build_model

    params, cfg, elemental = orc.load_model_npz(GOLDEN / f"{CASE_MODEL[case]}.npz")
    _, expect = orc.load_case_npz(GOLDEN / f"case_{case}_{mode}.npz")
    model = build_model(cfg.cutoff, cfg.threebody_cutoff, cfg.l_max, cfg.n_max, cfg.num_types, cfg.embedding_dim,
                        cfg.num_blocks, elemental_energies=elemental, energy_scale=cfg.energy_scale,
                        length_scale=cfg.length_scale)
    model.load_state_dict({k: v for k, v in params.items()})
    for mod in model.model:
        if type(mod).__name__ == "ThreeBodyInteration":
            mod.nsb.factors = expect["const_factors"].clone()
    return model, cfg


def engine_graph(graph: dict, device="cuda"):
    from torch_m3gnet.data.material_graph import Batch

    g = Batch.__new__(Batch)
    dict.__init__(g)
    for k, v in graph.items():
        g[k] = v.to(device)
    g["num_nodes"] = int(graph["pos"].size(0))
    return g


def preactivation_stats(params, cfg, consts, graph):
    """Pre-activation statistics of every 64-wide Linear of the gated MLPs, in call order, from one oracle evaluation (checker):
    per layer (in_features, mean |p|, share of |p| > 2, share of |p| > 4, max |p|).  Per conv block the order is edge MLP
    {dense.0, gate.0, dense.2, gate.2}, node MLP likewise; the readout's layers come last."""
    stats = []
    orig = torch.nn.functional.linear

    def spy(x, w, b=None):
        y = orig(x, w, b)
        if w.shape[0] == cfg.embedding_dim and w.shape[1] in (cfg.embedding_dim, 3 * cfg.embedding_dim):
            a = y.detach().abs().double()
            stats.append((int(w.shape[1]), float(a.mean()), float((a > 2).double().mean()), float((a > 4).double().mean()), float(a.max())))
        return y

    torch.nn.functional.linear = spy
    try:
        orc.energy_forces(params, cfg, consts, graph, want_forces=False)
    finally:
        torch.nn.functional.linear = orig
    return stats


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a-b| / max|b| (the metric SURVEY.md §8(d) prescribes for forces)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- the persistent (large-system) kernel selection, forced on inputs the default selection sends down the small-system path
# (resolve_step_path, csrc/m3g_step_path.h).  Order matters: setting small_tiles also moves small_tiles_fwd (option table of
# csrc/m3g_api.hip), so both edge kernels become the persistent ones; split_node_tiles = 0 selects k_node_pre_mfma<fp32> and
# k_readout_mfma<fp32>; split_tail = 0 keeps every tile in the whole-tile body of k_edge_rev_f32.
PERSISTENT = dict(small_tiles=0, split_node_tiles=0, split_tail=0)
PERSISTENT_TAIL = dict(PERSISTENT, split_tail=1)


def persistent_tile_counts(n_edges: int) -> Counter:
    """How many workgroups of a persistent edge kernel get how many 16-edge tiles: {tiles per workgroup: workgroups}.  A restatement
    of tiles_for, grid_for_tiles and the TileQueue constructor of csrc/m3g_edge_common.h (tests/test_step_path_cpu.py pins it to a table
    computed from that code)."""
    tiles = (n_edges + 15) // 16                       # tiles_for
    grid = min(max((tiles + 7) // 8 * 8, 8), 256)      # grid_for_tiles
    per_xcd, wgs = (tiles + 7) // 8, grid >> 3         # TileQueue: an eighth of the tiles per blockIdx % 8, equal chunks inside it
    chunk = (per_xcd + wgs - 1) // wgs
    counts = Counter()
    for block in range(grid):
        xcd, q = block & 7, block >> 3
        lo = xcd * per_xcd + q * chunk
        hi = min(lo + chunk, (xcd + 1) * per_xcd, tiles)
        counts[max(hi - lo, 0)] += 1
    return counts


def wave_takes_a_second_tile(counts: Counter) -> bool:
    """k_edge_rev_f32 runs 8 waves per workgroup: a wave comes round its loop again once a workgroup has more than 8 tiles."""
    return max(counts) > 8


def split_tail_runs(counts: Counter, split_tail: int = 1) -> bool:
    """Some workgroup's left-over tiles (count mod 4 in 1..split_tail) leave the queue for rev_split_run."""
    return any(1 <= count % 4 <= split_tail for count, workgroups in counts.items() if workgroups > 0)


def set_options(model, **options):
    for name, value in options.items():
        model.engine.set_option(name, value)
    return model


def record_line(name: str, line: str) -> None:
    """Measured margins kept with the run: printed, and appended to the file `name` in the directory that the environment variable
    M3G_MARGINS_DIR names, where it is set and exists (profiles/persistent_path_margins.txt is such a file)."""
    import os

    print(line)
    out_dir = os.environ.get("M3G_MARGINS_DIR", "")
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, name), "a") as fh:
            fh.write(line + "\n")


# workload builders live in the package (bench.py uses them without importing this module, which imports the oracle)
from torch_m3gnet.data.synthetic import fcc_cu_graph, random_cell_arrays, random_cell_graph  # noqa: E402,F401
