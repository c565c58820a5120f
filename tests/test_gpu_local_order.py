"""Local-order observables on the MI355X (torch_m3gnet.local_order, C ABI m3g_lo_*) against the numpy restatement
(tests/local_order_reference.py) over the batch of tests/local_order_cases.py: every continuous output within MARGIN = 8 times the
reference's own fp64 rounding (measured against its long-double evaluation, per quantity), every discrete output exactly, the ideal
lattices against their closed forms, bitwise reproducibility and independence of the batch and of its order, graph capture, the error
inputs (a NaN position, a singular cell, an r_cut beyond half the width, more than 32 neighbours), the series cap, the one-shot
`local_order`, and MolecularDynamics runs with all three observables and with local order alone under npt_mtk.

The measured deviations are in the docstring of test_outputs_match_the_reference and in profiles/local_order.txt."""
import functools

import numpy as np
import pytest
import torch

import local_order_cases as lc
import local_order_reference as ref
from helpers import record_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = "local_order.txt"
ACC_KEYS = ("hist_q", "hist_qbar", "hist_nb", "moments", "series_counts", "series_order", "n_samples", "n_skipped", "flags")
FRAME_KEYS = ("qlm", "ql", "qbar", "n_neighbors", "n_conn", "solid", "label")
ALL = list(range(len(lc.SIZES)))


def _state(order, r_cut=None):
    """A fresh LoState of the structures `order` of the batch; r_cut: {structure: another cut-off}."""
    from torch_m3gnet.local_order import LoState

    b = lc.batch()
    offsets = np.concatenate([[0], np.cumsum([lc.SIZES[s] for s in order])])
    cut = np.array([(r_cut or {}).get(s, lc.R_CUT[s]) for s in order])
    return LoState(int(offsets[-1]), offsets, np.concatenate([b["species"][s] for s in order]), cut, degrees=lc.DEGREES,
                   solid_degree=lc.SOLID[0], solid_threshold=lc.SOLID[1], solid_bonds=lc.SOLID[2], hist_bins=lc.BINS,
                   series_cap=lc.SERIES_CAP, max_species=lc.M, device=DEV)


def _accumulate(n_samples=lc.N_FRAMES, order=None, pos=None, lats=None, graph=False, take=None, r_cut=None):
    """Feed the first `n_samples` frames to a fresh LoState of the batch, or of the structures `order` in that order, reading the
    per-atom frame after every sample; pos: the frames to use; lats: a lattice array per sample; graph: through one captured
    lo_sample; take: f(tensor) -> the device tensor to use (guarded copies); r_cut: {structure: another cut-off}.  Returns
    {structure: its accumulators, and `frames`: one dict of per-atom arrays per sample}."""
    from torch_m3gnet.local_order import lo_sample

    b = lc.batch()
    off = b["offsets"]
    order = ALL if order is None else list(order)
    rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in order])
    st = _state(order, r_cut)
    take = (lambda x: x) if take is None else take
    pos = b["pos"] if pos is None else pos
    lat_of = lambda k: take(torch.tensor((b["lats"] if lats is None else lats[k])[order], dtype=torch.float64, device=DEV))
    data = [take(torch.tensor(pos[k][rows], device=DEV)) for k in range(n_samples)]
    frames = []
    lat = lat_of(0)
    if graph:
        p = torch.empty_like(data[0])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):   # one stream, no parallel branches; nothing executes here
            lo_sample(st, p, lat)
        for pk in data:
            p.copy_(pk)
            g.replay()
            frames.append(st.frame())
    else:
        for k, pk in enumerate(data):
            if lats is not None and k:
                lat = lat_of(k)
            lo_sample(st, pk, lat)
            frames.append(st.frame())
    torch.cuda.synchronize()
    out = st.read()
    per = {}
    for k, s in enumerate(order):
        lo, hi = st.offsets[k], st.offsets[k + 1]
        per[s] = {key: out[key][k] for key in ACC_KEYS}
        per[s]["frames"] = [{key: fr[key][lo:hi] for key in FRAME_KEYS} for fr in frames]
    per["state_bytes"] = st.state.numel()
    return per


@functools.lru_cache(maxsize=None)
def _full():
    """The five frames through the whole batch, kept: the bitwise tests compare against it."""
    return _accumulate()


def _same(a, b, keys=ACC_KEYS, frames=True):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True) and np.asarray(a[key]).dtype == np.asarray(b[key]).dtype, key
    if frames:
        assert len(a["frames"]) == len(b["frames"])
        for k, (fa, fb) in enumerate(zip(a["frames"], b["frames"])):
            for key in FRAME_KEYS:
                assert np.array_equal(fa[key], fb[key], equal_nan=True) and fa[key].dtype == fb[key].dtype, (k, key)


def test_outputs_match_the_reference():
    """Continuous outputs (the q_lm, q_l and qbar_l of every frame, the moment sums, the Q_l and mean-qbar series) against the
    long-double reference: the gate is MARGIN = 8 units of the fp64 reference's own deviation from it (tests/local_order_cases.py:
    chosen on the CPU, where another fp64 evaluation of the reference stays near 1 unit); discrete outputs (N_b, n_conn, solid,
    labels, n_solid, n_clusters, largest_cluster, every histogram, n_samples, n_skipped, flags) exactly.  Measured on the MI355X,
    deviation / unit:
      qlm 3.108, ql 3.144, qbar 2.716, moments 1.271, Q 1.830, mean_qbar 1.919
    (the units: qlm 1.5e-13, ql 1.1e-13, qbar 3.7e-14, moments 1.8e-15 per term, Q 1.7e-15, mean_qbar 1.6e-15 -- the per-atom ones are
    large because a bond of 2.5 A is the difference of two fp64 positions some 40 cells of up to 40 A away)."""
    assert lc.long_double_is_wider(), "np.longdouble is no wider than fp64 on this host: the tolerance would measure nothing"
    got = _full()
    hi = lc.reference("longdouble")
    for s, acc in enumerate(hi):
        g = got[s]
        assert g["n_samples"] == acc.n_samples and g["n_skipped"] == acc.n_skipped and g["flags"] == acc.flags == lc.FLAGGED.get(s, 0), s
        assert np.array_equal(g["hist_nb"], acc.hist_nb) and np.array_equal(g["series_counts"], acc.series_counts), s
        if s not in lc.IDEAL:   # (the values of an ideal lattice sit on a point, which may be an edge)
            assert np.array_equal(g["hist_q"], acc.hist_q) and np.array_equal(g["hist_qbar"], acc.hist_qbar), s
        assert g["hist_q"].sum() == g["hist_qbar"].sum() == acc.n_samples * lc.SIZES[s] * len(lc.DEGREES)
        for k, fr in enumerate(acc.frames):
            assert np.array_equal(g["frames"][k]["n_neighbors"], fr["n_neighbors"]), (s, k)
            if not fr["flags"]:
                for key in ("n_conn", "solid", "label"):
                    assert np.array_equal(g["frames"][k][key], fr[key]), (s, k, key)
    worst = {}
    for name in ("qlm", "ql", "qbar"):
        dev = max(lc.deviation(None, name, k, got={s: got[s]["frames"][k][name] for s in lc.CLEAN}) / lc.unit(name, k) for k in range(lc.N_FRAMES))
        worst[name] = dev
    worst["moments"] = lc.deviation(None, "moments", got={s: got[s]["moments"] for s in lc.CLEAN}) / lc.unit("moments")
    for at, name in enumerate(("Q", "mean_qbar")):
        worst[name] = lc.deviation(None, name, got={s: got[s]["series_order"][:, at] for s in lc.CLEAN}) / lc.unit(name)
    record_line(RECORD, f"deviation / unit (gate {lc.MARGIN:g}): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    record_line(RECORD, f"state of the test batch ({sum(lc.SIZES)} atoms, {len(lc.SIZES)} structures, 3 degrees, 20 bins, 3 series rows): "
                        f"{got['state_bytes']} B")
    for key, ratio in worst.items():
        assert ratio <= lc.MARGIN, (key, ratio)
    # a species a structure does not hold: exactly nothing
    assert (got[3]["moments"][2] == 0).all() and (got[3]["hist_q"][2] == 0).all() and (got[3]["hist_nb"][2] == 0).all()
    assert np.abs(got[2]["moments"]).min() > 0


def test_ideal_lattices_against_the_closed_forms():
    got = _full()
    closed = {"fcc": (np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0), 12), "sc": (np.sqrt(7.0 / 12.0), np.sqrt(1.0 / 8.0), 6),
              "hcp": (0.097222, 0.484762, 12), "bcc": (0.036370, 0.510688, 14)}
    for name, (q4, q6, nb) in closed.items():
        s = lc.NAMES.index(name)
        fr, tol = got[s]["frames"][-1], 1e-11 if name in ("fcc", "sc") else 1e-6   # (positions near 40 cells out: 1e-13 relative)
        n = lc.SIZES[s]
        assert (fr["n_neighbors"] == nb).all() and (fr["n_conn"] == nb).all() and (fr["solid"] == 1).all() and (fr["label"] == 0).all(), name
        assert np.abs(fr["ql"][:, 0] - q4).max() < tol and np.abs(fr["ql"][:, 1] - q6).max() < tol, name
        assert np.abs(fr["qbar"] - fr["ql"]).max() < 1e-11, name
        assert (got[s]["series_counts"] == [n, 1, n]).all() and np.abs(got[s]["series_order"][:, 0, :2] - [q4, q6]).max() < tol, name
    two, one = got[1]["frames"][-1], got[0]["frames"][-1]
    assert np.abs(two["ql"] - 1).max() < 1e-12 and (two["n_neighbors"] == 1).all() and (two["label"] == -1).all()
    assert (one["ql"] == 0).all() and (one["qbar"] == 0).all() and (one["qlm"] == 0).all() and one["n_neighbors"][0] == 0
    assert (got[0]["series_order"] == 0).all() and (got[0]["series_counts"] == 0).all() and got[0]["hist_q"][0, :, 0].tolist() == [5, 5, 5]


def test_bitwise_reproducible_alone_and_in_any_order():
    first = _full()
    second = _accumulate()
    for s in ALL:
        _same(first[s], second[s])
        _same(first[s], _accumulate(order=[s])[s])
    order = [4, 8, 2, 0, 6, 3, 1, 7, 5]
    permuted = _accumulate(order=order)
    for s in ALL:
        _same(first[s], permuted[s])


def test_captured_sample_replays_bitwise():
    """One lo_sample captured on static buffers, the five frames copied in and replayed: the counters are device-resident, so the
    replays equal five eager samples (the series cap is crossed in both)."""
    eager, graphed = _full(), _accumulate(graph=True)
    for s in ALL:
        _same(eager[s], graphed[s])
    assert eager[2]["n_samples"] == 5 and (eager[2]["series_order"] != 0).all()


def test_series_cap_and_the_overflow_structure():
    got = _full()
    dense = got[lc.NAMES.index("dense")]
    assert dense["flags"] == ref.NEIGHBORS and dense["n_samples"] == 0 and dense["n_skipped"] == lc.N_FRAMES
    for key in ("hist_q", "hist_qbar", "hist_nb", "moments", "series_counts", "series_order"):
        assert (dense[key] == 0).all(), key
    assert max(fr["n_neighbors"].max() for fr in dense["frames"]) > 32 and all(np.isfinite(fr["ql"]).all() for fr in dense["frames"])
    three = _accumulate(lc.SERIES_CAP)
    for s in lc.CLEAN:   # the series holds the first three samples and nothing of the later ones; the histograms hold all five
        assert np.array_equal(got[s]["series_counts"], three[s]["series_counts"]) and np.array_equal(got[s]["series_order"], three[s]["series_order"])
        assert got[s]["n_samples"] == 5 and three[s]["n_samples"] == 3 and got[s]["hist_nb"].sum() == 5 * lc.SIZES[s]


def _error_case(flag, others_same=True, **kw):
    """Three samples with the error input in all of them against three clean ones: structure 2 is flagged and skipped, the others
    untouched."""
    clean, out = _accumulate(3), _accumulate(3, **kw)
    bad = out[2]
    assert bad["flags"] & flag and bad["n_samples"] == 0 and bad["n_skipped"] == 3
    for key in ("hist_q", "hist_qbar", "hist_nb", "moments", "series_counts", "series_order"):
        assert (bad[key] == 0).all(), key
    for fr in bad["frames"]:   # nothing out of range
        assert ((fr["label"] >= -1) & (fr["label"] < lc.SIZES[2])).all() and (fr["n_neighbors"] >= 0).all() and (fr["n_conn"] >= 0).all()
        assert set(np.unique(fr["solid"])) <= {0, 1}
    for s in ALL:
        if s != 2:
            _same(clean[s], out[s])
    return out


def test_nan_position_is_flagged_and_stays_in_its_structure():
    b = lc.batch()
    pos = [p.copy() for p in b["pos"][:3]]
    for p in pos:
        p[b["offsets"][2] + 5, 1] = np.nan
    _error_case(ref.NONFINITE, pos=pos)


def test_singular_cell_is_flagged_and_left_out():
    b = lc.batch()
    bad = b["lats"].copy()
    bad[2, 1] = 0.0   # a cell without its second vector: det = 0
    out = _error_case(ref.CELL, lats=[bad] * 3)
    assert out[2]["flags"] == ref.CELL and all((fr["n_neighbors"] == 0).all() and (fr["ql"] == 0).all() for fr in out[2]["frames"])
    # one bad sample between good ones: the good ones count, the flag stays
    mixed = _accumulate(3, lats=[b["lats"], bad, b["lats"]])
    assert mixed[2]["flags"] == ref.CELL and mixed[2]["n_samples"] == 2 and mixed[2]["n_skipped"] == 1
    assert mixed[2]["hist_nb"].sum() == 2 * lc.SIZES[2] and np.isfinite(mixed[2]["moments"]).all()


def test_r_cut_beyond_half_the_width_is_flagged():
    width = ref.half_width(lc.batch()["lats"][2])
    out = _error_case(ref.RANGE, r_cut={2: width * 1.001})
    assert out[2]["flags"] & ref.RANGE
    fits = _accumulate(1, order=[8], r_cut={8: 0.5 * 4 * 2.6})   # exactly half the width of the simple-cubic cell: allowed
    assert fits[8]["flags"] == 0 and fits[8]["n_samples"] == 1


def test_one_shot_equals_init_sample_frame():
    from torch_m3gnet.local_order import local_order

    b = lc.batch()
    off = b["offsets"]
    order = [1, 2, 4, 7]
    got = _accumulate(1, order=order)
    res = local_order([b["lats"][s] for s in order], [b["pos"][0][off[s]:off[s + 1]] for s in order],
                      [np.array([13, 28, 29])[b["species"][s]] if s == 2 else np.full(lc.SIZES[s], 29) for s in order],
                      [lc.R_CUT[s] for s in order], lc.DEGREES, *lc.SOLID, device=DEV)
    for s, r in zip(order, res):
        fr = got[s]["frames"][0]
        for key in ("ql", "qbar", "n_neighbors", "n_conn", "solid", "label"):
            assert np.array_equal(r[key], fr[key]), (s, key)
        assert np.array_equal(r["qlm"], fr["qlm"])
        if s in lc.FLAGGED:
            assert r["flags"]["neighbors"] and r["n_solid"] is None and r["Q"] is None
        else:
            assert not any(r["flags"].values()) and [r["n_solid"], r["n_clusters"], r["largest_cluster"]] == list(got[s]["series_counts"][0])
            assert np.array_equal(r["Q"], got[s]["series_order"][0, 0]) and np.array_equal(r["mean_qbar"], got[s]["series_order"][0, 1])


def test_frame_before_any_sample_is_refused():
    st = _state([0, 1])
    with pytest.raises(ValueError, match="m3g_lo_frame: no sample has been taken"):
        st.frame()
    acc = st.read()
    assert all((acc[key] == 0).all() for key in ACC_KEYS)


def test_md_runs_with_local_order():
    from test_gpu_dynamics import _fcc, _fitted_model
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.local_order import LocalOrderObservables
    from torch_m3gnet.scattering import ScatteringObservables
    from torch_m3gnet.trajectory import TrajectoryObservables

    pos0, lat = _fcc(3.5, 2)
    pos = pos0 + np.random.default_rng(4).normal(0, 0.02, pos0.shape)
    z, m = np.full(32, 29), [np.full(32, 63.546)]
    lo = LocalOrderObservables({29: 3.0}, sample_interval=4, max_samples=4)
    md = MolecularDynamics(_fitted_model(), ensemble="nvt_langevin", timestep=1.0, temperature=300.0, seed=3)
    others = [TrajectoryObservables(rdf_bins=50, n_lags=8, sample_interval=2), ScatteringObservables(q_max=3.0, n_lags=8, sample_interval=2)]
    (plain,) = md.run([lat], [pos], [z], 20, masses=m, loginterval=5, observables=others)
    (both,) = md.run([lat], [pos], [z], 20, masses=m, loginterval=5, observables=others + [lo])
    assert "local_order" not in plain and np.array_equal(plain["positions"], both["positions"])
    assert np.array_equal(plain["scattering"]["s"], both["scattering"]["s"]) and "observables" in both
    npt = MolecularDynamics(_fitted_model(), ensemble="npt_mtk", timestep=1.0, temperature=300.0, pressure=0.0, seed=3)
    (moved,) = npt.run([lat], [pos], [z], 20, masses=m, loginterval=5, observables=lo)
    for res in (both, moved):
        r = res["local_order"]
        assert r["n_samples"] == 6 and r["n_skipped"] == 0 and not any(r["flags"].values()) and list(r["degrees"]) == [4, 6]
        assert list(r["step"]) == [0, 4, 8, 12] and r["Q"].shape == (4, 2) and r["q_mean"].shape == (1, 2)   # four series rows of six samples
        for key in ("q_mean", "q_var", "qbar_mean", "qbar_var", "q_hist", "qbar_hist", "coordination_hist", "Q", "mean_qbar", "solid_fraction"):
            assert np.isfinite(r[key]).all(), key
        assert np.isclose(r["coordination_hist"][0, 12], 1.0) and (r["n_solid"] == 32).all() and (r["largest_cluster"] == 32).all()
        assert abs(r["qbar_mean"][0, 1] - 0.5745) < 0.03 and r["frame"]["ql"].shape == (32, 2) and np.isfinite(r["frame"]["qlm"]).all()
    with pytest.raises(ValueError, match="observables are not supported with npt_mtk"):
        npt.run([lat], [pos], [z], 2, masses=m, observables=[lo, others[0]])
