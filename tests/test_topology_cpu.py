"""The topology restatement (tests/topology_reference.py) against brute-force definitions, the regimes its cases
(tests/topology_cases.py) are there for, and the layout hook m3g_debug_topology_layout.  CPU only: nothing here touches a device."""
import ctypes as C

import numpy as np
import pytest

import topology_cases as tc
import topology_reference as tr

SMALL = 25_000   # triplets up to which a case is also walked slot by slot in Python


# ------------------------------------------------------------------ the layout hook
def _layout(N, E, T, S, max_regions=64):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    off, n, b = (C.c_int64 * 64)(), (C.c_int64 * 64)(), (C.c_int32 * 64)()
    count = C.c_int32(-1)
    _lib.check(lib.m3g_debug_topology_layout(N, E, T, S, max_regions, off, n, b, C.byref(count)))
    k = min(count.value, max_regions)
    return count.value, list(off[:k]), list(n[:k]), list(b[:k])


@pytest.mark.parametrize("sizes", [(0, 0, 0, 0), (1, 0, 0, 1), (2, 2, 0, 1), (4, 168, 1224, 1), (64, 2688, 19584, 3), (150, 15644, 1623524, 1),
                                   (7, 127, 5, 2), (7, 128, 5, 2), (9, 255, 256, 1), (100_000, 4_200_000, 30_600_000, 50)])
def test_layout_hook_reports_the_documented_regions(sizes):
    """Regions in the order of struct Topo's carve, of the documented lengths and element sizes, none overlapping the next, the last
    documented byte inside m3g_topology_data_bytes <= m3g_topology_bytes."""
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    N, E, T, S = sizes
    count, off, n, b = _layout(*sizes)
    assert count == len(tr.REGIONS) == 25
    assert _layout(*sizes, max_regions=0) == (25, [], [], [])
    want = tr.documented_elems(N, E, T, S)
    assert n == [want[name] for name in tr.REGIONS]
    assert b == [1 if name in tr.BYTE_REGIONS else 4 for name in tr.REGIONS]
    assert off[0] == 0 and all(o % 256 == 0 for o in off)
    for i, name in enumerate(tr.REGIONS[:-1]):
        assert off[i] + n[i] * b[i] <= off[i + 1], f"{name} runs into {tr.REGIONS[i + 1]}"
    data, total = C.c_size_t(), C.c_size_t()
    _lib.check(lib.m3g_topology_data_bytes(N, E, T, S, C.byref(data)))
    _lib.check(lib.m3g_topology_bytes(N, E, T, S, C.byref(total)))
    assert off[-1] + n[-1] * b[-1] <= data.value <= total.value


def test_layout_hook_rejects_bad_arguments():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    count = C.c_int32()
    assert lib.m3g_debug_topology_layout(1, 1, 1, 1, 4, None, None, None, C.byref(count)) != 0
    assert lib.m3g_debug_topology_layout(1, 1, 1, 1, 0, None, None, None, None) != 0
    assert lib.m3g_debug_topology_layout(-1, 1, 1, 1, 0, None, None, None, C.byref(count)) != 0


# ------------------------------------------------------------------ the regimes
def _hints_rows(word):
    return (word >> 8) & 0xFF


def _hints_atoms(word):
    return (word >> 16) & 0xFF


def test_every_regime_of_the_table_is_reached():
    """From the restatement alone: each case is in the regime it is named for (figures as measured with the host builder)."""
    c, r = tc.case("fcc 1x1x1"), tc.reference("fcc 1x1x1")
    assert r["A"] == 72 and len(tc.window_rows(r)) == 1 and r["hints"] & 1

    c, r = tc.case("fcc 2x2x4"), tc.reference("fcc 2x2x4")
    assert r["A"] == 1152 == 9 * tr.kTbRows and tc.window_rows(r).tolist() == [144] * 9
    win = r["tb_win"].reshape(-1, 6)
    assert len(win) > 9 and not win[9].any() and win[8].any()   # the record after the last window exists and reads as empty

    c, r = tc.case("fcc 4x4x4"), tc.reference("fcc 4x4x4")
    assert (c.E, c.T) == (10_752, 78_336) and len(tc.window_rows(r)) == 36

    c, r = tc.case("400 atoms in 30 A"), tc.reference("400 atoms in 30 A")
    fast = r["tb_fast"].reshape(-1, 2)
    assert tc.window_atoms(r).max() == 192 and len(tc.window_rows(r)) == 3 and int((fast[:3, 0] == 0).sum()) == 2
    assert r["flags"][4] == 2 and r["hints"] == 0

    c, r = tc.case("300 atoms in 24 A"), tc.reference("300 atoms in 24 A")
    assert tc.window_atoms(r).max() == tr.kTbFastAtoms == 64 and r["flags"][4] == 0 and _hints_atoms(r["hints"]) == 64

    c, r = tc.case("150 atoms in 10 A"), tc.reference("150 atoms in 10 A")
    rows = tc.window_rows(r)
    assert c.T == 1_623_524 and rows.max() == 328 and len(rows) == 123 and r["flags"][4] == 26 and r["hints"] == 0
    assert int((rows > tr.kTbCap).sum()) == 26 and (r["t1_b"] == 255).any() and (r["t2_b"] == 255).any()
    assert r["flags"][5] <= tr.kTbCap   # the certificate's maxima are over the windows that may use the moment path

    c, r = tc.case("24 atoms in 6.5 A"), tc.reference("24 atoms in 6.5 A")
    rows = tc.window_rows(r)
    assert c.T <= 24 * c.E and int(((rows >= 193) & (rows <= 255)).sum()) == 5 and rows.max() == 206
    assert r["flags"][4] == 0 and _hints_rows(r["hints"]) == 206
    for b in (r["t1_b"], r["t2_b"]):
        assert int(((b >= 192) & (b < 255)).sum()) > 100   # byte ids at or beyond the 192 rows the short-list kernels stage

    c, r = tc.case("idle atoms"), tc.reference("idle atoms")
    rows_of = np.diff(r["arow_ptr"])
    t_of = np.bincount(c.batch[c.edge_index[0][c.triplet_edge_index[0]]], minlength=c.S)
    assert t_of.tolist()[0::2] == [0, 0, 0] and all(t > 0 for t in t_of.tolist()[1::2])
    first, last = np.searchsorted(c.batch, 1), np.searchsorted(c.batch, 2) - 1
    idle = np.nonzero(rows_of[first:last + 1] == 0)[0].tolist()
    assert {0, 7, 14} <= set(idle) and last - first == 14 and len(idle) < 8   # start, middle and end of the second structure

    assert 64 < tc.case("7 atoms, rows of ~150").longest_row <= tc.kInStage
    assert tc.case("7 atoms, rows of ~590").longest_row > tc.kInStage
    c = tc.case("no edges")
    assert c.E == 0 and c.T == 0 and c.N == 2
    c = tc.case("dimer")
    assert c.E == 2 and c.T == 0 and tc.reference("dimer")["A"] == 0
    c = tc.case("one atom")
    assert c.N == 1 and c.T > 0

    r = tc.reference("one pair twice")
    keys = (r["t1_e2"].astype(np.int64) << 32) | np.repeat(np.arange(tc.case("one pair twice").E), np.diff(r["t1_ptr"]))
    assert len(np.unique(keys)) == len(keys) - 1
    r = tc.reference("unsorted batch")
    assert r["struct_ptr"] is None and r["flags"][3] != 0
    c, r = tc.case("triplets one-sided"), tc.reference("triplets one-sided")
    t1_rows, t2_rows = np.diff(r["t1_ptr"]) > 0, np.diff(r["t2_ptr"]) > 0
    assert (t2_rows & ~t1_rows).any()   # edges that only ever appear as the partner e2 are active all the same
    assert np.array_equal(r["act_id"] >= 0, t1_rows | t2_rows)
    assert not tc.reference("triplets thinned")["row_complete"].all() and tc.reference("triplets thinned")["hints"] == 0
    assert not tc.case("multigraph").canonical and len(np.unique(tc.case("multigraph").edge_index, axis=1)) < tc.case("multigraph").E
    assert tc.window_rows(tc.reference("dense cell")).max() > tr.kTbCap


def test_every_branch_of_the_build_is_reached():
    want = {"fcc 4x4x4": "optimistic", "triplets shuffled": "sorted again", "triplets one-sided": "one-sided second sort",
            "one pair twice": "one-sided second sort", "shuffled and one-sided": "sorted again, one-sided second sort",
            "asymmetric edge list": "in-edge sort fallback", "7 atoms, rows of ~590": "in-edge sort fallback", "dimer": "no triplets",
            "no edges": "no triplets", "multigraph": "optimistic"}
    for name, branch in want.items():
        assert tc.case(name).branch == branch, (name, tc.case(name).branch)
    assert not tc.case("asymmetric edge list").edges_symmetric
    fast = {name: tc.case(name).fast_build_applies for name in tc.NAMES if tc.case(name).canonical}
    assert fast["fcc 1x1x1"] and fast["idle atoms"] and fast["150 atoms in 10 A"]
    assert not fast["7 atoms, rows of ~590"] and not fast["dimer"] and not fast["no edges"]
    kinds = [tc.CASES[f"random batch {s}"][0].split(": ")[1] for s in range(tc.N_RANDOM)]
    assert tc.N_RANDOM == 20 and {k: kinds.count(k) for k in tc.PERTURBATIONS} == dict.fromkeys(tc.PERTURBATIONS, 5)
    for s in range(tc.N_RANDOM):
        c = tc.case(f"random batch {s}")
        assert c.E > 0 and c.T <= 200_000


# ------------------------------------------------------------------ the restatement against brute force
def _brute_force(c, r):
    """Every derived array from its definition, slot by slot (small cases)."""
    E, T, N = c.E, c.T, c.N
    ei, tei = c.edge_index, c.triplet_edge_index
    src, dst = ei[0], ei[1]
    assert np.array_equal(r["src"], src) and np.array_equal(r["dst"], dst)
    for i in range(N + 1):
        assert r["row_ptr"][i] == int((src < i).sum()) and r["in_ptr"][i] == int((dst < i).sum())
    # by-neighbour list: grouped by neighbour, ascending edge id inside, and its inverse
    in_edge, in_pos = r["in_edge"], r["in_pos"]
    assert sorted(in_edge.tolist()) == list(range(E))
    for j in range(N):
        assert in_edge[r["in_ptr"][j]: r["in_ptr"][j + 1]].tolist() == [e for e in range(E) if dst[e] == j]
    assert np.array_equal(in_edge[in_pos], np.arange(E))
    # every triplet sits once in t1 and once in t2
    pairs = sorted(zip(tei[0].tolist(), tei[1].tolist()))
    t1 = [(e, int(p)) for e in range(E) for p in r["t1_e2"][r["t1_ptr"][e]: r["t1_ptr"][e + 1]]]
    t2 = [(int(p), e) for e in range(E) for p in r["t2_e1"][r["t2_ptr"][e]: r["t2_ptr"][e + 1]]]
    assert t1 == pairs and sorted(t2) == pairs and len(t1) == T
    assert t2 == sorted(t2, key=lambda p: (p[1], p[0]))
    assert r["t1_ptr"][0] == 0 == r["t2_ptr"][0] and r["t1_ptr"][E] == T == r["t2_ptr"][E]
    # active edges
    active = sorted(set(tei[0].tolist()) | set(tei[1].tolist()))
    A = len(active)
    assert r["A"] == A == r["flags"][2] and r["act_list"].tolist() == active
    cid = {e: k for k, e in enumerate(active)}
    assert r["act_id"].tolist() == [cid.get(e, -1) for e in range(E)]
    assert r["act_scan"].tolist() == [sum(1 for a in active if a < e) for e in range(E + 1)]
    assert r["act_dst"].tolist() == [int(dst[e]) for e in active]
    assert r["arow_ptr"].tolist() == [sum(1 for a in active if src[a] < i) for i in range(N + 1)]
    assert r["in_pair"].reshape(-1, 2).tolist() == [[int(e), cid.get(int(e), -1)] for e in in_edge]
    assert r["t1_e2c"].tolist() == [cid[int(e)] for e in r["t1_e2"]] and r["t2_e1c"].tolist() == [cid[int(e)] for e in r["t2_e1"]]
    # a window holds exactly the active rows of the centres its 128 rows touch
    win = r["tb_win"].reshape(-1, 6)
    assert len(win) == E // 128 + 1
    centre = [int(src[e]) for e in active]
    for b in range(len(win)):
        mine = list(range(128 * b, min(128 * b + 128, A)))
        if not mine:
            assert not win[b].any()
            continue
        touched = {centre[q] for q in mine}
        rows = [q for q in range(A) if centre[q] in touched]
        assert rows == list(range(win[b, 0], win[b, 1])), b
        first, last = active[mine[0]], active[mine[-1]]
        assert win[b, 2:].tolist() == [r["t1_ptr"][first], r["t1_ptr"][last + 1], r["t2_ptr"][first], r["t2_ptr"][last + 1]]
    # byte-sized partner ids
    for ptr, other, got in ((r["t1_ptr"], r["t1_e2c"], r["t1_b"]), (r["t2_ptr"], r["t2_e1c"], r["t2_b"])):
        want = np.empty(T, dtype=np.uint8)
        for e in active:
            lo, hi = (int(x) for x in win[cid[e] // 128, :2])
            for t in range(ptr[e], ptr[e + 1]):
                d = int(other[t]) - lo
                want[t] = d if 0 <= d < min(hi - lo, 255) else 255
        assert np.array_equal(got, want)
    # completeness by set comparison, then the certificate
    complete = []
    for q, e in enumerate(active):
        others = {k for k in range(A) if centre[k] == centre[q]} - {q}
        ok = True
        for ptr, other in ((r["t1_ptr"], r["t1_e2c"]), (r["t2_ptr"], r["t2_e1c"])):
            mine = other[ptr[e]: ptr[e + 1]].tolist()
            ok = ok and set(mine) == others and len(mine) == len(others) and mine == sorted(mine)
        complete.append(ok)
    assert r["row_complete"].tolist() == complete
    fast = r["tb_fast"].reshape(-1, 2)
    bad = rows = atoms = 0
    for b in range(len(win)):
        lo, hi = int(win[b, 0]), int(win[b, 1])
        if 128 * b >= A:
            assert fast[b].tolist() == [0, 0]
            continue
        na = centre[hi - 1] - centre[lo] + 1
        if na <= 64 and hi - lo <= 255 and all(complete[lo:hi]):
            assert fast[b].tolist() == [na, centre[lo]]
            rows, atoms = max(rows, hi - lo), max(atoms, na)
        else:
            assert fast[b].tolist() == [0, centre[lo]]
            bad += 1
    word = (1 | (rows << 8) | (atoms << 16)) if bad == 0 and rows > 0 else 0
    assert r["flags"].tolist() == [0, 0, A, int(bool(np.any(np.diff(c.batch) < 0))), bad, rows, atoms, word] + [0] * 8
    assert r["hints"] == word
    assert np.array_equal(r["batch"], c.batch)
    if r["struct_ptr"] is not None:
        assert r["struct_ptr"].tolist() == [int((c.batch < s).sum()) for s in range(c.S + 1)]
    bare = tr.without_certificate(r)
    assert not bare["tb_fast"].any() and not bare["flags"][4:8].any() and bare["hints"] == 0 and bare["flags"][2] == A


@pytest.mark.parametrize("name", tc.NAMES)
def test_restatement_against_brute_force_definitions(name):
    c = tc.case(name)
    r = tc.reference(name)
    want = tr.documented_elems(c.N, c.E, c.T, c.S)
    for region in tr.REGIONS:
        if r[region] is None:
            continue
        n = r["A"] if region in ("act_list", "act_dst") else want[region]
        assert len(r[region]) == n, region
        assert r[region].dtype == (np.uint8 if region in tr.BYTE_REGIONS else np.int32), region
    assert tr.first_mismatch(r, r) is None
    if c.T <= SMALL and c.E <= 4000:
        _brute_force(c, r)
    else:   # the properties that need no walk
        assert np.array_equal(r["in_edge"][r["in_pos"]], np.arange(c.E))
        for ptr, low, first, second in ((r["t1_ptr"], r["t1_e2"], 0, 1), (r["t2_ptr"], r["t2_e1"], 1, 0)):
            row = np.repeat(np.arange(c.E), np.diff(ptr))
            got = np.sort((row.astype(np.int64) << 32) | low)
            tei = c.triplet_edge_index
            assert np.array_equal(got, np.sort((tei[first] << 32) | tei[second]))


def test_first_mismatch_names_region_index_and_values():
    r = tc.reference("fcc 1x1x1")
    dev = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    dev["t2_b"][5] ^= 1
    assert tr.first_mismatch(dev, r) == ("t2_b", 5, int(dev["t2_b"][5]), int(r["t2_b"][5]))
    dev["tb_win"][1] += 1   # an off-by-one in a window's hi comes first in the buffer's order
    assert tr.first_mismatch(dev, r)[:2] == ("tb_win", 1)
