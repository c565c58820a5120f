"""The topology buffer restated on the host: every array of `struct Topo` (csrc/m3g_internal.h) from the index tensors, in plain
numpy on integers only (checker plumbing, CPU only).

`restate(N, S, edge_index, triplet_edge_index, batch)` follows the comments of `struct Topo` and nothing of csrc/m3g_topology.hip:
sorts are numpy's, lower bounds are `searchsorted`, and each derived array is written from its definition.  It returns
{region name: array of the documented length}, the regions of m3g_debug_topology_layout in its order (REGIONS), plus the scalars
"A" and "hints".  `tb_fast` and `flags[4..7]` are the certificate (m3g_topology_hints); `without_certificate` gives what a bare
m3g_topology_build leaves.  tests/test_topology_cpu.py pins this file against brute-force definitions on the small cases,
tests/test_gpu_topology.py holds the device against it."""
from __future__ import annotations

import numpy as np

kTbRows = 128        # compacted rows per three-body workgroup
kTbCap = 255         # most rows of a staged window: a window-relative partner id fits a byte, 255 = "outside"
kTbFastAtoms = 64    # most centre atoms of a window that may use the moment path
kTopoFlags = 16
TOPO_TB_COMPLETE = 1

REGIONS = ("src", "dst", "row_ptr", "in_ptr", "in_edge", "in_pair", "in_pos", "t1_ptr", "t1_e2", "t2_ptr", "t2_e1", "act_list",
           "act_scan", "act_id", "arow_ptr", "act_dst", "tb_win", "tb_fast", "t1_e2c", "t2_e1c", "t1_b", "t2_b", "batch", "struct_ptr",
           "flags")
BYTE_REGIONS = ("t1_b", "t2_b")


def tb_win_blocks(E: int) -> int:
    return E // kTbRows + 1


def documented_elems(N: int, E: int, T: int, S: int) -> dict:
    """{region: documented length} as m3g_debug_topology_layout reports it (act_list and act_dst: their capacity E, of which A are
    written)."""
    W = tb_win_blocks(E)
    return dict(src=E, dst=E, row_ptr=N + 1, in_ptr=N + 1, in_edge=E, in_pair=2 * E, in_pos=E, t1_ptr=E + 1, t1_e2=T, t2_ptr=E + 1,
                t2_e1=T, act_list=E, act_scan=E + 1, act_id=E, arow_ptr=N + 1, act_dst=E, tb_win=6 * W, tb_fast=2 * W, t1_e2c=T,
                t2_e1c=T, t1_b=T, t2_b=T, batch=N, struct_ptr=S + 1, flags=kTopoFlags)


def hints_word(bad: int, rows: int, atoms: int) -> int:
    """topo_hints_word (csrc/m3g_step_path.h): 0 unless every window with rows may use the moment path."""
    if bad != 0 or rows <= 0:
        return 0
    return TOPO_TB_COMPLETE | ((rows & 0xFF) << 8) | ((atoms & 0xFF) << 16)


def _grouped(first, second, E):
    """Triplets grouped by `first`: (ptr [E+1], partner [T], row of each slot [T]) from the sorted keys (first << 32) | second."""
    keys = np.sort((first.astype(np.uint64) << np.uint64(32)) | second.astype(np.uint64), kind="stable")
    high = (keys >> np.uint64(32)).astype(np.int64)
    ptr = np.searchsorted(high, np.arange(E + 1), side="left")
    return ptr.astype(np.int32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int32), high


def _rows_complete(A, ptr, slot_row, other_c, act_list, act_id, src, arow_ptr):
    """ok[r]: the partner list (ptr, other_c) of compacted row r holds every other compacted row of its centre exactly once, ascending."""
    ok = np.zeros(A, dtype=bool)
    if A == 0:
        return ok
    e = act_list.astype(np.int64)
    c = src[e].astype(np.int64)
    s0, s1 = arow_ptr[c].astype(np.int64), arow_ptr[c + 1].astype(np.int64)
    count = ptr[e + 1].astype(np.int64) - ptr[e]
    ok = count == s1 - s0 - 1
    # slot t is the k-th of its row r: complete means it holds the k-th element of [s0, s1) without r
    r = act_id[slot_row].astype(np.int64)
    k = np.arange(len(slot_row), dtype=np.int64) - ptr[slot_row]
    want = s0[r] + k
    want = want + (want >= r)
    wrong = np.bincount(r[other_c != want], minlength=A) > 0
    return ok & ~wrong


def restate(N, S, edge_index, triplet_edge_index, batch):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    tei = np.asarray(triplet_edge_index, dtype=np.int64).reshape(2, -1)
    batch = np.asarray(batch, dtype=np.int64).reshape(-1)
    N, S, E, T = int(N), int(S), ei.shape[1], tei.shape[1]
    assert batch.shape[0] == N
    assert E == 0 or (ei.min() >= 0 and ei.max() < N and np.all(np.diff(ei[0]) >= 0)), "edge list out of range or not sorted by centre"
    assert T == 0 or (tei.min() >= 0 and tei.max() < E and np.array_equal(ei[0][tei[0]], ei[0][tei[1]])), "malformed triplet list"
    out = {}
    src, dst = ei[0].astype(np.int32), ei[1].astype(np.int32)
    out["src"], out["dst"] = src, dst
    row_ptr = np.searchsorted(src, np.arange(N + 1), side="left").astype(np.int32)
    out["row_ptr"] = row_ptr
    in_edge = np.argsort(dst, kind="stable").astype(np.int32)
    out["in_edge"] = in_edge
    out["in_ptr"] = np.searchsorted(dst[in_edge], np.arange(N + 1), side="left").astype(np.int32)
    in_pos = np.empty(E, dtype=np.int32)
    in_pos[in_edge] = np.arange(E, dtype=np.int32)
    out["in_pos"] = in_pos

    t1_ptr, t1_e2, t1_row = _grouped(tei[0], tei[1], E)
    t2_ptr, t2_e1, t2_row = _grouped(tei[1], tei[0], E)
    out.update(t1_ptr=t1_ptr, t1_e2=t1_e2, t2_ptr=t2_ptr, t2_e1=t2_e1)

    active = np.zeros(E, dtype=bool)
    active[tei[0]] = True
    active[tei[1]] = True
    act_scan = np.concatenate([[0], np.cumsum(active)]).astype(np.int32)   # [E+1], exclusive
    A = int(act_scan[E])
    act_id = np.where(active, act_scan[:E], -1).astype(np.int32)
    act_list = np.nonzero(active)[0].astype(np.int32)
    arow_ptr = act_scan[row_ptr]
    out.update(act_list=act_list, act_scan=act_scan, act_id=act_id, arow_ptr=arow_ptr, act_dst=dst[act_list])
    out["in_pair"] = np.stack([in_edge, act_id[in_edge]], axis=1).reshape(-1).astype(np.int32)
    t1_e2c, t2_e1c = act_scan[t1_e2], act_scan[t2_e1]
    out.update(t1_e2c=t1_e2c, t2_e1c=t2_e1c)

    W = tb_win_blocks(E)
    win = np.zeros((W, 6), dtype=np.int32)
    for b in range(W):
        if kTbRows * b >= A:
            continue
        ef, el = int(act_list[kTbRows * b]), int(act_list[min(kTbRows * b + kTbRows - 1, A - 1)])
        win[b] = (arow_ptr[src[ef]], arow_ptr[src[el] + 1], t1_ptr[ef], t1_ptr[el + 1], t2_ptr[ef], t2_ptr[el + 1])
    out["tb_win"] = win.reshape(-1)

    def partner_bytes(slot_row, other_c):
        blk = act_id[slot_row].astype(np.int64) // kTbRows
        lo, hi = win[blk, 0].astype(np.int64), win[blk, 1].astype(np.int64)
        d = other_c.astype(np.int64) - lo
        inside = (d >= 0) & (d < np.minimum(hi - lo, kTbCap))
        return np.where(inside, d, 255).astype(np.uint8)

    out["t1_b"], out["t2_b"] = partner_bytes(t1_row, t1_e2c), partner_bytes(t2_row, t2_e1c)

    # the certificate
    ok = (_rows_complete(A, t1_ptr, t1_row, t1_e2c, act_list, act_id, src, arow_ptr)
          & _rows_complete(A, t2_ptr, t2_row, t2_e1c, act_list, act_id, src, arow_ptr))
    fast = np.zeros((W, 2), dtype=np.int32)
    bad = rows = atoms = 0
    for b in range(W):
        if kTbRows * b >= A:
            continue
        lo, hi = int(win[b, 0]), int(win[b, 1])
        assert 0 <= lo < hi <= A    # a window of a well-formed graph has rows
        a0 = int(src[act_list[lo]])
        na = int(src[act_list[hi - 1]]) - a0 + 1
        if na <= kTbFastAtoms and hi - lo <= kTbCap and bool(ok[lo:hi].all()):
            fast[b] = (na, a0)
            rows, atoms = max(rows, hi - lo), max(atoms, na)
        else:
            fast[b] = (0, a0)
            bad += 1
    out["tb_fast"] = fast.reshape(-1)
    out["row_complete"] = ok   # (not a region: for the brute-force comparison)

    out["batch"] = batch.astype(np.int32)
    unsorted = bool(np.any(np.diff(batch) < 0))
    out["struct_ptr"] = None if unsorted else np.searchsorted(batch, np.arange(S + 1), side="left").astype(np.int32)
    word = hints_word(bad, rows, atoms)
    flags = np.zeros(kTopoFlags, dtype=np.int32)
    flags[2], flags[3] = A, int(unsorted)
    flags[4:8] = (bad, rows, atoms, word)
    out["flags"] = flags
    out["A"], out["hints"] = A, word
    return out


def without_certificate(ref: dict) -> dict:
    """What m3g_topology_build leaves: the same arrays, no window may use the moment path, flags[4..7] == 0, hints 0."""
    out = dict(ref)
    out["tb_fast"] = np.zeros_like(ref["tb_fast"])
    flags = ref["flags"].copy()
    flags[4:8] = 0
    out["flags"] = flags
    out["hints"] = 0
    return out


def first_mismatch(device: dict, ref: dict):
    """(region, index, device value, reference value) of the first documented element that differs, None when there is none.  `device`
    holds each region at (at least) its documented length; flags[3] is compared as a truth value, an unspecified region (None) is skipped."""
    for name in REGIONS:
        want = ref[name]
        if want is None:
            continue
        got = np.asarray(device[name])[: len(want)]
        if len(got) != len(want):
            return name, len(got), None, None
        if name == "flags":
            got, want = got.copy(), want.copy()
            got[3], want[3] = got[3] != 0, want[3] != 0
        bad = np.nonzero(got != want)[0]
        if len(bad):
            i = int(bad[0])
            return name, i, int(got[i]), int(want[i])
    return None
